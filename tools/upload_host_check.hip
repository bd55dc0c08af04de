// upload_host_check.hip -- the host side of upload under a sanitizer, without a device.
//
// A stand-alone program (its own main; never loaded into python, never run on a GPU): the source object and the handle
// guard of upload_ops.hpp on plain host memory, then the no-device paths of the library -- the two plan checks and the
// argument refusals of the uploads before spmv_hip_init().  Built by `make -C sparsematrixvectormultiplication_amd/csrc
// upload_host_check`: this file and the upload translation units with -fsanitize=address,undefined on the host side,
// linked with the library's other objects.  Exit status 0 and "upload_host_check ok": nothing failed, and the
// sanitizers had nothing to say.
#include <cstdio>
#include <cstring>
#include <vector>

#include "upload_ops.hpp"

#include "hll_matrix.h"

static int g_failed = 0;
#define CHECK(cond)                                                         \
    do {                                                                    \
        if (!(cond)) {                                                      \
            fprintf(stderr, "%s:%d: %s is false\n", __FILE__, __LINE__, #cond); \
            ++g_failed;                                                     \
        }                                                                   \
    } while (0)

struct Handle {
    int *col = nullptr;
    double *val = nullptr;
};
static int g_freed = 0;
static void free_handle(Handle *h) {
    ++g_freed;
    delete h;
}

// the addresses stand in for device arrays: the source stores and compares them and never reads through them
static void check_source_and_guard() {
    int d_col[4] = {0, 1, 2, 3};
    double d_val[4] = {1, 2, 3, 4};
    const MatrixSource<double> from = MatrixSource<double>::adopting(d_col, d_val);
    {  // a failed upload: the adopted arrays leave the handle before the guard frees it
        Handle *seen = nullptr;
        {
            HandleGuard<Handle, free_handle> guard(new Handle());
            seen = guard.h;
            MatrixSource<double> src(from);
            src.bind(&guard.h->col, &guard.h->val, 0, 4, 0);
            CHECK(guard.h->col == d_col && guard.h->val == d_val && src.on_device() && !src.on_host());
            CHECK(src.col.device_view() == 0 && src.val.device_view() == 0);  // there already: no upload
        }
        CHECK(g_freed == 1 && seen != nullptr);
    }
    {  // a finished upload: the handle keeps them and the guard lets go
        Handle *h = nullptr;
        {
            HandleGuard<Handle, free_handle> guard(new Handle());
            MatrixSource<double> src(from);
            src.bind(&guard.h->col, &guard.h->val, 0, 4, 0);
            src.keep();
            h = guard.release();
        }
        CHECK(g_freed == 1 && h && h->col == d_col && h->val == d_val);
        delete h;
    }
    {  // host arrays: the host view is the caller's window, and no copy is made
        const int col[6] = {5, 4, 3, 2, 1, 0};
        const double val[6] = {0, 1, 2, 3, 4, 5};
        Handle h;
        MatrixSource<double> src = MatrixSource<double>::on_host(col, val);
        src.bind(&h.col, &h.val, 2, 3, 8);
        CHECK(src.on_host() && !src.on_device() && src.col.count == 3 && src.col.pad == 8);
        CHECK(src.col.host_view("unused") == col + 2 && src.val.host_view("unused") == val + 2 && src.col.back.empty());
    }
    CHECK(lanes_for_mean_row(0.0) == 2 && lanes_for_mean_row(9.0) == 4 && lanes_for_mean_row(1e9) == 32);
}

static void check_library_without_device() {
    // a band of 300 rows, 5 per row
    const int M = 300, N = 300;
    std::vector<int> rp(1, 0), col;
    for (int r = 0; r < M; ++r) {
        for (int c = r - 2; c <= r + 2; ++c)
            if (c >= 0 && c < N) col.push_back(c);
        rp.push_back((int)col.size());
    }
    std::vector<double> val(col.size(), 0.5);
    int stats[6] = {0};
    CHECK(spmv_hip_csr_plan_check(M, N, rp.data(), col.data(), 8, stats) == 0 && stats[1] > 0);
    CHECK(spmv_hip_csr_plan_check(M, N, rp.data(), col.data(), 4, stats) == 0 && stats[1] > 0);
    CHECK(spmv_hip_csr_plan_check(M, N, nullptr, col.data(), 8, stats) == -1);
    col[7] = N;  // a column out of range
    CHECK(spmv_hip_csr_plan_check(M, N, rp.data(), col.data(), 8, stats) == -1 && strstr(spmv_hip_last_error(), "outside"));
    col[7] = 1;

    // the same matrix as hacks of 32 rows, 5 slots per row
    const int H = (M + 31) / 32;
    std::vector<std::vector<int>> ja((size_t)H);
    std::vector<std::vector<double>> as((size_t)H);
    std::vector<ELLPACKBlock> blocks((size_t)H);
    for (int h = 0; h < H; ++h) {
        const int rows = std::min(32, M - 32 * h);
        ja[h].assign((size_t)rows * 5, 0);
        as[h].assign((size_t)rows * 5, 0.0);
        for (int i = 0; i < rows; ++i) {
            const int r = 32 * h + i;
            for (int e = rp[r], k = 0; e < rp[r + 1]; ++e, ++k) {
                ja[h][(size_t)i * 5 + k] = col[e];
                as[h][(size_t)i * 5 + k] = val[e];
            }
        }
        blocks[h].M = rows;
        blocks[h].N = N;
        blocks[h].MAXNZ = 5;
        blocks[h].JA = ja[h].data();
        blocks[h].AS = as[h].data();
    }
    HLLMatrix hll;
    hll.num_blocks = H;
    hll.blocks = blocks.data();
    int hstats[4] = {0};
    CHECK(spmv_hip_hll_plan_check(&hll, M, N, hstats) == 0 && hstats[0] > 0 && hstats[1] > 0);
    CHECK(spmv_hip_hll_plan_check(&hll, M + 40, N, hstats) == -1);
    CHECK(spmv_hip_hll_plan_check(nullptr, M, N, hstats) == -1);

    // the uploads refuse: NULL arguments by name, everything else for want of spmv_hip_init()
    spmv_csr_dev *c = nullptr;
    spmv_hll_dev *l = nullptr;
    CHECK(spmv_hip_csr_upload_matrix(nullptr, &c) == -1 && strstr(spmv_hip_last_error(), "NULL") && !c);
    CHECK(spmv_hip_hll_upload(nullptr, M, N, &l) == -1 && strstr(spmv_hip_last_error(), "NULL") && !l);
    CHECK(spmv_hip_csr_upload(M, N, rp.data(), col.data(), val.data(), 0, M, &c) == -1 && !c);
    CHECK(spmv_hip_csr_upload(M, N, nullptr, nullptr, nullptr, 0, M, nullptr) == -1);
    CHECK(spmv_hip_hll_upload_part(&hll, M, N, 0, H, &l) == -1 && !l);
    CHECK(spmv_hip_hll_from_csr(nullptr, &l) == -1 && !l);
}

int main() {
    check_source_and_guard();
    check_library_without_device();
    if (g_failed) {
        fprintf(stderr, "upload_host_check: %d checks failed\n", g_failed);
        return 1;
    }
    puts("upload_host_check ok");
    return 0;
}
