// fsai_kernels.hpp -- the device build of the FSAI factor G (spmv_fsai.hip launches it; host/fsai_plan.c chose the
// patterns and the lane widths) (gfx950).
//
// Row i of G has the pattern S = S_i (m columns ascending, i last) and is the solution of C^T g = e_last with
// C C^T = A~[S, S], A~ the symmetric matrix whose lower triangle is the canonical block's.  fsai_rows<T, W> builds the
// rows of one lane width W (the smallest power of two >= m, at least 4): W lanes per row, 64 / W rows per wavefront,
// lane a owns row a of the local matrix.
//
//   gather   the m (m + 1) / 2 entries (a, b), b <= a, dealt out to the W lanes: column S[b] by binary search in
//            canonical row S[a] (0 when the row does not store it)
//   factor   right-looking Cholesky in place: at step k the lanes a > k scale column k by 1 / sqrt(pivot), then lane a
//            updates its row's entries (a, b), k < b <= a, by one fma each; an entry's updates come in ascending k.  A
//            pivot that is not positive or not finite marks the row bad (status 1)
//   solve    g_b = (e_last[b] - sum_{a > b} C[a][b] g_a) / C[b][b] for b = m - 1 .. 0: the products of the lanes a > b
//            are added by a butterfly over the W lanes (a fixed tree), lane b divides
//   store    g rounded once to T into G's values; a rounded value that is not finite marks the row (status 2)
//
// The LDS tile: entry (a, b) of the row built by lanes [t0, t0 + W) of the workgroup sits at tile[b][t0 + a], so the
// W^2 doubles of a row's tile interleave with those of the workgroup's other rows: at a fixed b the kFsaiBlock lanes
// read or write kFsaiBlock consecutive doubles (every 32-lane half a whole 256-byte bank row: no conflict at any W),
// and a read of column k's entry b by all lanes of a row is one address per row (a broadcast), W doubles apart between
// rows.  W = 32: 32 x 32 doubles = 8 KiB per row, 32 KiB per workgroup.
//
// fp64 throughout, no atomics, nothing waits for another workgroup: two builds give the same bytes.  Every loop that
// holds a barrier or a shuffle runs W times on every lane; m only masks the work.
#pragma once
#include <hip/hip_runtime.h>

namespace spmv {

constexpr int kFsaiMaxCap = 32;      // the largest pattern: one row per 32 lanes
constexpr int kFsaiBlock = 128;      // threads per workgroup: 128 / W rows
constexpr int kFsaiMaxGrid = 1 << 20;  // grid cap (the workgroups stride beyond it)

// rows[count]: the rows of width W.  a_*: the canonical block (fp64).  g_rp / g_col: G's pattern; g_val: its values.
// status[n]: zeroed by the caller; 1 = a bad pivot, 2 = a value of G that is not finite in T
template <typename T, int W>
__global__ __launch_bounds__(kFsaiBlock) void fsai_rows(int count, const int *__restrict__ rows,
                                                        const int *__restrict__ a_rp, const int *__restrict__ a_col,
                                                        const double *__restrict__ a_val,
                                                        const int *__restrict__ g_rp, const int *__restrict__ g_col,
                                                        T *__restrict__ g_val, int *__restrict__ status) {
    static_assert(W >= 4 && W <= kFsaiMaxCap && (W & (W - 1)) == 0, "a row's lanes lie in one wavefront half");
    __shared__ double tile[W][kFsaiBlock];
    constexpr int kRows = kFsaiBlock / W;
    const int tid = threadIdx.x, a = tid % W, t0 = tid - a;
    for (long long first = (long long)blockIdx.x * kRows; first < count; first += (long long)gridDim.x * kRows) {
        const long long which = first + tid / W;
        const bool have = which < count;
        const int i = have ? rows[which] : 0;
        const int g0 = have ? g_rp[i] : 0;
        const int m = have ? g_rp[i + 1] - g0 : 0;
        __syncthreads();  // the previous rows' tiles have been read
        for (int t = a; t < m * (m + 1) / 2; t += W) {
            int pa = (int)((sqrtf(8.0f * (float)t + 1.0f) - 1.0f) * 0.5f);  // t = pa (pa + 1) / 2 + pb, pb <= pa
            while (pa * (pa + 1) / 2 > t) --pa;
            while ((pa + 1) * (pa + 2) / 2 <= t) ++pa;
            const int pb = t - pa * (pa + 1) / 2;
            const int r = g_col[g0 + pa], c = g_col[g0 + pb];
            const int end = a_rp[r + 1];
            int lo = a_rp[r], hi = end;
            while (lo < hi) {
                const int mid = lo + ((hi - lo) >> 1);
                if (a_col[mid] < c) lo = mid + 1;
                else hi = mid;
            }
            tile[pb][t0 + pa] = lo < end && a_col[lo] == c ? a_val[lo] : 0.0;
        }
        bool bad = false;
        for (int k = 0; k < W; ++k) {
            __syncthreads();
            const bool live = k < m;
            const double d = live ? tile[k][t0 + k] : 1.0;
            if (live && !(d > 0.0 && isfinite(d))) bad = true;
            const double c = sqrt(d);
            const bool below = live && a > k && a < m;
            const double x = below ? tile[k][tid] / c : 0.0;  // C[a][k]
            __syncthreads();  // every lane holds the pivot before lane k replaces it
            if (below) tile[k][tid] = x;
            else if (live && a == k) tile[k][tid] = c;
            __syncthreads();
            if (below)
                for (int b = k + 1; b <= a; ++b) tile[b][tid] = fma(-x, tile[k][t0 + b], tile[b][tid]);
        }
        __syncthreads();
        double g = 0.0;
        for (int b = W - 1; b >= 0; --b) {
            double part = a > b && a < m ? tile[b][tid] * g : 0.0;  // C[a][b] g_a
            for (int off = W / 2; off; off >>= 1) part += __shfl_xor(part, off, W);
            if (a == b && b < m) g = ((b == m - 1 ? 1.0 : 0.0) - part) / tile[b][tid];
        }
        if (a < m) {
            const T out = (T)g;
            g_val[g0 + a] = out;
            if (bad) {
                if (a == 0) status[i] = 1;
            } else if (!isfinite((double)out)) {
                status[i] = 2;
            }
        }
    }
}

}  // namespace spmv
