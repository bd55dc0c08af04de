// canon_rows.hpp -- the canonical diagonal block of a CSR handle on the host, shared by the builds that start from it
// (spmv_trsv.hip: the triangular solves, SSOR, ILU(0); spmv_fsai.hip: FSAI; spmv_amg.hip: AMG; spmv_cheb.hip:
// CHEBYSHEV).  Host code only.
#pragma once
#include "spmv_internal.hpp"

#include <algorithm>

// the canonical diagonal block: sorted rows without repeats, local columns; diag[i] = the place of (i, i) or -1
struct Canon {
    int n = 0;
    std::vector<int> rp, col, diag;
    std::vector<double> val;
};

inline double now_ms() { return UploadTrace::now() * 1e3; }

// the handle's CSR arrays downloaded and A[row0:row1, row0:row1] made canonical: local columns, every row sorted by
// column (a stable sort), entries that repeat a column added in entry order in fp64
template <typename T>
int canon_download(const spmv_csr_dev *m, Canon &A) {
    const int n = m->M_local;
    const size_t nz = (size_t)m->nz;
    std::vector<int> rp((size_t)n + 1, 0), col(nz);
    std::vector<T> val(nz);
    HIP_TRY(hipMemcpy(rp.data(), m->row_ptr, ((size_t)n + 1) * sizeof(int), hipMemcpyDeviceToHost));
    if (nz) HIP_TRY(hipMemcpy(col.data(), m->col, nz * sizeof(int), hipMemcpyDeviceToHost));
    if (nz) HIP_TRY(hipMemcpy(val.data(), m->val, nz * sizeof(T), hipMemcpyDeviceToHost));
    A.n = n;
    A.rp.assign((size_t)n + 1, 0);
    A.diag.assign((size_t)n, -1);
    A.col.clear();
    A.val.clear();
    A.col.reserve(nz);
    A.val.reserve(nz);
    std::vector<int> idx;
    for (int i = 0; i < n; ++i) {
        idx.clear();
        for (int e = rp[i]; e < rp[i + 1]; ++e)
            if (col[e] >= m->row0 && col[e] < m->row0 + n) idx.push_back(e);
        std::stable_sort(idx.begin(), idx.end(), [&](int a, int b) { return col[a] < col[b]; });
        for (size_t k = 0; k < idx.size(); ++k) {
            const int c = col[idx[k]] - m->row0;
            if (k && c == A.col.back()) {
                A.val.back() += (double)val[idx[k]];
                continue;
            }
            if (c == i) A.diag[i] = (int)A.col.size();
            A.col.push_back(c);
            A.val.push_back((double)val[idx[k]]);
        }
        A.rp[i + 1] = (int)A.col.size();
    }
    return 0;
}

template <typename V>
int to_device(V **d, const std::vector<V> &h) {
    return upload_array(d, h.data(), h.size(), h.empty() ? 4 : 0);
}

// the first row (B's numbering) whose diagonal is missing; -1: none
inline int first_missing_diag(const Canon &B) {
    for (int i = 0; i < B.n; ++i)
        if (B.diag[i] < 0) return i;
    return -1;
}

// the plan a build's own upload got (fsai_info, cheb_info): 0 the gather kernels, 1 an x-window plan, 2 an x-window plan
// with a pattern plan, 3 csr_tile
inline int plan_of(const spmv_csr_dev *m) {
    if (!m) return 0;
    return m->xw.blocks > 0 ? (m->xw.pat.ptab ? 2 : 1) : m->tile.blocks > 0 ? 3 : 0;
}
