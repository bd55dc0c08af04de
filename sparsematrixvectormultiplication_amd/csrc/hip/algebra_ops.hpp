// algebra_ops.hpp -- the host frame of the operations that build a CSR matrix on the device and hand it to csr_adopt as a
// new handle: csr_from_coo (spmv_coo.hip), csr_transpose (spmv_transpose.hip), csr_spgemm (spmv_spgemm.hip), csr_add
// (spmv_spadd.hip), and of the AMG device setup (spmv_amg_setup.hip), which strings their cores together.  The refusals
// the entries share, the step from per-row counts to row_ptr, the adopt with its hand-over of ownership, the sort widths
// and the phase timer.  The arrays themselves are CsrView and DevCsr (spmv_internal.hpp).  Host code only.
#pragma once
#include "spmv_internal.hpp"

namespace algebra {

// An operand of `who` must be a whole matrix that holds its CSR arrays.  operand: "A" / "B", or NULL for the only one.
inline int operand_ok(const char *who, const char *operand, const char *verb, const spmv_csr_dev *m) {
    const std::string is_handle = operand ? std::string(operand) + " is a handle" : "a handle";
    if (m->row0 != 0 || m->M_local != m->M_total)
        return fail("%s: %s of rows [%d, %d) of %d; only whole matrices %s", who, is_handle.c_str(), m->row0,
                    m->row0 + m->M_local, m->M_total, verb);
    if (!csr_holds_arrays(m)) return fail("%s: %s does not hold its CSR arrays", who, operand ? operand : "the handle");
    return 0;
}

// row_ptr of C on the host from the entries of every row (counts_to_row_ptr), or the refusal of a C beyond a handle
inline int row_ptr_of_counts(const char *who, const std::vector<int> &cnt, std::vector<int> &rp, RowCounts &counts) {
    const int M = (int)cnt.size();
    rp.assign((size_t)M + 1, 0);
    counts = counts_to_row_ptr(M, cnt.data(), rp.data());
    if (counts.over >= 0)
        return fail("%s: C has more than %lld entries (by row %d of %d): beyond the 32-bit entry index of a handle", who,
                    kMaxEntries, counts.over, M);
    return 0;
}

// csr_adopt of what a core made: on success the handle owns col and val.  C is spent either way: what it still holds (its
// row_ptr; after a refusal everything) goes when the caller's object does.
template <typename T>
int adopt(DevCsr &&C, const std::vector<int> &rp_host, spmv_csr_dev **out) {
    ClearHipError clear;
    const int rc = csr_adopt<T>(C.rows, C.cols, rp_host.data(), C.col, static_cast<T *>(C.val), out);
    if (rc == 0) C.entries_adopted();
    return rc;
}

inline unsigned bits_for(unsigned long long n) {  // bits that hold 0 .. n - 1 (at least one): a radix sort's width
    unsigned bits = 1;
    while (bits < 63 && (1ull << bits) < n) ++bits;
    return bits;
}

// wall time of a build's phases in ms: lap(k) closes phase k (no synchronisation: each phase ends in its own)
struct PhaseTimer {
    double *ms;
    double t0 = UploadTrace::now();
    void lap(int k) {
        const double t = UploadTrace::now();
        ms[k] = (t - t0) * 1e3;
        t0 = t;
    }
};

}  // namespace algebra
