// row_counts.hpp -- per-row entry counts to the row_ptr of a handle, on the host: the step between the symbolic and the
// numeric pass of the product and the sum (algebra_ops.hpp).  Includes no HIP header, so a host compiler alone can test it.
#pragma once

constexpr int kPad = 8192 + 64;  // zero entries behind col/val: the stream / LDS kernels stage
                                   // whole units without bounds tests (>= kStreamCapMax, kHllCap)
constexpr long long kMaxEntries = 0x7fffffffLL - kPad;  // the 32-bit entry index of a handle, the pad included

struct RowCounts {
    long long nz = 0, widest = 0;  // entries of all rows, of the widest row
    int over = -1;                 // the first row at which the running sum passes kMaxEntries (rp is filled up to it); -1: none
};

// rp[0] = 0, rp[i + 1] = cnt[0] + .. + cnt[i] for the M rows
inline RowCounts counts_to_row_ptr(int M, const int *cnt, int *rp) {
    RowCounts r;
    rp[0] = 0;
    for (int i = 0; i < M; ++i) {
        r.nz += cnt[i];
        if (cnt[i] > r.widest) r.widest = cnt[i];
        if (r.nz > kMaxEntries) {
            r.over = i;
            return r;
        }
        rp[i + 1] = (int)r.nz;
    }
    return r;
}
