// The cases of tests/test_row_counts_host.py: counts_to_row_ptr (csrc/hip/row_counts.hpp) alone, no HIP, no GPU.
// Built with -fsanitize=address,undefined; exit code 0 and "ok" when every case holds.
#include <cstdio>
#include <vector>

#include "row_counts.hpp"

static int failures = 0;

static void check(const char *name, const std::vector<int> &cnt, const std::vector<int> &rp_want, long long nz, long long widest,
                  int over) {
    const int M = (int)cnt.size();
    std::vector<int> rp((size_t)M + 1, -7);  // exactly M + 1: a write behind it is the sanitizer's to find
    const RowCounts r = counts_to_row_ptr(M, cnt.data(), rp.data());
    bool ok = r.nz == nz && r.widest == widest && r.over == over;
    for (size_t i = 0; i < rp_want.size(); ++i) ok = ok && rp[i] == rp_want[i];  // (a refusal: the rows in front of it)
    for (size_t i = rp_want.size(); i < rp.size(); ++i) ok = ok && rp[i] == -7;  // ... and nothing from it on
    if (!ok) {
        ++failures;
        printf("FAILED %s: nz %lld (want %lld), widest %lld (want %lld), over %d (want %d)\n", name, r.nz, nz, r.widest, widest,
               r.over, over);
    }
}

int main() {
    const int P = 1 << 30;
    const long long L = 0x7fffffffLL - kPad;  // what a handle's 32-bit entry index takes, the pad behind it included
    if (kMaxEntries != L) ++failures, printf("FAILED kMaxEntries = %lld, want %lld\n", kMaxEntries, L);
    check("no rows", {}, {0}, 0, 0, -1);
    check("one empty row", {0}, {0, 0}, 0, 0, -1);
    check("3 0 5", {3, 0, 5}, {0, 3, 3, 8}, 8, 5, -1);
    check("three rows of 2^30", {P, P, P}, {0, P}, 2LL * P, P, 1);  // 2^30 is under the limit, 2^31 beyond it: row 1
    check("exactly the limit", {(int)(L - 5), 5}, {0, (int)(L - 5), (int)L}, L, L - 5, -1);
    check("one entry more", {(int)(L - 5), 0, 6}, {0, (int)(L - 5), (int)(L - 5)}, L + 1, L - 5, 2);
    if (!failures) printf("ok\n");
    return failures ? 1 : 0;
}
