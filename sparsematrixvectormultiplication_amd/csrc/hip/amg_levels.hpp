// amg_levels.hpp -- the AMG preconditioner object as the device holds it, and what its two setups share: the host setup
// (spmv_amg.hip: amg_build, from host/amg_plan.c's plan) and the device setup (spmv_amg_setup.hip) both fill the
// per-level operators, g and the scalars of a spmv_amg_precond and then call amg_finish, which writes the cycle's passes,
// picks the chained tail and makes the workspace, and amg_wrap; both entry points begin with amg_check_args and read the
// object of a finished P through amg_of.  Host code only.
#pragma once
#include "spmv_internal.hpp"

#include <cmath>

#include "amg_kernels.hpp"
#include "precond_kernels.hpp"

struct AmgOp {  // a CSR operator of P's own: values of the handle's dtype
    int *rp = nullptr, *col = nullptr;
    void *val = nullptr;
    int rows = 0, G = 1;
    long long nz = 0;
    void release() {
        (void)hipFree(rp), (void)hipFree(col), (void)hipFree(val);
        rp = col = nullptr, val = nullptr;
    }
    // rows, entries and the lanes per row: the largest power of two <= the mean row, at most 32
    void shape(int rows_, long long nz_) {
        rows = rows_, nz = nz_;
        const long long mean = rows ? nz / rows : 0;
        G = pow2_floor((int)std::min<long long>(std::max<long long>(mean, 1), 32));
    }
};

enum { kAmgSetupHost = 0, kAmgSetupDevice = 1 };
// the phases of the device setup, in the order of spmv_hip_precond_amg_setup_info's words 1 ..
enum { kAmgPhStats = 0, kAmgPhStrength, kAmgPhAggregate, kAmgPhTentative, kAmgPhTranspose, kAmgPhAP, kAmgPhRAP,
       kAmgPhInverse, kAmgPhRound, kAmgPhases };
static_assert(1 + kAmgPhases == SPMV_PRECOND_AMG_SETUP_INFO_WORDS, "the setup info words and the phases are out of step");

struct spmv_amg_precond {
    int levels = 0, chain = 1, first_chained = -1, launches = 0, coarsest = 0;
    spmv_csr_dev *A0 = nullptr;  // level 0 when it is not DIRECT
    AmgOp A[kAmgMaxLevels], P[kAmgMaxLevels], R[kAmgMaxLevels], inv;
    double *g[kAmgMaxLevels] = {};
    double w[kAmgMaxLevels] = {}, rho[kAmgMaxLevels] = {};
    int kind[kAmgMaxLevels] = {}, n[kAmgMaxLevels] = {}, na[kAmgMaxLevels] = {};
    long long a_nz[kAmgMaxLevels] = {};
    std::vector<AmgStep> steps;
    AmgStep *d_steps = nullptr;
    int tail0 = -1, tail1 = -1;    // the passes of the chained tail
    long long work_values = 0;     // values of all level vectors at k = 1
    void *work = nullptr;          // P's own, for one right-hand side
    int us[3] = {0, 0, 0};
    int setup = kAmgSetupHost;     // which setup made it, and the device setup's microseconds per phase
    int phase_us[kAmgPhases] = {};
    ~spmv_amg_precond() {
        spmv_hip_csr_free(A0);
        for (int l = 0; l < kAmgMaxLevels; ++l) {
            A[l].release(), P[l].release(), R[l].release();
            (void)hipFree(g[l]);
        }
        inv.release();
        (void)hipFree(d_steps);
        (void)hipFree(work);
        (void)hipGetLastError();
    }
};

// the refusals of the rounding to the handle's dtype, in both setups' words
constexpr const char *kAmgMsgEntry = "csr_precond_build_amg: level %d: an entry of %s is not finite in the handle's dtype";
constexpr const char *kAmgMsgDiagonal =
    "csr_precond_build_amg: level %d: the diagonal of row %d is not finite and > 0 in the handle's dtype";
constexpr const char *kAmgMsgPlan = "csr_precond_build_amg (local rows; the handle's first row is global row %d): %s";

// one operator on the host: fp64
struct HostOp {
    std::vector<int> rp, col;
    std::vector<double> val;
};

// h rounded once to T and uploaded as op
template <typename T>
int amg_op_upload(const HostOp &h, int rows, AmgOp &op, const char *what, int level) {
    const size_t nz = h.col.size();
    std::vector<T> v(nz);
    for (size_t e = 0; e < nz; ++e) {
        v[e] = (T)h.val[e];
        if (!std::isfinite((double)v[e]))
            return fail(kAmgMsgEntry, level, what);
    }
    op.shape(rows, (long long)nz);
    if (upload_array(&op.rp, h.rp.data(), (size_t)rows + 1, 0) || upload_array(&op.col, h.col.data(), nz, 4) ||
        upload_array((T **)&op.val, v.data(), nz, 4))
        return -1;
    return 0;
}

// spmv_amg.hip: the levels of ap are filled (levels, kind, n, na, a_nz, the operators, g, A0): the passes of the cycle,
// the chained tail, the launches and the zeroed workspace for one right-hand side of value_bytes-byte values
int amg_finish(spmv_amg_precond *ap, int value_bytes);
// ... and the preconditioner object of handle m around it (takes ap)
spmv_precond *amg_wrap(const spmv_csr_dev *m, spmv_amg_precond *ap, size_t value_bytes);
// P's hierarchy, or NULL with the refusal "<what>: kind K is not AMG"
const spmv_amg_precond *amg_of(const spmv_precond *P, const char *what);

// the argument checks of both setups' entry points, in the host setup's words
inline int amg_check_args(double theta, int coarse_rows, int max_levels) {
    if (!(theta >= 0.0 && theta < 1.0)) return fail("csr_precond_build_amg: theta = %g, must be in [0, 1)", theta);
    if (coarse_rows < 1 || coarse_rows > kAmgChainRows)
        return fail("csr_precond_build_amg: coarse_rows = %d, must be in [1, %d]", coarse_rows, kAmgChainRows);
    if (max_levels < 1 || max_levels > kAmgMaxLevels)
        return fail("csr_precond_build_amg: max_levels = %d, must be in [1, %d]", max_levels, kAmgMaxLevels);
    return 0;
}
