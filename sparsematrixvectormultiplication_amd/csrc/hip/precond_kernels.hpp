// precond_kernels.hpp -- the kernels of the Jacobi and block-Jacobi preconditioners on CSR handles
// (spmv_precond.hip builds them; csr_pcg and csr_pbicgstab apply them) (gfx950), and below them the preconditioner
// object of every kind: the table a kind family with launches of its own fills in (precond_family), what the solvers
// ask of it (precond_path, precond_apply, precond_work_bytes, precond_refuse_one_wide) and the frame of every build
// entry point (precond_build_frame, precond_new).
//
// P covers the handle's own rows [row0, row0 + n) in blocks of b consecutive rows from row0 (the last block may be
// shorter, bk = min(b, n - k b) rows).  Local row i = global row row0 + i sits in block k = i / b at place ii = i % b.
//
//   pc_extract      one wavefront per row: the row's entries in coalesced chunks of 64; the few that fall into the
//                   block's columns [row0 + k b, row0 + k b + bk) are added lane by lane in entry order (a ballot over
//                   the chunk, its set bits in lane order) into the fp64 block D_k, row-major.  A row of 10^5 entries is
//                   1600 chunk loads of one wavefront while the other wavefronts take the other rows.  A row without a
//                   (i, i) entry records itself in bad[0] (the smallest such row).
//   pc_invert_diag  b = 1: inv[i] = 1.0 / d_i, a correctly rounded fp64 division, rounded once to T.  A zero or
//                   non-finite d_i (or a stored inverse that is not finite) records row i in bad[1].
//   pc_invert_block b > 1: one wavefront per block, Gauss-Jordan with partial pivoting (the first largest |pivot|
//                   wins) on [D_k | I] in LDS, lane j = column j of the bk x 2 bk system; fp64 throughout, the inverse
//                   rounded once to T.  A zero or non-finite pivot (or a non-finite inverse) records block k in bad[1].
//   pc_apply        z = M^-1 r, one lane per row: sum_c inv_k[c][ii] r[k b + c] in double, c ascending, the first
//                   term the plain product, rounded once to T.  With DOTS the lanes also accumulate r.r and r.z for
//                   block_partials<2> (the reduction order of solver_ops.hpp, lanes walking single rows).
//
// The stored inverse: block k at inv[k b^2], column-major inside the block (element (ii, c) at c b + ii), so at a
// fixed c neighbouring lanes (neighbouring rows of a block) read neighbouring addresses; b = 1 is inv[i] = 1 / d_i.
// The apply reads every stored value once: b sizeof(T) bytes of inv, plus r and z, per row.
#pragma once
#include "refresh_kernels.hpp"
#include "solver_ops.hpp"

namespace spmv {

constexpr int kPcMaxBlock = 32;  // widest block: 2 b columns on the 64 lanes of one wavefront
constexpr int kPcWaves = kBlock / 64;
constexpr int kPcBlocks = 2048;  // grid cap of pc_apply outside csr_pcg (csr_pcg uses csr_cg's grid)

// wavefront per row.  D: n_blocks * b * b doubles (zeroed), block k row-major at k b^2.  bad[0]: first row without
// its diagonal entry (atomicMin; INT_MAX when none)
template <typename T>
__global__ __launch_bounds__(kBlock) void pc_extract(int n, int row0, int b, const int *__restrict__ row_ptr,
                                                     const int *__restrict__ col, const T *__restrict__ val,
                                                     double *__restrict__ D, int *__restrict__ bad) {
    const int lane = threadIdx.x & 63;
    const long long waves = (long long)gridDim.x * kPcWaves;
    for (long long i = (long long)blockIdx.x * kPcWaves + (threadIdx.x >> 6); i < n; i += waves) {
        const long long k = i / b;
        const int ii = (int)(i - k * b);
        const int bk = (int)std::min<long long>(b, n - k * b);
        const long long c0 = row0 + k * b;
        const int e0 = row_ptr[i], e1 = row_ptr[i + 1];
        double acc = 0.0;  // lane j < bk: the sum of the row's entries in column c0 + j
        bool have = false;
        for (int base = e0; base < e1; base += 64) {
            const int e = base + lane;
            int rel = -1;
            double v = 0.0;
            if (e < e1) {
                const long long d = (long long)col[e] - c0;
                if (d >= 0 && d < bk) {
                    rel = (int)d;
                    v = (double)val[e];
                }
            }
            unsigned long long mask = __ballot(rel >= 0);
            while (mask) {  // in lane (= entry) order
                const int src = __ffsll((long long)mask) - 1;
                mask &= mask - 1;
                const int r = __shfl(rel, src);
                const double x = __shfl(v, src);
                if (lane == r) {
                    acc = have ? acc + x : x;
                    have = true;
                }
            }
        }
        if (lane < bk) D[k * b * b + (long long)ii * b + lane] = acc;
        if (lane == ii && !have) atomicMin(bad, (int)i);
    }
}

// b = 1: inv[i] = 1.0 / d_i in T; bad[1]: first row whose d_i or inverse is zero or not finite
template <typename T>
__global__ __launch_bounds__(kBlock) void pc_invert_diag(int n, const double *__restrict__ D, T *__restrict__ inv,
                                                         int *__restrict__ bad) {
    const long long stride = (long long)gridDim.x * kBlock;
    for (long long i = (long long)blockIdx.x * kBlock + threadIdx.x; i < n; i += stride) {
        const double d = D[i];
        const T t = (T)(1.0 / d);
        inv[i] = t;
        if (d == 0.0 || !isfinite(d) || !isfinite((double)t)) atomicMin(bad + 1, (int)i);
    }
}

// b > 1: one wavefront per block (grid-stride over the blocks); bad[1]: first block with a zero or non-finite pivot
// or a non-finite inverse
template <typename T>
__global__ __launch_bounds__(64) void pc_invert_block(int n, int b, const double *__restrict__ D, T *__restrict__ inv,
                                                      int *__restrict__ bad) {
    __shared__ double aug[kPcMaxBlock][2 * kPcMaxBlock];
    const int j = threadIdx.x;  // column j of [D_k | I]
    const long long nblocks = (n + (long long)b - 1) / b;
    for (long long k = blockIdx.x; k < nblocks; k += gridDim.x) {
        const int bk = (int)std::min<long long>(b, n - k * b);
        const double *Dk = D + k * b * b;
        __syncthreads();
        if (j < 2 * bk)
            for (int r = 0; r < bk; ++r) aug[r][j] = j < bk ? Dk[r * b + j] : (j - bk == r ? 1.0 : 0.0);
        __syncthreads();
        bool ok = true;
        for (int c = 0; c < bk; ++c) {
            // every lane finds the same pivot row: the first largest |aug[r][c]|, r >= c
            int p = c;
            double best = fabs(aug[c][c]);
            for (int r = c + 1; r < bk; ++r) {
                const double v = fabs(aug[r][c]);
                if (v > best) best = v, p = r;
            }
            const double piv = aug[p][c];
            if (!(best > 0.0) || !isfinite(piv)) {
                ok = false;
                break;
            }
            __syncthreads();
            if (j < 2 * bk && p != c) {
                const double t = aug[c][j];
                aug[c][j] = aug[p][j];
                aug[p][j] = t;
            }
            __syncthreads();
            if (j < 2 * bk) aug[c][j] = aug[c][j] / piv;
            __syncthreads();
            for (int r = 0; r < bk; ++r) {
                if (r == c) continue;
                const double f = aug[r][c];
                __syncthreads();  // every lane holds f before lane c overwrites aug[r][c]
                if (j < 2 * bk) aug[r][j] = aug[r][j] - f * aug[c][j];
            }
            __syncthreads();
        }
        bool fin = true;
        if (ok && j >= bk && j < 2 * bk) {
            T *out = inv + k * b * b + (long long)(j - bk) * b;  // column j - bk of the inverse
            for (int r = 0; r < bk; ++r) {
                const T t = (T)aug[r][j];
                out[r] = t;
                fin = fin && isfinite((double)t);
            }
        }
        if ((!ok || __ballot(!fin) != 0) && j == 0) atomicMin(bad + 1, (int)k);
    }
}

// z = M^-1 r on local rows [0, n) (r, z: element i = global row row0 + i).  flags (NULL: none): a solver's stop flags
// (solver_ops.hpp), any state but kSolverRun returns before writing.  DOTS: the workgroup's partials of r.r and r.z in
// part[2 g], part[2 g + 1].  Lanes walk single rows (PieceLane with V = 1).
template <typename T, bool DOTS>
__global__ __launch_bounds__(kBlock) void pc_apply(long long n, int b, const T *__restrict__ inv,
                                                   const T *__restrict__ r, T *__restrict__ z,
                                                   const int *__restrict__ flags, double *__restrict__ part) {
    if (flags && flags[kSolverState] != kSolverRun) return;
    double acc[2] = {0.0, 0.0};
    for (PieceLane l(0, n, 1); l.q < l.end; l.q += l.stride) {
        const long long i = l.q, k = i / b;
        const int ii = (int)(i - k * b);
        const int bk = (int)std::min<long long>(b, n - k * b);
        const T *ik = inv + k * b * b + ii;
        const T *rk = r + k * b;
        double s = (double)ik[0] * (double)rk[0];
        for (int c = 1; c < bk; ++c) s += (double)ik[(long long)c * b] * (double)rk[c];
        const T zi = (T)s;
        z[i] = zi;
        if constexpr (DOTS) {
            const double ri = (double)r[i];
            acc[0] += ri * ri;
            acc[1] += ri * (double)zi;
        }
    }
    if constexpr (DOTS) block_partials<2>(acc, part);
}

}  // namespace spmv

// ---------------------------------------------------------------- the preconditioner object (include/spmv_hip.h)
struct spmv_precond;

// What a kind family with launches of its own -- SSOR / ILU(0), FSAI, AMG, CHEBYSHEV -- gives the shared code: one
// static const instance in the file that owns the family, the only file that knows what P->impl points to.
struct precond_family {
    const char *name;       // the end of "<entry point>: kind K is not <name>" (precond_impl)
    const char *work_text;  // what spmv_hip_precond_apply_multi_on says of a missing d_work
    // z = M^-1 r by the family's launches on stream s.  flags as pc_apply: SSOR's / ILU(0)'s solves return once a solver
    // has stopped.  FSAI, AMG and CHEBYSHEV do not look at them: their launches are handles' own, and after a stop r no
    // longer changes, so z is rewritten with the bits it holds.
    int (*apply)(const spmv_precond *P, const void *r, void *z, const int *flags, hipStream_t s);
    // the same for rows x k row-major R and Z through products alone, P's own vectors not used (k = 1: the bits of
    // apply); work: work_bytes(P, k) bytes.  NULL (both): the family takes one right-hand side
    int (*apply_multi)(const spmv_precond *P, int k, const void *R, void *Z, void *work, hipStream_t s);
    long long (*work_bytes)(const spmv_precond *P, int k);
    // spmv_hip_precond_factors past its argument checks; NULL: the family has no factors
    int (*factors)(const spmv_precond *P, int which, int *row_ptr, int *col, void *val);
    void (*free)(void *impl);
    // spmv_hip_precond_refresh past the shared checks (P fits m, m's pattern is the stamp's): P from m's values, all or
    // nothing.  NULL: the kind's pattern, hierarchy or interval is a function of the values -- refused, build it again
    int (*refresh)(spmv_precond *P, const spmv_csr_dev *m);
};

struct spmv_precond {
    int kind = 0, block = 1;  // SPMV_PRECOND_*; rows per block (1 for all but BLOCK_JACOBI)
    int rows = 0, row0 = 0;   // the handle's own rows [row0, row0 + rows)
    int value_bytes = 8;      // the handle's dtype
    void *inv = nullptr;      // JACOBI / BLOCK_JACOBI: ceil(rows / block) * block^2 values of that dtype (layout above); owned
    void *impl = nullptr;     // the other kinds: the family's own object; owned, inv is NULL
    const precond_family *family = nullptr;  // NULL: JACOBI / BLOCK_JACOBI, applied by pc_apply / mpc_apply
    PatternStamp stamp;       // the pattern of the first refresh's handle (refresh_kernels.hpp); none before it
};

// the object every build ends with: the five fields from the handle, and the family's payload
inline spmv_precond *precond_new(const spmv_csr_dev *m, int kind, int block, size_t value_bytes,
                                 const precond_family *family = nullptr, void *impl = nullptr) {
    spmv_precond *P = new spmv_precond;
    P->kind = kind;
    P->block = block;
    P->rows = m->M_local;
    P->row0 = m->row0;
    P->value_bytes = (int)value_bytes;
    P->family = family;
    P->impl = impl;
    return P;
}

// P's payload for a reader of family f (the *_info entry points); NULL with the refusal when P is of another kind
inline void *precond_impl(const spmv_precond *P, const precond_family *f, const char *what) {
    if (P->family == f) return P->impl;
    fail("%s: kind %d is not %s", what, P->kind, f->name);
    return nullptr;
}

// The one question a solver asks.  kPathJacobi: D^-1 fuses into the solver's update kernels; kPathBlock: a pc_apply /
// mpc_apply pass (which can carry the dots); kPathOwn: the family's launches, then a pass of the solver's for its dots.
enum PrecondPath { kPathNone = 0, kPathJacobi = 1, kPathBlock = 2, kPathOwn = 3 };
inline PrecondPath precond_path(const spmv_precond *P) {
    return !P ? kPathNone : P->family ? kPathOwn : P->block == 1 ? kPathJacobi : kPathBlock;
}

// bytes of the workspace of a k-wide apply: 0 without P and for Jacobi and block-Jacobi, else the family's (FSAI's G R
// with a line tail, the level vectors of AMG, the three arrays of CHEBYSHEV); -1 where there is no k-wide apply
inline long long precond_work_bytes(const spmv_precond *P, int k) {
    if (!P || !P->family) return 0;
    return P->family->apply_multi ? P->family->work_bytes(P, k) : -1;
}
// that workspace from a solver's scope; NULL where the kind needs none
inline void *precond_work_alloc(SolverScope &scope, const spmv_precond *P, int k) {
    const long long bytes = precond_work_bytes(P, k);
    return bytes > 0 ? scope.alloc((size_t)bytes) : nullptr;
}

// a kind without a k-wide apply (SSOR, ILU(0)): -1 with the one sentence, naming `what`
inline int precond_refuse_one_wide(const spmv_precond *P, const char *what) {
    if (P->family && !P->family->apply_multi)
        return fail("%s: an SSOR or ILU(0) preconditioner is two triangular solves, and those take one right-hand side", what);
    return 0;
}

// The frame of every spmv_hip_csr_precond_build*: the device, the two NULL refusals, the kind's own argument checks
// (check() != 0: refused, the message is set), the handle, then build(T(), &P) with T the handle's dtype under guarded().
// A refused build or a failed allocation is reported by the return value, not by the next launch.
template <typename Check, typename Build>
int precond_build_frame(const char *what, const spmv_csr_dev *m, spmv_precond **out, Check check, Build build) {
    if (need_device()) return -1;
    if (!out) return fail("%s: out is NULL", what);
    *out = nullptr;
    if (!m) return fail("%s: NULL handle", what);
    if (check() || handle_ok(m, what)) return -1;
    spmv_precond *P = nullptr;
    const int rc = solver_dispatch(what, m->value_bytes, [&](auto t) { return build(t, &P); });
    (void)hipGetLastError();
    if (!rc) *out = P;
    return rc;
}

// z = M^-1 r on P's rows (r, z at local row 0) on stream s; flags / part as pc_apply; grid 0: by the row count
template <typename T, bool DOTS>
void precond_launch(const spmv_precond *P, const void *r, void *z, const int *flags, double *part, int grid,
                    hipStream_t s) {
    const long long n = P->rows;
    if (!grid) grid = solver_grid(kPcBlocks, n, kBlock);
    hipLaunchKernelGGL((pc_apply<T, DOTS>), dim3(grid), dim3(kBlock), 0, s, n, P->block, (const T *)P->inv,
                       (const T *)r, (T *)z, flags, part);
}

// z = M^-1 r outside the fused paths: the family's own launches, or a pc_apply pass on the row count's grid
template <typename T>
int precond_apply(const spmv_precond *P, const void *r, void *z, const int *flags, hipStream_t s) {
    if (P->family) return P->family->apply(P, r, z, flags, s);
    precond_launch<T, false>(P, r, z, flags, nullptr, 0, s);
    return 0;
}

// P fits handle m (its rows, first row and dtype); else -1 with a message naming `what`
inline int precond_matches(const spmv_csr_dev *m, const spmv_precond *P, const char *what) {
    if (P->rows != m->M_local || P->row0 != m->row0 || P->value_bytes != m->value_bytes)
        return fail("%s: the preconditioner covers rows [%d, %d) with %d-byte values, the handle rows [%d, %d) with %d",
                    what, P->row0, P->row0 + P->rows, P->value_bytes, m->row0, m->row0 + m->M_local, m->value_bytes);
    return 0;
}
