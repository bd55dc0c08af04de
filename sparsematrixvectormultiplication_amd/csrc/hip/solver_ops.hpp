// solver_ops.hpp -- what the iterated methods on CSR handles share: csr_cg and csr_cg_multi (spmv_cg.hip), csr_pcg
// (spmv_pcg.hip), csr_pcg_multi (spmv_pcg_multi.hip), csr_bicgstab and csr_pbicgstab (spmv_bicgstab.hip), csr_minres
// (spmv_minres.hip), csr_gmres (spmv_gmres.hip), csr_cgls (spmv_cgls.hip), csr_lobpcg (spmv_lobpcg.hip) and the power
// iterations (spmv_comm.hip).
// For the device: the pieces a vector kernel loads and stores, the lanes' walk over them, the fixed-order reductions
// and the stop flags.  For the host: the frame of a solve -- the refusals the entries share (solver_check_*), the
// buffers and events (SolverScope), the start and the end of the timed part (solver_begin, solver_finish), the grid
// clamp (solver_grid), the poll of the stop word (solver_poll) and the dtype dispatch (solver_dispatch).
//
// Reduction order.  Products are accumulated in double for fp32 and fp64 data alike.  A lane adds its pieces in stride
// order (and a piece's rows in row order), group_sum<64> adds the lanes of a wave, the waves of a workgroup are added in
// wave order (workgroup_sum), the workgroups in workgroup order (solver_fold) and the ranks in rank order
// (solver_rank_sum).  No atomics: every run gives the same bits.  The grid is each solver's own: it decides the bits.
#pragma once
#include "spmv_internal.hpp"

#include "spmm_kernels.hpp"  // v4f
#include "wave_ops.hpp"

namespace spmv {

constexpr int kNormBlocks = 512;  // grid cap of the vector kernels of csr_cg, cg_multi at k = 1 and the power iterations

// one piece at p: V = 1 element, or V elements of T in one 16-byte load / store
template <typename T, int V>
__device__ __forceinline__ void piece_load(const T *__restrict__ p, T (&v)[V]) {
    static_assert(V == 1 || V * sizeof(T) == 16, "one element or one 16-byte piece");
    if constexpr (V == 1) {
        v[0] = p[0];
    } else if constexpr (sizeof(T) == 8) {
        const v2d w = *reinterpret_cast<const v2d *>(p);
        v[0] = w.x, v[1] = w.y;
    } else {
        const v4f w = *reinterpret_cast<const v4f *>(p);
        v[0] = w.x, v[1] = w.y, v[2] = w.z, v[3] = w.w;
    }
}

template <typename T, int V>
__device__ __forceinline__ void piece_store(T *__restrict__ p, const T (&v)[V]) {
    static_assert(V == 1 || V * sizeof(T) == 16, "one element or one 16-byte piece");
    if constexpr (V == 1) {
        p[0] = v[0];
    } else if constexpr (sizeof(T) == 8) {
        *reinterpret_cast<v2d *>(p) = v2d{v[0], v[1]};
    } else {
        *reinterpret_cast<v4f *>(p) = v4f{v[0], v[1], v[2], v[3]};
    }
}

// piece [i0, i0 + V) of a; rows outside [lo, hi) read as 0.  A piece that holds lo or hi - 1 may be cut: its rows are
// then read one by one (the buffers are hipMalloc-aligned, so a whole piece starting at a multiple of V is one load).
template <typename T, int V>
__device__ __forceinline__ void piece_load(const T *__restrict__ a, long long i0, long long lo, long long hi, T (&v)[V]) {
    if (i0 >= lo && i0 + V <= hi) {
        piece_load<T, V>(a + i0, v);
    } else {
#pragma unroll
        for (int j = 0; j < V; ++j) v[j] = i0 + j >= lo && i0 + j < hi ? a[i0 + j] : T(0);
    }
}

// piece [i0, i0 + V) of a; rows outside [lo, hi) are not written
template <typename T, int V>
__device__ __forceinline__ void piece_store(T *__restrict__ a, long long i0, long long lo, long long hi,
                                            const T (&v)[V]) {
    if (i0 >= lo && i0 + V <= hi) {
        piece_store<T, V>(a + i0, v);
    } else {
#pragma unroll
        for (int j = 0; j < V; ++j)
            if (i0 + j >= lo && i0 + j < hi) a[i0 + j] = v[j];
    }
}

// the lane's pieces of rows [lo, hi): q = first, first + stride, ... < end; piece q covers rows [q V, q V + V).  Lane g
// of the launch starts at lo / V + g, the stride is grid x kBlock.
struct PieceLane {
    long long q, stride, end;
    __device__ __forceinline__ PieceLane(long long lo, long long hi, int V) {
        q = lo / V + (long long)blockIdx.x * kBlock + threadIdx.x;
        stride = (long long)gridDim.x * kBlock;
        end = (hi + V - 1) / V;
    }
};

// the workgroup's sums of the lanes' NV values (group_sum<64> per wave, then the waves in order): thread j < NV returns
// sum j, the other threads 0
template <int NV>
__device__ __forceinline__ double workgroup_sum(double (&acc)[NV]) {
    __shared__ double wave_sum[kBlock / 64][NV];
#pragma unroll
    for (int j = 0; j < NV; ++j) acc[j] = group_sum<64>(acc[j]);
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (int j = 0; j < NV; ++j) wave_sum[threadIdx.x >> 6][j] = acc[j];
    }
    __syncthreads();
    double s = 0;
    if (threadIdx.x < NV) {
        const int j = threadIdx.x;
        s = wave_sum[0][j];
        for (int w = 1; w < kBlock / 64; ++w) s += wave_sum[w][j];
    }
    return s;
}

// the lanes' NV sums -> the workgroup's partials part[blockIdx.x * NV + j]
template <int NV>
__device__ __forceinline__ void block_partials(double (&acc)[NV], double *__restrict__ part) {
    const double s = workgroup_sum<NV>(acc);
    if (threadIdx.x < NV) part[(long long)blockIdx.x * NV + threadIdx.x] = s;
}

// part[g * nv + j], g = 0 .. nparts, added in workgroup order by one workgroup; the sum in thread 0
__device__ __forceinline__ double fold_partials(const double *__restrict__ part, int nparts, int nv, int j) {
    double acc[1] = {0.0};
    for (int g = threadIdx.x; g < nparts; g += kBlock) acc[0] += part[(long long)g * nv + j];
    return workgroup_sum<1>(acc);
}

// The stop flags of the solvers with one right-hand side: kSolverFlagWords ints, zeroed with the solve's buffers.  Word
// kSolverState is kSolverRun (0) while the solve iterates; a vector kernel that finds anything else there returns
// before it writes, and so do pc_apply and the triangular solves' kernels, which are handed the same words.  A stop
// leaves the steps taken and the solver's status in words kSolverSteps and kSolverStatus; word 3 is the solver's own
// (BiCGSTAB's half step, MINRES's final step), and so are state values past kSolverStop.
constexpr int kSolverState = 0, kSolverSteps = 1, kSolverStatus = 2, kSolverFlagWords = 4;
constexpr int kSolverRun = 0, kSolverStop = 1;

// one thread: stop with `status` after `steps` steps
__device__ __forceinline__ void solver_stop(int *__restrict__ flags, int status, int steps, int state = kSolverStop) {
    flags[kSolverState] = state;
    flags[kSolverStatus] = status;
    flags[kSolverSteps] = steps;
}

// Kernels of more than one translation unit: internal linkage, one copy in each
namespace {

// grid nv: workgroup j folds part[g * nv + j] into out[j]
__global__ __launch_bounds__(kBlock) void solver_fold(const double *__restrict__ part, int nparts, int nv,
                                                      double *__restrict__ out) {
    const double s = fold_partials(part, nparts, nv, blockIdx.x);
    if (threadIdx.x == 0) out[blockIdx.x] = s;
}

// the ranks' nv sums (gathered[r * nv + j]) in rank order -> out[j]; one wavefront, nv <= 64
__global__ __launch_bounds__(64) void solver_rank_sum(const double *__restrict__ gathered, int ranks, int nv,
                                                      double *__restrict__ out) {
    const int j = threadIdx.x;
    if (j >= nv) return;
    double t = 0;
    for (int r = 0; r < ranks; ++r) t += gathered[r * nv + j];
    out[j] = t;
}

}  // namespace
}  // namespace spmv

// ---------------------------------------------------------------- the host side of a solve
// workgroups for `items` items at `per_block` each: at least 1, at most cap
inline int solver_grid(long long cap, long long items, long long per_block) {
    return (int)std::max<long long>(1, std::min<long long>(cap, (items + per_block - 1) / per_block));
}

// The refusals the entries share, each -1 with a message naming `what`; an entry calls them in its own order, with its
// own refusals in between.
inline int solver_check_steps(const char *what, int iters, double tol) {
    if (iters < 0) return fail("%s: iters = %d, must be >= 0", what, iters);
    if (!(tol >= 0) || !std::isfinite(tol)) return fail("%s: tol = %g, must be finite and >= 0", what, tol);
    return 0;
}
inline int solver_check_square(const char *what, const spmv_csr_dev *m) {
    if (m->M_total != m->N) return fail("%s: needs a square matrix (%d x %d)", what, m->M_total, m->N);
    return 0;
}
// the rows of a handle and the communicator fit together
inline int solver_check_rows(const char *what, const spmv_csr_dev *m, const int *bounds) {
    if (g_comm && !bounds) return fail("%s: a communicator exists, the row bounds are required", what);
    if (!g_comm && (m->row0 != 0 || m->M_local != m->M_total))
        return fail("%s: a handle of rows [%d, %d) needs a communicator", what, m->row0, m->row0 + m->M_local);
    if (g_comm_size > kMaxRanks) return fail("%s: more than %d ranks", what, kMaxRanks);
    return 0;
}

inline int solver_setup_failed(const char *what, hipError_t e) {
    return fail("%s: setup failed: %s", what, hipGetErrorString(e));
}
inline int solver_run_failed(const char *what, hipError_t e) {
    return fail("%s: run failed: %s", what, hipGetErrorString(e));
}

// the all-gatherv's row bounds for rows of k values (empty without a communicator)
inline std::vector<int> solver_scaled_bounds(const int *bounds, int k) {
    std::vector<int> kbounds;
    if (g_comm) {
        kbounds.resize((size_t)g_comm_size + 1);
        for (int r = 0; r <= g_comm_size; ++r) kbounds[r] = bounds[r] * k;
    }
    return kbounds;
}

// body(T()) with T the handle's dtype, under guarded()
template <typename F>
int solver_dispatch(const char *what, int value_bytes, F body) {
    return guarded(what, [&] { return value_bytes == 8 ? body(double()) : body(float()); });
}

namespace {

// part[g * nv + j] of this rank's `grid` workgroups -> out[j], the sums over all ranks, on every rank.  Without a
// communicator the fold alone; with one the rank's sums go to local[], are all-gathered into gath[r * nv + j] and added
// in rank order, so every rank holds the same bits whatever tree an all-reduce would pick.
[[maybe_unused]] int solver_reduce(const double *part, int grid, int nv, double *out, double *local, double *gath,
                                   const char *what) {
    hipLaunchKernelGGL(solver_fold, dim3(nv), dim3(kBlock), 0, g_stream, part, grid, nv, g_comm ? local : out);
    if (!g_comm) return 0;
    const ncclResult_t n = ncclAllGather(local, gath, (size_t)nv, ncclDouble, g_comm, g_stream);
    if (n != ncclSuccess) return fail("%s: ncclAllGather failed: %s", what, ncclGetErrorString(n));
    hipLaunchKernelGGL(solver_rank_sum, dim3(1), dim3(64), 0, g_stream, gath, g_comm_size, nv, out);
    return 0;
}

}  // namespace

// The device buffers and the two timing events of one solve.  alloc() zero-fills on g_stream; after the first error
// (kept in err) it allocates nothing more.  The destructor waits for g_stream -- nothing queued may outlive the
// buffers it uses --, frees everything and clears the last HIP error, which a failed allocation would otherwise leave
// for the next launch to report as its own.
struct SolverScope {
    hipError_t err = hipSuccess;
    hipEvent_t e0 = nullptr, e1 = nullptr;
    std::vector<void *> bufs;

    SolverScope() {
        err = hipEventCreate(&e0);
        if (err == hipSuccess) err = hipEventCreate(&e1);
    }
    SolverScope(const SolverScope &) = delete;
    SolverScope &operator=(const SolverScope &) = delete;
    ~SolverScope() {
        (void)hipStreamSynchronize(g_stream);
        for (void *p : bufs) (void)hipFree(p);
        if (e0) (void)hipEventDestroy(e0);
        if (e1) (void)hipEventDestroy(e1);
        (void)hipGetLastError();
    }
    template <typename P = void>
    P *alloc(size_t bytes) {
        void *p = nullptr;
        if (err == hipSuccess) err = hipMalloc(&p, bytes);
        if (err != hipSuccess) return nullptr;
        bufs.push_back(p);
        err = hipMemsetAsync(p, 0, bytes, g_stream);
        return (P *)p;
    }
};

// rows 0 .. steps_run of a device history of `row` doubles per row -> host (NULL: nothing); a solve that stopped early
// repeats its last row up to row iters
inline hipError_t copy_history(double *host, const double *dev, int steps_run, int iters, size_t row) {
    if (!host) return hipSuccess;
    const size_t run = ((size_t)steps_run + 1) * row, all = ((size_t)iters + 1) * row;
    const hipError_t e = hipMemcpy(host, dev, run * sizeof(double), hipMemcpyDeviceToHost);
    if (e == hipSuccess)
        for (size_t i = run; i < all; ++i) host[i] = host[i - row];
    return e;
}

// The start of a solve's timed part, after the allocations and the body's own copies of its input (e: their first
// error, beginning with scope.err): records e0.
inline int solver_begin(SolverScope &scope, hipError_t e, const char *what) {
    if (e == hipSuccess) e = hipEventRecord(scope.e0, g_stream);
    return e == hipSuccess ? 0 : solver_setup_failed(what, e);
}

struct SolverHistory {
    double *host;  // iters + 1 rows (NULL: not wanted)
    const double *dev;
};

// The end of a solve: records e1, all-gathers x_dev with `bounds` when a communicator exists and x is wanted (bounds
// NULL: every rank holds all of x), waits, takes the time, and copies to the host x (x_bytes; nothing for 0 bytes or
// a NULL x_host), the histories (rows of `row` doubles: 0 .. steps_run copied, the last one repeated up to iters) and
// flag_words ints of flags_dev (flags_host NULL: not read).  *ms_total (NULL: not wanted) is set on success only.
inline int solver_finish(SolverScope &scope, const char *what, int value_bytes, const int *bounds, void *x_dev,
                         void *x_host, size_t x_bytes, std::initializer_list<SolverHistory> hists, int steps_run,
                         int iters, size_t row, const int *flags_dev, int *flags_host, size_t flag_words,
                         float *ms_total) {
    hipError_t e = hipEventRecord(scope.e1, g_stream);
    // the solution: every rank holds its rows; with a communicator all rows everywhere
    if (e == hipSuccess && g_comm && x_host && bounds && spmv_hip_comm_allgatherv(x_dev, bounds, value_bytes, g_stream))
        return -1;
    if (e == hipSuccess) e = hipStreamSynchronize(g_stream);
    float ms = 0;
    if (e == hipSuccess) e = hipEventElapsedTime(&ms, scope.e0, scope.e1);
    if (e == hipSuccess && x_host && x_bytes) e = hipMemcpy(x_host, x_dev, x_bytes, hipMemcpyDeviceToHost);
    for (const SolverHistory &h : hists)
        if (e == hipSuccess) e = copy_history(h.host, h.dev, steps_run, iters, row);
    if (e == hipSuccess && flags_host)
        e = hipMemcpy(flags_host, flags_dev, flag_words * sizeof(int), hipMemcpyDeviceToHost);
    if (e != hipSuccess) return solver_run_failed(what, e);
    if (ms_total) *ms_total = ms;
    return 0;
}

constexpr int kSolverPoll = 16;  // tol > 0: steps between reads of the device's stop word

// after step t of iters with tol > 0, every kSolverPoll steps but the last: *stop = (the device int at word == value).
// Every rank holds the same bits, so every rank stops at the same step.
inline int solver_poll(int t, int iters, double tol, const int *word, int value, bool *stop) {
    *stop = false;
    if (!(tol > 0 && t % kSolverPoll == 0 && t < iters)) return 0;
    int v = 0;
    HIP_TRY(hipMemcpyAsync(&v, word, sizeof(int), hipMemcpyDeviceToHost, g_stream));
    HIP_TRY(hipStreamSynchronize(g_stream));
    *stop = v == value;
    return 0;
}
