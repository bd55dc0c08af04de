// spmv_amg_setup.hip -- spmv_hip_csr_precond_build_amg_device: the setup of the AMG preconditioner on the device
// (include/spmv_hip.h; the kernels are in amg_setup_kernels.hpp).  The definition is the host setup, host/amg_plan.c:
// for every handle and argument set on which spmv_hip_csr_precond_build_amg succeeds this gives the same object byte for
// byte, and where that refuses this refuses in the same words.
//
// The level loop, on fp64 device arrays (the host only orchestrates):
//
//   level 0     the canonical diagonal block (canon_rows.hpp) uploaded as bare arrays
//   statistics  as_row_stats: d, the lowest bad diagonal, rho = max q (a NaN or an infinity anywhere: refused); w on the host
//   kind        DIRECT (n_l <= coarse_rows: A_l downloaded, amg_dense_inverse on the host), max_levels and the stall rule
//               decided on the host as amg_plan.c does
//   strength    as_strong_count, an exclusive scan, as_strong_emit (both directions of every strong entry), a radix sort
//               of the keys on the bits in use, repeats dropped, as_graph; s_rp and s_col go to the host
//   aggregates  amg_aggregate on the host (serial by definition); T from agg on the host, uploaded
//   P           A T by the product core, as_smooth in place
//   R           P^T by the transpose core (a stable sort: csr_transpose's order)
//   A_{l+1}     A P, then R (A P) by the product core (the serial sum of csr_multiply by definition)
//   rounding    as_g and as_round: g_l, A_l (l > 0), P_l, R_l in the handle's dtype, once; a value that is not finite there
//               is refused in the host setup's words -- but only after the hierarchy is complete, because the host setup
//               makes its whole plan before it rounds anything: a refusal of the plan at a deeper level comes first
//
// Transient device memory: the fp64 A_l, T_l, P_l, R_l and A_l P_l of ONE level, the next level's A, the keys of the
// strength graph (twice: the sort's output) and the product core's workspace; each is freed as soon as the next step has
// what it needs.  amg_finish (spmv_amg.hip) then makes the cycle, the tail and the workspace as for a host-built P.
#include "amg_levels.hpp"
#include "algebra_ops.hpp"

#include <climits>
#include <memory>

#include <rocprim/rocprim.hpp>

#include "../host/amg_plan_parts.h"
#include "amg_setup_kernels.hpp"
#include "canon_rows.hpp"

namespace {

int grid_for(long long items, int per_block = kBlock) {
    return (int)std::max<long long>(1, std::min<long long>(kAsMaxGrid, (items + per_block - 1) / per_block));
}

using algebra::bits_for;

template <typename V>
int upload_async(V *dst, const V *src, size_t count) {
    if (count) HIP_TRY(hipMemcpyAsync(dst, src, count * sizeof(V), hipMemcpyHostToDevice, g_stream));
    return 0;
}
template <typename V>
int download(V *dst, const V *src, size_t count) {  // waits for the stream: what was launched before has run
    if (count) HIP_TRY(hipMemcpyAsync(dst, src, count * sizeof(V), hipMemcpyDeviceToHost, g_stream));
    HIP_TRY(hipStreamSynchronize(g_stream));
    return 0;
}

// bare fp64 device arrays of host CSR arrays (a level's own: no pad behind the entries)
int csr_to_device(int rows, int cols, const int *rp, const int *col, const double *val, DevCsr &out) {
    const size_t nz = (size_t)rp[rows];
    out = DevCsr(rows, cols);
    HIP_TRY(out.alloc_rp());
    HIP_TRY(out.alloc_entries<double>((long long)nz, 0, g_stream));
    if (upload_async(out.rp, rp, (size_t)rows + 1) || upload_async(out.col, col, nz) ||
        upload_async((double *)out.val, val, nz))
        return -1;
    HIP_TRY(hipStreamSynchronize(g_stream));  // the host arrays may go away
    return 0;
}

// the strength graph of A on the host: s_rp[n + 1], s_col; 1: more edges than an int counts
int strength_graph(const CsrView &A, const double *d, double theta, std::vector<int> &s_rp, std::vector<int> &s_col) {
    const int n = A.rows;
    const unsigned col_bits = bits_for((unsigned long long)n);
    DevBuf d_cnt, d_off, d_tmp;
    hipError_t e = d_cnt.alloc(((size_t)n + 1) * sizeof(int));
    if (e == hipSuccess) e = d_off.alloc(((size_t)n + 1) * sizeof(long long));
    if (e == hipSuccess) e = hipMemsetAsync(d_cnt.p, 0, ((size_t)n + 1) * sizeof(int), g_stream);
    if (e != hipSuccess) return fail("csr_precond_build_amg_device: allocation of the strength counts failed: %s", hipGetErrorString(e));
    hipLaunchKernelGGL(as_strong_count, dim3(grid_for(n)), dim3(kBlock), 0, g_stream, n, A.rp, A.col, (const double *)A.val, d,
                       theta, d_cnt.as<int>());
    size_t tmp_bytes = 0;
    HIP_TRY(rocprim::exclusive_scan(nullptr, tmp_bytes, d_cnt.as<int>(), d_off.as<long long>(), 0LL, (size_t)n + 1,
                                    rocprim::plus<long long>(), g_stream));
    HIP_TRY(d_tmp.alloc(tmp_bytes));
    HIP_TRY(rocprim::exclusive_scan(d_tmp.p, tmp_bytes, d_cnt.as<int>(), d_off.as<long long>(), 0LL, (size_t)n + 1,
                                    rocprim::plus<long long>(), g_stream));
    long long strong = 0;
    if (download(&strong, d_off.as<long long>() + n, 1)) return -1;
    s_rp.assign((size_t)n + 1, 0);
    s_col.clear();
    if (!strong) return 0;  // no row has a neighbour
    const size_t keys = (size_t)strong * 2;
    DevBuf d_kin, d_kout, d_sort, d_count, d_srp, d_scol;
    e = d_kin.alloc(keys * 8);
    if (e == hipSuccess) e = d_kout.alloc(keys * 8);
    if (e == hipSuccess) e = d_count.alloc(sizeof(unsigned long long));
    if (e == hipSuccess) e = d_srp.alloc(((size_t)n + 1) * sizeof(int));
    if (e != hipSuccess)
        return fail("csr_precond_build_amg_device: allocation of %zu strength keys failed: %s", keys, hipGetErrorString(e));
    hipLaunchKernelGGL(as_strong_emit, dim3(grid_for(n)), dim3(kBlock), 0, g_stream, n, A.rp, A.col, (const double *)A.val, d,
                       theta, (int)col_bits, d_off.as<long long>(), d_kin.as<unsigned long long>());
    unsigned long long *kin = d_kin.as<unsigned long long>(), *kout = d_kout.as<unsigned long long>();
    size_t sort_bytes = 0, unique_bytes = 0;
    HIP_TRY(rocprim::radix_sort_keys(nullptr, sort_bytes, kin, kout, keys, 0u, 2 * col_bits, g_stream));
    HIP_TRY(rocprim::unique(nullptr, unique_bytes, kout, kin, d_count.as<unsigned long long>(), keys,
                            rocprim::equal_to<unsigned long long>(), g_stream));
    HIP_TRY(d_sort.alloc(std::max(sort_bytes, unique_bytes)));
    HIP_TRY(rocprim::radix_sort_keys(d_sort.p, sort_bytes, kin, kout, keys, 0u, 2 * col_bits, g_stream));
    HIP_TRY(rocprim::unique(d_sort.p, unique_bytes, kout, kin, d_count.as<unsigned long long>(), keys,
                            rocprim::equal_to<unsigned long long>(), g_stream));  // kin: the edges, sorted, once each
    unsigned long long edges = 0;
    if (download(&edges, d_count.as<unsigned long long>(), 1)) return -1;
    if (edges > (unsigned long long)INT_MAX) return 1;  // beyond the host setup's int counts
    HIP_TRY(d_scol.alloc((size_t)edges * sizeof(int)));
    const long long E = (long long)edges;
    hipLaunchKernelGGL(as_graph, dim3((unsigned)((E + kBlock) / kBlock)), dim3(kBlock), 0, g_stream, E, n, (int)col_bits, kin,
                       d_srp.as<int>(), d_scol.as<int>());
    HIP_TRY(hipGetLastError());
    s_col.assign((size_t)edges, 0);
    HIP_TRY(hipMemcpyAsync(s_rp.data(), d_srp.p, ((size_t)n + 1) * sizeof(int), hipMemcpyDeviceToHost, g_stream));
    return download(s_col.data(), d_scol.as<int>(), (size_t)edges);
}

// src's values rounded once to T as op (flag: set when one is not finite in T).  take: op takes src's row_ptr and col
// (src keeps its values alone); else it gets copies
template <typename T>
int round_op(DevCsr &src, bool take, AmgOp &op, int *d_flag) {
    const size_t nz = (size_t)src.nz;
    op.shape(src.rows, src.nz);
    HIP_TRY(hipMalloc(&op.val, std::max<size_t>(nz, 4) * sizeof(T)));
    if (nz)
        hipLaunchKernelGGL((as_round<T>), dim3(grid_for(src.nz)), dim3(kBlock), 0, g_stream, src.nz, (const double *)src.val,
                           (T *)op.val, d_flag);
    HIP_TRY(hipGetLastError());
    if (take) {
        op.rp = src.rp, op.col = src.col;
        src.rp = src.col = nullptr;
        return 0;
    }
    HIP_TRY(hipMalloc((void **)&op.rp, ((size_t)src.rows + 1) * sizeof(int)));
    HIP_TRY(hipMalloc((void **)&op.col, std::max<size_t>(nz, 4) * sizeof(int)));
    HIP_TRY(hipMemcpyAsync(op.rp, src.rp, ((size_t)src.rows + 1) * sizeof(int), hipMemcpyDeviceToDevice, g_stream));
    if (nz) HIP_TRY(hipMemcpyAsync(op.col, src.col, nz * sizeof(int), hipMemcpyDeviceToDevice, g_stream));
    return 0;
}

struct HostFree {
    void operator()(double *p) const { free(p); }
};

template <typename T>
int amg_build_device(const spmv_csr_dev *m, double theta, int coarse_rows, int max_levels, int chain, int block_products,
                     spmv_precond **out) {
    const double t0 = now_ms();
    Canon A;
    if (canon_download<T>(m, A)) return -1;
    const int n = A.n;
    const double t1 = now_ms();
    std::unique_ptr<spmv_amg_precond> ap(new spmv_amg_precond);
    ap->chain = chain != 0;
    ap->setup = kAmgSetupDevice;
    double phase_ms[kAmgPhases] = {};
    double t_lap = now_ms();
    auto lap = [&](int phase) -> int {  // the device work launched so far belongs to this phase
        HIP_TRY(hipStreamSynchronize(g_stream));
        const double t = now_ms();
        phase_ms[phase] += t - t_lap;
        t_lap = t;
        return 0;
    };
    auto plan_refusal = [&](const char *fmt, auto... args) {
        char msg[200];
        snprintf(msg, sizeof msg, fmt, args...);
        return fail(kAmgMsgPlan, m->row0, msg);
    };
    std::string deferred;  // the first refusal of the rounding, in the host setup's order
    auto defer = [&](const char *fmt, auto... args) {
        if (!deferred.empty()) return;
        char msg[200];
        snprintf(msg, sizeof msg, fmt, args...);
        deferred = msg;
    };
    enum { kFlagG = 0, kFlagA, kFlagP, kFlagR, kFlags };  // kFlagG: a row, the others 0 / 1
    DevBuf d_flags, d_res;
    HIP_TRY(d_flags.alloc(kFlags * sizeof(int)));
    HIP_TRY(d_res.alloc(kAsStatWords * sizeof(unsigned long long)));

    DevCsr cur;  // A_l in fp64; like every level's arrays below, freed on every way out
    if (n && csr_to_device(n, n, A.rp.data(), A.col.data(), A.val.data(), cur)) return -1;
    for (int l = 0; n && l < kAmgMaxLevels; ++l) {
        const int nl = cur.rows;
        ap->levels = l + 1;
        ap->n[l] = nl;
        ap->a_nz[l] = cur.nz;
        t_lap = now_ms();

        // ---- row statistics
        DevBuf d_d;
        HIP_TRY(d_d.alloc((size_t)nl * sizeof(double)));
        const unsigned long long res0[kAsStatWords] = {~0ull, 0, 0};
        unsigned long long res[kAsStatWords];
        if (upload_async(d_res.as<unsigned long long>(), res0, kAsStatWords)) return -1;
        hipLaunchKernelGGL(as_row_stats, dim3(grid_for(nl)), dim3(kBlock), 0, g_stream, nl, cur.rp, cur.col,
                           (const double *)cur.val, d_d.as<double>(), d_res.as<unsigned long long>());
        HIP_TRY(hipGetLastError());
        if (download(res, d_res.as<unsigned long long>(), kAsStatWords) || lap(kAmgPhStats)) return -1;
        if (res[kAsBadRow] != ~0ull) {
            const int row = (int)(res[kAsBadRow] >> 1);
            const char *why = (res[kAsBadRow] & 1) ? AMG_WHY_BAD_DIAGONAL : AMG_WHY_NO_DIAGONAL;
            return l == 0 ? plan_refusal(AMG_REFUSE_ROW, row, why) : plan_refusal(AMG_REFUSE_COARSE_ROW, l, row, why);
        }
        double rho;
        memcpy(&rho, &res[kAsMaxQ], sizeof rho);
        if (res[kAsNotFinite] || !(rho > 0.0)) return plan_refusal(AMG_REFUSE_NOT_FINITE, l);
        const double w = 4.0 / (3.0 * rho);
        ap->rho[l] = rho, ap->w[l] = w;

        // ---- the level's kind: DIRECT and max_levels now, the stall rule after the aggregation
        int kind = SPMV_AMG_SMOOTH;
        if (nl <= coarse_rows) kind = SPMV_AMG_DIRECT;
        std::vector<int> agg;
        int na = 0;
        if (kind == SPMV_AMG_SMOOTH && l + 1 < max_levels) {
            std::vector<int> s_rp, s_col;
            const int over = strength_graph(cur.view(), d_d.as<double>(), theta, s_rp, s_col);
            if (over > 0) return plan_refusal("%s", AMG_REFUSE_MEMORY);
            if (over || lap(kAmgPhStrength)) return -1;
            agg.assign((size_t)nl + 1, -1);
            s_col.push_back(0);  // (never read: data() of an empty vector may be NULL)
            na = amg_aggregate(nl, s_rp.data(), s_col.data(), agg.data());
            if (na < 0) return plan_refusal("%s", AMG_REFUSE_MEMORY);
            if (lap(kAmgPhAggregate)) return -1;
            if (!(na == 0 || 10LL * na > 9LL * nl)) kind = SPMV_AMG_NOT_COARSEST;
        }
        ap->kind[l] = kind;
        ap->na[l] = kind == SPMV_AMG_NOT_COARSEST ? na : 0;

        // ---- g and A_l in the handle's dtype (level 0 that is not DIRECT: the ordinary upload below)
        const int flags0[kFlags] = {INT_MAX, 0, 0, 0};
        int flags[kFlags];
        if (upload_async(d_flags.as<int>(), flags0, kFlags)) return -1;
        HIP_TRY(hipMalloc((void **)&ap->g[l], std::max<size_t>((size_t)nl, 4) * sizeof(double)));
        hipLaunchKernelGGL((as_g<T>), dim3(grid_for(nl)), dim3(kBlock), 0, g_stream, nl, d_d.as<double>(), w, ap->g[l],
                           d_flags.as<int>() + kFlagG);
        if (!(l == 0 && kind != SPMV_AMG_DIRECT) && round_op<T>(cur, false, ap->A[l], d_flags.as<int>() + kFlagA)) return -1;
        if (lap(kAmgPhRound)) return -1;

        if (kind == SPMV_AMG_DIRECT) {
            if (download(flags, d_flags.as<int>(), kFlags)) return -1;
            if (flags[kFlagG] != INT_MAX) defer(kAmgMsgDiagonal, l, flags[kFlagG]);
            if (flags[kFlagA]) defer(kAmgMsgEntry, l, "A");
            HostOp h;
            h.rp.assign((size_t)nl + 1, 0);
            if (download(h.rp.data(), cur.rp, (size_t)nl + 1)) return -1;
            const size_t nz = (size_t)h.rp[(size_t)nl];
            h.col.assign(nz + 1, 0), h.val.assign(nz + 1, 0.0);
            HIP_TRY(hipMemcpyAsync(h.col.data(), cur.col, nz * sizeof(int), hipMemcpyDeviceToHost, g_stream));
            if (download(h.val.data(), (const double *)cur.val, nz)) return -1;
            const amg_csr Al = {nl, nl, h.rp.data(), h.col.data(), h.val.data()};
            double *inv_raw = nullptr;
            const int bad = amg_dense_inverse(&Al, &inv_raw);
            std::unique_ptr<double, HostFree> inv(inv_raw);
            if (bad < 0) return plan_refusal("%s", AMG_REFUSE_MEMORY);
            if (bad) return plan_refusal(AMG_REFUSE_PIVOT, l, nl);
            if (lap(kAmgPhInverse)) return -1;
            if (deferred.empty()) {
                h.col.resize((size_t)nl * nl), h.val.assign(inv.get(), inv.get() + (size_t)nl * nl);
                for (int i = 0; i <= nl; ++i) h.rp[(size_t)i] = i * nl;
                for (int i = 0; i < nl; ++i)
                    for (int j = 0; j < nl; ++j) h.col[(size_t)i * nl + j] = j;
                if (amg_op_upload<T>(h, nl, ap->inv, "the inverse", l)) return -1;
            }
            if (lap(kAmgPhRound)) return -1;
            break;
        }
        if (kind == SPMV_AMG_SMOOTH) {
            if (download(flags, d_flags.as<int>(), kFlags)) return -1;
            if (flags[kFlagG] != INT_MAX) defer(kAmgMsgDiagonal, l, flags[kFlagG]);
            if (flags[kFlagA]) defer(kAmgMsgEntry, l, "A");
            break;
        }

        // ---- T from agg (host), P = T - diag(w / d) A T
        DevCsr Tm, Pm, Rm, APm, next;
        std::vector<int> rp_host;
        DevBuf d_agg;
        {
            std::vector<int> t_rp((size_t)nl + 1, 0), t_col;
            t_col.reserve((size_t)nl);
            for (int i = 0; i < nl; ++i) {
                if (agg[(size_t)i] >= 0) t_col.push_back(agg[(size_t)i]);
                t_rp[(size_t)i + 1] = (int)t_col.size();
            }
            const std::vector<double> ones(t_col.size() + 1, 1.0);
            t_col.push_back(0);
            HIP_TRY(d_agg.alloc((size_t)nl * sizeof(int)));
            if (upload_async(d_agg.as<int>(), agg.data(), (size_t)nl) ||
                csr_to_device(nl, na, t_rp.data(), t_col.data(), ones.data(), Tm))
                return -1;
        }
        if (spgemm_core(8, cur.view(), Tm.view(), block_products, 0, Pm, rp_host, nullptr, nullptr)) return -1;
        Tm = DevCsr();
        hipLaunchKernelGGL(as_smooth, dim3(grid_for(nl, kBlock / kAsSmoothLanes)), dim3(kBlock), 0, g_stream, nl, Pm.rp,
                           Pm.col, (double *)Pm.val, d_agg.as<int>(), d_d.as<double>(), w);
        HIP_TRY(hipGetLastError());
        if (lap(kAmgPhTentative)) return -1;
        // ---- R = P^T, A_{l+1} = R (A P)
        if (transpose_core(8, Pm.view(), Rm, rp_host) || lap(kAmgPhTranspose)) return -1;
        if (spgemm_core(8, cur.view(), Pm.view(), block_products, 0, APm, rp_host, nullptr, nullptr) || lap(kAmgPhAP)) return -1;
        if (spgemm_core(8, Rm.view(), APm.view(), block_products, 0, next, rp_host, nullptr, nullptr) || lap(kAmgPhRAP)) return -1;
        APm = DevCsr();
        // ---- P_l and R_l in the handle's dtype
        if (round_op<T>(Pm, true, ap->P[l], d_flags.as<int>() + kFlagP) ||
            round_op<T>(Rm, true, ap->R[l], d_flags.as<int>() + kFlagR) || download(flags, d_flags.as<int>(), kFlags))
            return -1;
        if (flags[kFlagG] != INT_MAX) defer(kAmgMsgDiagonal, l, flags[kFlagG]);
        if (flags[kFlagA]) defer(kAmgMsgEntry, l, "A");
        if (flags[kFlagP]) defer(kAmgMsgEntry, l, "P");
        if (flags[kFlagR]) defer(kAmgMsgEntry, l, "R");
        if (lap(kAmgPhRound)) return -1;
        cur = std::move(next);
    }
    cur = DevCsr();
    if (!deferred.empty()) return fail("%s", deferred.c_str());
    const double t2 = now_ms();
    // level 0 is the ordinary upload of the canonical block, as in the host setup
    if (ap->levels && ap->kind[0] != SPMV_AMG_DIRECT) {
        int rc;
        if constexpr (sizeof(T) == 8) {
            rc = spmv_hip_csr_upload(n, n, A.rp.data(), A.col.data(), A.val.data(), 0, n, &ap->A0);
        } else {
            std::vector<float> v(A.val.begin(), A.val.end());
            rc = spmv_hip_csr_upload_f32(n, n, A.rp.data(), A.col.data(), v.data(), 0, n, &ap->A0);
        }
        if (rc) return -1;
    }
    if (amg_finish(ap.get(), (int)sizeof(T))) return -1;
    for (int p = 0; p < kAmgPhases; ++p) ap->phase_us[p] = (int)(phase_ms[p] * 1e3);
    ap->us[0] = (int)((t1 - t0) * 1e3);
    ap->us[1] = (int)((t2 - t1) * 1e3);
    ap->us[2] = (int)((now_ms() - t2) * 1e3);
    *out = amg_wrap(m, ap.release(), sizeof(T));
    return 0;
}

}  // namespace

extern "C" int spmv_hip_csr_precond_build_amg_device(const spmv_csr_dev *m, double theta, int coarse_rows, int max_levels,
                                                     int chain, int block_products, spmv_precond **out) {
    // (the host setup's prefix throughout, so that both setups refuse in the same words; block_products is this one's own)
    auto check = [&] {
        if (amg_check_args(theta, coarse_rows, max_levels)) return -1;
        if (!spgemm_block_products_ok(block_products))
            return fail("csr_precond_build_amg_device: block_products = %d; 0 (auto), -1 (no on-chip tier) or a power of two "
                        "in [64, %d]", block_products, spgemm_max_block_products());
        return 0;
    };
    return precond_build_frame("csr_precond_build_amg", m, out, check, [&](auto t, spmv_precond **P) {
        return amg_build_device<decltype(t)>(m, theta, coarse_rows, max_levels, chain, block_products, P);
    });
}

extern "C" int spmv_hip_precond_amg_setup_info(const spmv_precond *P, int *info) {
    if (!P || !info) return fail("precond_amg_setup_info: bad arguments");
    const spmv_amg_precond *ap = amg_of(P, "precond_amg_setup_info");
    if (!ap) return -1;
    info[0] = ap->setup;
    for (int p = 0; p < kAmgPhases; ++p) info[1 + p] = ap->setup == kAmgSetupDevice ? ap->phase_us[p] : 0;
    return 0;
}
