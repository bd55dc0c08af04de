// lobpcg_kernels.hpp -- the kernels of spmv_hip_csr_lobpcg (gfx950): the two tall-skinny dense passes over the basis
// S = [X | W | P], AS = [AX | AW | AP], the residual pass and ||A||_inf.
//
// Every block of the basis is a row-major n x k fp64 array (element (i, j) at i * k + j, the SpMM's layout), k <= 16,
// nb <= 3 blocks: m = nb * k <= 48 logical columns, logical column c = column c % k of block c / k.
//
//   lob_gram<MT>      G_B = S^T S and G_A = S^T AS in one pass, MT = ceil(m / 16) tiles of 16 columns.  A GEMM with a
//                     very long inner dimension: v_mfma_f64_16x16x4_f64 takes 4 rows per instruction, lane l supplies
//                     row l >> 4, column l & 15 of a tile to both operands, straight from global loads (one value per
//                     lane and tile: no LDS on the way in).  Pad columns (c >= m) and rows >= n supply 0 and are not
//                     loaded.  A wave keeps the upper-triangle tiles of G_B and all tiles of G_A in registers, at most
//                     6 + 9 tiles of 4 doubles per lane; the accumulator of lane l, register r is row (l >> 4) + 4 r,
//                     column l & 15 of its tile (the f64 layout, not the f32 one).
//   lob_update<NB,KP,VEC> X = S C, P = S Cp, AX = AS C, AP = AS Cp.  A lane owns a row and keeps its m values of S and of
//                     AS in registers; {C, Cp} pairs are staged per workgroup in LDS (KP = k rounded up to 4, 8 or 16;
//                     the pad is 0) and read as wave-uniform 16-byte broadcasts, one per four FMAs.  The outputs may be
//                     the inputs: a row is read completely before it is written.  Plain VALU.
//   lob_residual<V>   R = AX - X diag(theta) and the workgroup partials of ||r_j||^2, cg_multi's lane shape and sums.
//   lob_row_abs_max / lob_max   anorm: row sums of |a| in entry order, then a maximum (exact, no order issues).
//
// Reduction order of lob_gram: a wave walks its row groups (4 rows) in grid-stride order, the waves of a workgroup are
// added in wave order through LDS, one tile at a time, the workgroups by solver_fold in workgroup order.  No atomics.
//
// Registers and grids.  lob_gram<3> holds 15 tiles x 4 doubles = 120 VGPRs of accumulators and two sets of 6 operand
// values (the next row group is loaded before this one's 15 MFMAs): it is compiled for 256-thread workgroups without a
// waves-per-SIMD promise, so the compiler may take every register a lone wave of a SIMD can have rather than spill.
// The grid is capped at kLobGramBlocks = 512 workgroups.  lob_gram<3> takes 288 registers, so a SIMD holds one of its
// waves and a CU one workgroup: on a 256-CU chip its 512 workgroups run as two rounds (256 would fold half as many
// partials; not measured).  lob_gram<2> and lob_gram<1> (about 150 and 60 registers) fit several workgroups per CU;
// caps of 1024 and 2048 for them were measured and gained nothing (profiles/lobpcg_step.md).  Every workgroup leaves
// 2 (16 MT)^2 doubles to fold.  lob_update<3, 16> holds 96 row values; kLobUpdateBlocks = 256 workgroups of 256 rows.
// LDS: lob_gram 8 KB (4 waves x 256 doubles), lob_update NB * KP * KP * 16 bytes <= 12 KB.
#pragma once
#include "cg_multi_kernels.hpp"

namespace spmv {

constexpr int kLobMaxK = 16;           // widest block
constexpr int kLobMaxBlocks = 3;       // X, W, P
constexpr int kLobGramBlocks = 512;    // grid cap of lob_gram: 16 rows per workgroup pass
constexpr int kLobUpdateBlocks = 256;  // grid cap of lob_update: 256 rows per workgroup pass

typedef double v4d __attribute__((ext_vector_type(4)));

template <int MT>
__global__ __launch_bounds__(kBlock) void lob_gram(long long n, int k, int m, const double *S0, const double *S1,
                                                   const double *S2, const double *A0, const double *A1,
                                                   const double *A2, double *__restrict__ part) {
    constexpr int NG = MT * (MT + 1) / 2, NA = MT * MT, MP = MT * 16;
    __shared__ double wbuf[kBlock / 64][256];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int c16 = lane & 15, r4 = lane >> 4;
    // the lane's column of every tile: element (0, j) of its block, or nullptr for a pad column
    const double *ps[MT], *pa[MT];
#pragma unroll
    for (int t = 0; t < MT; ++t) {
        const int c = t * 16 + c16;
        const int b = c / k, j = c - b * k;
        const bool real = c < m;
        ps[t] = real ? (b == 0 ? S0 : b == 1 ? S1 : S2) + j : nullptr;
        pa[t] = real ? (b == 0 ? A0 : b == 1 ? A1 : A2) + j : nullptr;
    }
    v4d gb[NG], ga[NA];
#pragma unroll
    for (int i = 0; i < NG; ++i) gb[i] = v4d{0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int i = 0; i < NA; ++i) ga[i] = v4d{0.0, 0.0, 0.0, 0.0};
    const long long groups = (n + 3) >> 2, stride = (long long)gridDim.x * (kBlock / 64);
    long long g = (long long)blockIdx.x * (kBlock / 64) + wave;
    double s[MT], a[MT], sn[MT], an[MT];
    auto load = [&](long long grp, double(&sv)[MT], double(&av)[MT]) {
        const long long row = grp * 4 + r4;
        const bool in = grp < groups && row < n;
#pragma unroll
        for (int t = 0; t < MT; ++t) {
            const bool ok = in && ps[t] != nullptr;
            sv[t] = ok ? ps[t][row * k] : 0.0;
            av[t] = ok ? pa[t][row * k] : 0.0;
        }
    };
    load(g, s, a);
    for (; g < groups; g += stride) {
        load(g + stride, sn, an);  // the next group's loads fly while this one's MFMAs run
        int q = 0;
#pragma unroll
        for (int ti = 0; ti < MT; ++ti) {
#pragma unroll
            for (int tj = ti; tj < MT; ++tj, ++q) gb[q] = __builtin_amdgcn_mfma_f64_16x16x4f64(s[ti], s[tj], gb[q], 0, 0, 0);
        }
#pragma unroll
        for (int ti = 0; ti < MT; ++ti) {
#pragma unroll
            for (int tj = 0; tj < MT; ++tj)
                ga[ti * MT + tj] = __builtin_amdgcn_mfma_f64_16x16x4f64(s[ti], a[tj], ga[ti * MT + tj], 0, 0, 0);
        }
#pragma unroll
        for (int t = 0; t < MT; ++t) s[t] = sn[t], a[t] = an[t];
    }
    // the workgroup's sums, tile by tile: element e = r * 64 + l of a tile is row (l >> 4) + 4 r, column l & 15
    double *out = part + (long long)blockIdx.x * (2 * MP * MP);
    const int e = threadIdx.x, el = e & 63, er = e >> 6;
    const int erow = (el >> 4) + 4 * er, ecol = el & 15;
    auto reduce_tile = [&](const v4d &v, int which, int ti, int tj) {
        wbuf[wave][0 * 64 + lane] = v.x;
        wbuf[wave][1 * 64 + lane] = v.y;
        wbuf[wave][2 * 64 + lane] = v.z;
        wbuf[wave][3 * 64 + lane] = v.w;
        __syncthreads();
        double sum = wbuf[0][e];
        for (int w = 1; w < kBlock / 64; ++w) sum += wbuf[w][e];
        out[which * MP * MP + (ti * 16 + erow) * MP + tj * 16 + ecol] = sum;
        __syncthreads();
    };
    int q = 0;
#pragma unroll
    for (int ti = 0; ti < MT; ++ti) {
#pragma unroll
        for (int tj = ti; tj < MT; ++tj, ++q) reduce_tile(gb[q], 0, ti, tj);
    }
#pragma unroll
    for (int ti = 0; ti < MT; ++ti) {
#pragma unroll
        for (int tj = 0; tj < MT; ++tj) reduce_tile(ga[ti * MT + tj], 1, ti, tj);
    }
}

// coef: m x k pairs {C[c][j], Cp[c][j]} (element (c, j) at 2 (c k + j)).  VEC: k is even and every array is 16-byte
// aligned: a row is loaded and stored in 16-byte pieces and two output columns are made at a time (the same sums in the
// same order: the same bits as VEC = false)
template <int NB, int KP, bool VEC>
__global__ __launch_bounds__(kBlock) void lob_update(long long n, int k, const double *S0, const double *S1,
                                                     const double *S2, const double *A0, const double *A1,
                                                     const double *A2, const double *__restrict__ coef, double *X,
                                                     double *P, double *AX, double *AP) {
    __shared__ v2d cl[NB * KP * KP];
    for (int i = threadIdx.x; i < NB * KP * KP; i += kBlock) {
        const int j = i % KP, c = (i / KP) % KP, b = i / (KP * KP);
        v2d v = {0.0, 0.0};
        if (c < k && j < k) v = *reinterpret_cast<const v2d *>(coef + 2 * ((long long)(b * k + c) * k + j));
        cl[i] = v;
    }
    __syncthreads();
    const double *Sb[3] = {S0, S1, S2}, *Ab[3] = {A0, A1, A2};
    const long long stride = (long long)gridDim.x * kBlock;
    constexpr int W = VEC ? 2 : 1;  // columns per load, store and pass over the coefficients
    for (long long row = (long long)blockIdx.x * kBlock + threadIdx.x; row < n; row += stride) {
        const long long o = row * k;
        double s[NB][KP], a[NB][KP];
#pragma unroll
        for (int b = 0; b < NB; ++b) {
#pragma unroll
            for (int c = 0; c < KP; c += W) {
                double sv[W], av[W];
#pragma unroll
                for (int w = 0; w < W; ++w) sv[w] = av[w] = 0.0;
                if (c < k) {
                    piece_load<double, W>(Sb[b] + o + c, sv);
                    piece_load<double, W>(Ab[b] + o + c, av);
                }
#pragma unroll
                for (int w = 0; w < W; ++w) s[b][c + w] = sv[w], a[b][c + w] = av[w];
            }
        }
        for (int j = 0; j < k; j += W) {
            double x[W], p[W], ax[W], ap[W];
#pragma unroll
            for (int w = 0; w < W; ++w) x[w] = p[w] = ax[w] = ap[w] = 0.0;
#pragma unroll
            for (int b = 0; b < NB; ++b) {
#pragma unroll
                for (int c = 0; c < KP; ++c) {
#pragma unroll
                    for (int w = 0; w < W; ++w) {
                        const v2d q = cl[(b * KP + c) * KP + j + w];
                        x[w] += s[b][c] * q.x;
                        p[w] += s[b][c] * q.y;
                        ax[w] += a[b][c] * q.x;
                        ap[w] += a[b][c] * q.y;
                    }
                }
            }
            piece_store<double, W>(X + o + j, x);
            piece_store<double, W>(P + o + j, p);
            piece_store<double, W>(AX + o + j, ax);
            piece_store<double, W>(AP + o + j, ap);
        }
    }
}

// R = AX - X diag(theta) (R == nullptr: not stored) and the workgroup's partials of ||r_j||^2
template <int V>
__global__ __launch_bounds__(kBlock) void lob_residual(long long n, int k, int cl, const double *__restrict__ theta,
                                                       const double *__restrict__ X, const double *__restrict__ AX,
                                                       double *__restrict__ R, double *__restrict__ part) {
    const McgLane l(cl, V);
    double acc[V], th[V];
#pragma unroll
    for (int v = 0; v < V; ++v) {
        acc[v] = 0;
        th[v] = l.j0 + v < k ? theta[l.j0 + v] : 0.0;
    }
    if (l.j0 < k) {
        for (long long i = l.row; i < n; i += l.stride) {
            const long long o = i * k + l.j0;
            double xv[V], av[V];
            piece_load<double, V>(X + o, xv);
            piece_load<double, V>(AX + o, av);
#pragma unroll
            for (int v = 0; v < V; ++v) {
                av[v] -= th[v] * xv[v];
                acc[v] += av[v] * av[v];
            }
            if (R) piece_store<double, V>(R + o, av);
        }
    }
    mcg_block_partials<V>(acc, k, cl, l.j0, part);
}

// part[workgroup] = the largest row sum of |a| among the workgroup's rows (a row's entries added in entry order)
__global__ __launch_bounds__(kBlock) void lob_row_abs_max(long long n, const int *__restrict__ row_ptr,
                                                          const double *__restrict__ val, double *__restrict__ part) {
    __shared__ double wave_max[kBlock / 64];
    double mx = 0.0;
    for (long long i = (long long)blockIdx.x * kBlock + threadIdx.x; i < n; i += (long long)gridDim.x * kBlock) {
        double s = 0.0;
        for (int e = row_ptr[i]; e < row_ptr[i + 1]; ++e) s += fabs(val[e]);
        mx = s > mx || s != s ? s : mx;
    }
    for (int step = 32; step >= 1; step >>= 1) {
        const double o = __shfl_xor(mx, step);
        mx = o > mx || o != o ? o : mx;
    }
    if ((threadIdx.x & 63) == 0) wave_max[threadIdx.x >> 6] = mx;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < kBlock / 64; ++w) mx = wave_max[w] > mx || wave_max[w] != wave_max[w] ? wave_max[w] : mx;
        part[blockIdx.x] = mx;
    }
}

// one workgroup: out[0] = max part[0 .. nparts)
__global__ __launch_bounds__(kBlock) void lob_max(const double *__restrict__ part, int nparts, double *__restrict__ out) {
    __shared__ double wave_max[kBlock / 64];
    double mx = 0.0;
    for (int i = threadIdx.x; i < nparts; i += kBlock) mx = part[i] > mx || part[i] != part[i] ? part[i] : mx;
    for (int step = 32; step >= 1; step >>= 1) {
        const double o = __shfl_xor(mx, step);
        mx = o > mx || o != o ? o : mx;
    }
    if ((threadIdx.x & 63) == 0) wave_max[threadIdx.x >> 6] = mx;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < kBlock / 64; ++w) mx = wave_max[w] > mx || wave_max[w] != wave_max[w] ? wave_max[w] : mx;
        out[0] = mx;
    }
}

}  // namespace spmv
