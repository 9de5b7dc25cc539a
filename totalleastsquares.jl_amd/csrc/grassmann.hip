// rpca_ga — "Grassmann averages" robust PCA and its spherical averages.
//
// Reference (paths relative to /root/reference):
//     rpca_ga                 src/robustPCA.jl:255-281     component loop: column norms, U = X ./ norms, deflation
//     rpca_ga_1               src/robustPCA.jl:286-310     sign-weighted average iteration for one component
//     μ!                      src/robustPCA.jl:312-320     weighted mean of the columns
//     entrywise_trimmed_mean  src/robustPCA.jl:327-337
//     entrywise_median        src/robustPCA.jl:354-362
//
// X is d x N, column-major: a column is one observation, so every step is a sweep over columns.  One iteration of
// rpca_ga_1 is    w_n = sign(U[:,n]'q) * norm_n ;  s = sum_n w_n U[:,n] ;  q = normalised(s / sum_n w_n)
// and needs each column exactly once: k_ga_pass holds a column in the registers of a lane group (G lanes, G = the
// power of two >= d up to 64, then RPL rows per lane), forms the dot with a DPP reduction inside the
// group and accumulates w * column in registers.  HBM traffic is one read of U per iteration (the unfused reference
// reads it twice: :294-296 and :315-318).  Sums are ordered: lane-group registers -> fixed-order LDS reduction per
// block -> per-block partial rows -> fixed-order sum (k_ga_reduce), so results are reproducible run to run.
//
// The convergence test (:299-304) runs on the device: k_ga_reduce's last block normalises, forms dq and sets a
// `converged` flag that turns the kernels of already queued iterations into no-ops; the host queues eight
// iterations at a time and reads the 40-byte state block in between.  Small problems (U fits in LDS) run whole in
// one workgroup, k_ga_solo, with no host round trip at all.
//
// The robust averages need order statistics of every row of U (trimmed mean: once per component, the ordering of
// U[j,:] does not depend on w; median: every iteration, ordering of w .* U[j,:]).  Not a sort: what the reference takes
// from `sortperm` is the element at one rank (median, :357) or the set of elements between two ranks (trimmed mean,
// :329-332), so every row runs a most-significant-digit radix SELECT on the composite key (value in `isless` order,
// column index) - distinct for every element, hence the ranks of a stable sort exactly: twelve histogram passes over
// the row-major transposed keys (eight value bytes, four index bytes), both ranks of a trimmed mean in the same passes.

#include "internal.hpp"

#pragma clang fp contract(off)

namespace tlsq {

namespace {

#ifndef TLSQ_GA_UNR1
#define TLSQ_GA_UNR1 8
#endif
constexpr int kGaFusedMaxD = 2048;   // longest column a lane group holds in registers (64 lanes x 32 rows)

struct GaState {
    double dq, nrm, ws;
    int32_t iters, converged;
    uint32_t counter, pad;
};

__device__ __forceinline__ double ga_sign(double x) { return x > 0.0 ? 1.0 : (x < 0.0 ? -1.0 : x); }   // Julia sign()

// Sum over each aligned group of G lanes without the LDS crossbar (__shfl_xor compiles to ds_bpermute_b32, six
// dependent LDS round trips per fp64 wave reduction): DPP steps inside a row of 16 lanes (quad_perm, quad_perm,
// row_half_mirror, row_mirror), then v_readlane of the row totals.  Every lane of the wave must be active.
template <int CTRL>
__device__ __forceinline__ double dpp_perm(double v) {
    int lo = __double2loint(v), hi = __double2hiint(v);
    lo = __builtin_amdgcn_update_dpp(lo, lo, CTRL, 0xF, 0xF, false);
    hi = __builtin_amdgcn_update_dpp(hi, hi, CTRL, 0xF, 0xF, false);
    return __hiloint2double(hi, lo);
}
__device__ __forceinline__ double read_lane(double v, int lane) {
    const int lo = __builtin_amdgcn_readlane(__double2loint(v), lane);
    const int hi = __builtin_amdgcn_readlane(__double2hiint(v), lane);
    return __hiloint2double(hi, lo);
}
template <int G>
__device__ __forceinline__ double group_sum(double v) {
    v += dpp_perm<0xB1>(v);                          // quad_perm [1,0,3,2]
    v += dpp_perm<0x4E>(v);                          // quad_perm [2,3,0,1]
    if constexpr (G >= 8) v += dpp_perm<0x141>(v);   // row_half_mirror
    if constexpr (G >= 16) v += dpp_perm<0x140>(v);  // row_mirror
    if constexpr (G == 32) {
        const double a = read_lane(v, 0) + read_lane(v, 16), b = read_lane(v, 32) + read_lane(v, 48);
        v = (threadIdx.x & 32) ? b : a;
    }
    if constexpr (G == 64) v = (read_lane(v, 0) + read_lane(v, 16)) + (read_lane(v, 32) + read_lane(v, 48));
    return v;
}

// deterministic sum over the threads of a block (a multiple of 64, at most 1024; every thread returns the total)
__device__ __forceinline__ double block_sum(double v, double* sh /* 16 doubles */) {
    v = group_sum<64>(v);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
    __syncthreads();
    double t = 0.0;
    const int nw = blockDim.x >> 6;
    for (int i = 0; i < nw; ++i) t += sh[i];
    return t;
}

// ---- component set-up: (deflate,) norms, normalise                                      (:263-266, :270-271) ----
// src (d x N, lds) -> Xw (d x N, ld d) = src - q (q' src)  [only when q != nullptr],  norms[n] = ||Xw[:,n]||,
// U[:,n] = Xw[:,n] / norms[n].  One lane group per column.
template <int G>
__global__ __launch_bounds__(256) void k_ga_prepare(const double* src /* may alias Xw */, int64_t lds, int d, int64_t N,
                                                    const double* __restrict__ q, double* Xw,
                                                    double* __restrict__ U, double* __restrict__ norms) {
    constexpr int GPW = 64 / G;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, g = lane / G, gl = lane % G;
    const int64_t gpb = 4 * GPW, stride = (int64_t)gridDim.x * gpb;
    for (int64_t n0 = (int64_t)blockIdx.x * gpb + wave * GPW; n0 < N; n0 += stride) {
        const int64_t n = n0 + g;
        const bool valid = n < N;
        const double* c = src + (valid ? n : 0) * lds;
        double t = 0.0;
        if (q) {
            for (int r = gl; r < d; r += G) {
                const double x = c[r];                              // (column 0 when n is out of range)
                t += (valid ? x : 0.0) * q[r];
            }
            t = group_sum<G>(t);                                   // Xs1[n] = q' X[:,n]     (:270)
        }
        double ss = 0.0;
        for (int r = gl; r < d; r += G) {
            const double x = c[r];
            double v = valid ? x : 0.0;
            if (q) v = v - q[r] * t;                               // X .-= q * Xs1          (:271)
            if (valid) Xw[n * d + r] = v;
            ss += v * v;
        }
        ss = group_sum<G>(ss);
        const double nrm = sqrt(ss);                               // :264
        if (valid) {
            if (gl == 0) norms[n] = nrm;
            for (int r = gl; r < d; r += G) U[n * d + r] = Xw[n * d + r] / nrm;   // :265
        }
    }
}

// the same with the column held in registers (d <= 64 * 32): one load, two stores per element
template <int G, int RPL>
__global__ __launch_bounds__(256) void k_ga_prepare_reg(const double* src /* may alias Xw */, int64_t lds, int d,
                                                        int64_t N, const double* __restrict__ q, double* Xw,
                                                        double* __restrict__ U, double* __restrict__ norms) {
    constexpr int GPW = 64 / G;
    constexpr int UNR = RPL <= 2 ? 4 : (RPL <= 8 ? 2 : 1);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, g = lane / G, gl = lane % G;
    double qreg[RPL];
    int rowc[RPL];
#pragma unroll
    for (int k = 0; k < RPL; ++k) {
        const int row = gl + k * G;
        rowc[k] = row < d ? row : d - 1;
        qreg[k] = (q && row < d) ? q[row] : 0.0;
    }
    const int64_t gpb = 4 * GPW, stride = (int64_t)gridDim.x * gpb;
    for (int64_t n0 = (int64_t)blockIdx.x * gpb + wave * GPW; n0 < N; n0 += stride * UNR) {
        double col[UNR][RPL];
#pragma unroll
        for (int c = 0; c < UNR; ++c) {
            const int64_t n = n0 + c * stride + g, nc = n < N ? n : N - 1;
#pragma unroll
            for (int k = 0; k < RPL; ++k) col[c][k] = src[nc * lds + rowc[k]];
        }
#pragma unroll
        for (int c = 0; c < UNR; ++c) {
            const int64_t n = n0 + c * stride + g;
            const bool valid = n < N;
#pragma unroll
            for (int k = 0; k < RPL; ++k) col[c][k] = (valid && gl + k * G < d) ? col[c][k] : 0.0;
            if (q) {
                double t = 0.0;
#pragma unroll
                for (int k = 0; k < RPL; ++k) t += col[c][k] * qreg[k];
                t = group_sum<G>(t);                                       // Xs1[n] = q' X[:,n]     (:270)
#pragma unroll
                for (int k = 0; k < RPL; ++k) col[c][k] = col[c][k] - qreg[k] * t;   // X .-= q * Xs1  (:271)
            }
            double ss = 0.0;
#pragma unroll
            for (int k = 0; k < RPL; ++k) ss += col[c][k] * col[c][k];
            ss = group_sum<G>(ss);
            const double nrm = sqrt(ss);                                   // :264
            if (valid) {
                if (gl == 0) norms[n] = nrm;
#pragma unroll
                for (int k = 0; k < RPL; ++k) {
                    const int row = gl + k * G;
                    if (row < d) {
                        Xw[n * d + row] = col[c][k];
                        U[n * d + row] = col[c][k] / nrm;                  // :265
                    }
                }
            }
        }
    }
}

// ---- the fused iteration sweep, d <= 64 * 32 ----------------------------------------------------------------
// partial row of a block: [0,d) weighted column sum; mean: [d] sum of weights; TRIM: [d,2d) per-row weight sums
template <int G, int RPL, bool TRIM>
__global__ __launch_bounds__(256) void k_ga_pass(const double* __restrict__ U, int d, int64_t N,
                                                 const double* __restrict__ norms, const double* __restrict__ w_in,
                                                 const double* __restrict__ q, const uint8_t* __restrict__ mask,
                                                 double* __restrict__ partial, int pstride,
                                                 const GaState* __restrict__ st) {
    if (st && st->converged) return;
    constexpr int GPW = 64 / G, DP = G * RPL;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, g = lane / G, gl = lane % G;
    double qreg[RPL], acc[RPL], accw[TRIM ? RPL : 1];
    int rowc[RPL];   // row index clamped into the column: loads are unconditional, out-of-range values are zeroed
#pragma unroll
    for (int k = 0; k < RPL; ++k) {
        const int row = gl + k * G;
        rowc[k] = row < d ? row : d - 1;
        qreg[k] = (!w_in && row < d) ? q[row] : 0.0;
        acc[k] = 0.0;
        if (TRIM) accw[k] = 0.0;
    }
    if (!TRIM) accw[0] = 0.0;
    // UNR columns per lane group are in flight at once (the loads of all of them are issued before the first dot)
    constexpr int UNR = RPL == 1 ? TLSQ_GA_UNR1 : (RPL == 2 ? 4 : (RPL <= 8 ? 2 : 1));
    const int64_t gpb = 4 * GPW, stride = (int64_t)gridDim.x * gpb;
    for (int64_t n0 = (int64_t)blockIdx.x * gpb + wave * GPW; n0 < N; n0 += stride * UNR) {
        double col[UNR][RPL], wn[UNR];   // wn: the column's norm (or its given weight), loaded with the column
        const double* __restrict__ wsrc = w_in ? w_in : norms;
#pragma unroll
        for (int c = 0; c < UNR; ++c) {
            const int64_t n = n0 + c * stride + g, nc = n < N ? n : N - 1;
#pragma unroll
            for (int k = 0; k < RPL; ++k) col[c][k] = U[nc * d + rowc[k]];
            wn[c] = wsrc[nc];
        }
#pragma unroll
        for (int c = 0; c < UNR; ++c) {
            const bool valid = n0 + c * stride + g < N;
#pragma unroll
            for (int k = 0; k < RPL; ++k) col[c][k] = (valid && gl + k * G < d) ? col[c][k] : 0.0;
        }
#pragma unroll
        for (int c = 0; c < UNR; ++c) {
            const int64_t n = n0 + c * stride + g;
            const bool valid = n < N;
            const int64_t nc = valid ? n : N - 1;
            double w = wn[c];
            if (!w_in) {
                double dot = 0.0;
#pragma unroll
                for (int k = 0; k < RPL; ++k) dot += col[c][k] * qreg[k];
                dot = group_sum<G>(dot);
                w = ga_sign(dot) * w;                                 // :295
            }
            w = valid ? w : 0.0;                                      // (an out-of-range column adds +0)
            if (!TRIM) {
#pragma unroll
                for (int k = 0; k < RPL; ++k) acc[k] += w * col[c][k];   // :317
                accw[0] += w;                                             // :316
            } else {
#pragma unroll
                for (int k = 0; k < RPL; ++k) {
                    const bool in = mask[nc * d + rowc[k]] != 0 && valid && gl + k * G < d;   // :332-333
                    acc[k] += in ? w * col[c][k] : 0.0;
                    accw[k] += in ? w : 0.0;
                }
            }
        }
    }
    // block reduction in a fixed order over the 4*GPW lane groups
    extern __shared__ double red[];   // [4*GPW][DP] (+ [4*GPW] weights)
    const int gi = wave * GPW + g;
    double* pb = partial + (size_t)blockIdx.x * pstride;
#pragma unroll
    for (int k = 0; k < RPL; ++k) red[gi * DP + gl + k * G] = acc[k];
    if (!TRIM && gl == 0) red[4 * GPW * DP + gi] = accw[0];
    __syncthreads();
    for (int row = threadIdx.x; row < d; row += 256) {
        double s = 0.0;
        for (int i = 0; i < 4 * GPW; ++i) s += red[i * DP + row];
        pb[row] = s;
    }
    if (!TRIM) {
        if (threadIdx.x == 0) {
            double s = 0.0;
            for (int i = 0; i < 4 * GPW; ++i) s += red[4 * GPW * DP + i];
            pb[d] = s;
        }
    } else {
        __syncthreads();
#pragma unroll
        for (int k = 0; k < RPL; ++k) red[gi * DP + gl + k * G] = accw[k];
        __syncthreads();
        for (int row = threadIdx.x; row < d; row += 256) {
            double s = 0.0;
            for (int i = 0; i < 4 * GPW; ++i) s += red[i * DP + row];
            pb[d + row] = s;
        }
    }
}

// ---- two-kernel form for long columns (d > 2048) and for the median keys ---------------------------------------
// w[n] = sign(U[:,n]'q) * norms[n]                                                               (:294-296)
__global__ __launch_bounds__(256) void k_ga_dots(const double* __restrict__ U, int d, int64_t N,
                                                 const double* __restrict__ norms, const double* __restrict__ q,
                                                 double* __restrict__ w, const GaState* __restrict__ st) {
    if (st && st->converged) return;
    const int lane = threadIdx.x & 63;
    const int64_t wid = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6), stride = (int64_t)gridDim.x * 4;
    for (int64_t n = wid; n < N; n += stride) {
        double dot = 0.0;
        for (int r = lane; r < d; r += 64) dot += U[n * d + r] * q[r];
        dot = group_sum<64>(dot);
        if (lane == 0) w[n] = ga_sign(dot) * norms[n];
    }
}

// thread per row, blockIdx.y = column chunk: partial[chunk] = sum over the chunk's columns
template <bool TRIM>
__global__ __launch_bounds__(256) void k_ga_wsum_rows(const double* __restrict__ U, int d, int64_t N,
                                                      const double* __restrict__ w, const uint8_t* __restrict__ mask,
                                                      double* __restrict__ partial, int pstride,
                                                      const GaState* __restrict__ st) {
    if (st && st->converged) return;
    const int row = blockIdx.x * 256 + threadIdx.x;
    const int64_t per = (N + gridDim.y - 1) / gridDim.y;
    const int64_t c0 = (int64_t)blockIdx.y * per, c1 = (c0 + per < N) ? c0 + per : N;
    double acc = 0.0, aw = 0.0;
    if (row < d) {
        for (int64_t n = c0; n < c1; ++n) {
            const double wn = w[n];
            if (!TRIM) {
                acc += wn * U[n * d + row];
                aw += wn;
            } else if (mask[n * d + row]) {
                acc += wn * U[n * d + row];
                aw += wn;
            }
        }
        double* pb = partial + (size_t)blockIdx.y * pstride;
        pb[row] = acc;
        if (TRIM) pb[d + row] = aw;
        else if (row == 0) pb[d] = aw;
    }
}

// ---- finish of an iteration: mu -> q, dq, convergence flag                                     (:297-304) ----
// mode 0: mu = s / ws (:319);  1: mu[j] = s[j] / sw[j] (:333);  2: mu = s (:359)
__device__ void ga_finalize(const double* __restrict__ sbuf, int d, int mode, double* __restrict__ q,
                            double* __restrict__ qold, double tol, GaState* st, double* __restrict__ dq_hist,
                            int hist_cap, double* sh) {
    const double ws = (mode == 0) ? sbuf[d] : 1.0;
    double n2 = 0.0;
    for (int r = threadIdx.x; r < d; r += blockDim.x) {
        const double m = (mode == 0) ? sbuf[r] / ws : (mode == 1 ? sbuf[r] / sbuf[d + r] : sbuf[r]);
        n2 += m * m;
    }
    n2 = block_sum(n2, sh);
    const double nrm = sqrt(n2);                                   // norm(μᵢ)   (:298)
    double d2 = 0.0;
    for (int r = threadIdx.x; r < d; r += blockDim.x) {
        const double m = (mode == 0) ? sbuf[r] / ws : (mode == 1 ? sbuf[r] / sbuf[d + r] : sbuf[r]);
        const double qn = m / nrm;
        const double df = qn - qold[r];
        d2 += df * df;
        q[r] = qn;
        qold[r] = qn;                                              // :305 (immaterial once converged)
    }
    d2 = block_sum(d2, sh);
    if (threadIdx.x == 0) {
        const double dq = sqrt(d2);                                // :299
        st->dq = dq;
        st->nrm = nrm;
        st->ws = ws;
        const int it = st->iters;
        if (dq_hist && it < hist_cap) dq_hist[it] = dq;
        st->iters = it + 1;
        st->converged = (dq < tol) ? 1 : 0;                        // :301
        st->counter = 0;
    }
}

// sbuf[row] = sum over the per-block partial rows in a fixed order: a block owns 64 rows, each of its 16 waves sums a
// contiguous sixteenth of the partial rows (8 independent chains), LDS combines the waves.  The last block to finish
// runs ga_finalize.
__global__ __launch_bounds__(1024) void k_ga_reduce(const double* __restrict__ partial, int nblk, int pstride, int ne,
                                                    int d, int mode, double* __restrict__ sbuf, int do_finalize,
                                                    double* __restrict__ q, double* __restrict__ qold, double tol,
                                                    GaState* st, double* __restrict__ dq_hist, int hist_cap) {
    __shared__ double part[16][64];
    __shared__ double sh[16];
    __shared__ int last;
    if (st->converged) return;
    const int lane = threadIdx.x & 63, seg = threadIdx.x >> 6;
    const int row = blockIdx.x * 64 + lane;
    const int per = (nblk + 15) / 16, b0 = seg * per, b1 = (b0 + per < nblk) ? b0 + per : nblk;
    double a[8] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    if (row < ne) {
        for (int b = b0; b < b1; b += 8) {
#pragma unroll
            for (int u = 0; u < 8; ++u)
                if (b + u < b1) a[u] += partial[(size_t)(b + u) * pstride + row];
        }
    }
    part[seg][lane] = ((a[0] + a[1]) + (a[2] + a[3])) + ((a[4] + a[5]) + (a[6] + a[7]));
    __syncthreads();
    if (seg == 0 && row < ne) {
        double t = 0.0;
#pragma unroll
        for (int i = 0; i < 16; ++i) t += part[i][lane];
        sbuf[row] = t;
    }
    if (!do_finalize) return;
    __threadfence();
    __syncthreads();
    if (threadIdx.x == 0) last = (atomicAdd(&st->counter, 1u) == gridDim.x - 1) ? 1 : 0;
    __syncthreads();
    if (!last) return;
    __threadfence();
    ga_finalize(sbuf, d, mode, q, qold, tol, st, dq_hist, hist_cap, sh);
}

__global__ __launch_bounds__(256) void k_ga_finalize(const double* __restrict__ sbuf, int d, int mode,
                                                     double* __restrict__ q, double* __restrict__ qold, double tol,
                                                     GaState* st, double* __restrict__ dq_hist, int hist_cap) {
    __shared__ double sh[16];
    if (st->converged) return;
    ga_finalize(sbuf, d, mode, q, qold, tol, st, dq_hist, hist_cap, sh);
}

// q = q0 / ||q0||, qold = q, state cleared                                                        (:289-291)
__global__ __launch_bounds__(256) void k_ga_start(const double* __restrict__ q0, int d, double* __restrict__ q,
                                                  double* __restrict__ qold, GaState* st) {
    __shared__ double sh[16];
    double n2 = 0.0;
    for (int r = threadIdx.x; r < d; r += 256) n2 += q0[r] * q0[r];
    n2 = block_sum(n2, sh);
    const double nrm = sqrt(n2);
    for (int r = threadIdx.x; r < d; r += 256) {
        const double v = q0[r] / nrm;
        q[r] = v;
        qold[r] = v;
    }
    if (threadIdx.x == 0) {
        st->dq = 0.0;
        st->nrm = nrm;
        st->ws = 0.0;
        st->iters = 0;
        st->converged = 0;
        st->counter = 0;
    }
}

// ---- order statistics of the rows ------------------------------------------------------------------------------
// keys[j*N + n] = (w ? w[n] : 1) * U[j, n]     (row-major transposed: a row is one selection segment)
__global__ __launch_bounds__(256) void k_ga_keys(const double* __restrict__ U, const double* __restrict__ w, int d,
                                                 int64_t N, double* __restrict__ keys, const GaState* __restrict__ st) {
    if (st && st->converged) return;
    const int64_t total = (int64_t)d * N, stride = (int64_t)gridDim.x * 256;
    for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < total; e += stride) {
        const int64_t j = e / N, n = e - j * N;
        const double u = U[n * d + j];
        keys[e] = w ? w[n] * u : u;                                // :356  (w) .* U[j,:]
    }
}

// value -> unsigned integer with the order of Julia's isless (-0.0 < 0.0, every NaN after +Inf and equal to each other)
__device__ __forceinline__ unsigned long long ga_sortable(double x) {
    unsigned long long u = (unsigned long long)__double_as_longlong(x);
    if (x != x) u = 0x7FF8000000000000ull;
    return (u >> 63) ? ~u : (u | 0x8000000000000000ull);
}

// selection state of one (row, target): the bytes of the composite key fixed so far and the rank still to be found among
// the elements that match them
struct GaSel {
    unsigned long long pkey;   // value bytes fixed so far (high bytes; the rest zero)
    unsigned long long k;      // rank among the candidates
    unsigned int pidx;         // index bytes fixed so far
    unsigned int pad;
};

// pass p = 0..7: byte 7 - p of the value; pass 8..11: byte 11 - p of the column index among the elements whose value
// equals the selected one.  hist[(row * NT + t) * 256 + digit] += 1 for every candidate of target t.
template <int NT>
__global__ __launch_bounds__(256) void k_ga_sel_hist(const double* __restrict__ keys, int64_t N, const GaSel* __restrict__ sel,
                                                     unsigned int* __restrict__ hist, int pass,
                                                     const GaState* __restrict__ st, unsigned int col_off) {
    if (st && st->converged) return;
    __shared__ unsigned int sh[NT * 256];
    const int row = blockIdx.y;
    for (int i = threadIdx.x; i < NT * 256; i += 256) sh[i] = 0;
    __syncthreads();
    GaSel my[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t) my[t] = sel[row * NT + t];
    const double* __restrict__ kr = keys + (int64_t)row * N;
    const int64_t stride = (int64_t)gridDim.x * 256;
    for (int64_t n = (int64_t)blockIdx.x * 256 + threadIdx.x; n < N; n += stride) {
        const unsigned long long u = ga_sortable(kr[n]);
#pragma unroll
        for (int t = 0; t < NT; ++t) {
            if (pass < 8) {
                const int sh_hi = 8 * (8 - pass);   // bits above the current byte
                const bool cand = pass == 0 || (u >> sh_hi) == (my[t].pkey >> sh_hi);
                if (cand) atomicAdd(&sh[t * 256 + (int)((u >> (8 * (7 - pass))) & 255ull)], 1u);
            } else if (u == my[t].pkey) {
                const unsigned int i32 = (unsigned int)n + col_off;   // (column shards: the index within the whole row)
                const int q = pass - 8, sh_hi = 8 * (4 - q);
                const bool cand = q == 0 || (i32 >> sh_hi) == (my[t].pidx >> sh_hi);
                if (cand) atomicAdd(&sh[t * 256 + (int)((i32 >> (8 * (3 - q))) & 255u)], 1u);
            }
        }
    }
    __syncthreads();
    for (int i = threadIdx.x; i < NT * 256; i += 256)
        if (sh[i]) atomicAdd(&hist[(size_t)row * NT * 256 + i], sh[i]);
}

// one workgroup per (row, target): the bin that holds rank k, fixed into the state; the histogram is cleared for the
// next pass
// (column shards: `tot` holds the histograms summed over the ranks - as doubles, exact below 2^53 - and `hist` only has to be
//  cleared)
__global__ __launch_bounds__(256) void k_ga_sel_pick(unsigned int* __restrict__ hist, GaSel* __restrict__ sel, int pass,
                                                     const GaState* __restrict__ st, const double* __restrict__ tot) {
    if (st && st->converged) return;
    __shared__ unsigned long long cum[256];
    const int rt = blockIdx.x, t = threadIdx.x;
    unsigned int* hh = hist + (size_t)rt * 256;
    const unsigned long long mine = tot ? (unsigned long long)tot[(size_t)rt * 256 + t] : (unsigned long long)hh[t];
    cum[t] = mine;
    __syncthreads();
    for (int off = 1; off < 256; off <<= 1) {   // inclusive scan
        const unsigned long long v = t >= off ? cum[t - off] : 0ull;
        __syncthreads();
        cum[t] += v;
        __syncthreads();
    }
    const unsigned long long k = sel[rt].k;
    const unsigned long long before = cum[t] - mine;
    if (mine > 0 && before <= k && k < cum[t]) {   // exactly one thread
        GaSel sn = sel[rt];
        sn.k = k - before;
        if (pass < 8) sn.pkey |= (unsigned long long)t << (8 * (7 - pass));
        else sn.pidx |= (unsigned int)t << (8 * (11 - pass));
        sel[rt] = sn;
    }
    hh[t] = 0;
}

__global__ __launch_bounds__(256) void k_ga_sel_init(GaSel* __restrict__ sel, int n, int nt, unsigned long long k0,
                                                     unsigned long long k1, const GaState* __restrict__ st) {
    if (st && st->converged) return;
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < n) {
        GaSel s0;
        s0.pkey = 0ull;
        s0.pidx = 0u;
        s0.pad = 0u;
        s0.k = (i % nt) == 0 ? k0 : k1;
        sel[i] = s0;
    }
}

// the local histograms as doubles for the sum all-reduce of a column-sharded selection
__global__ __launch_bounds__(256) void k_ga_hist_f64(const unsigned int* __restrict__ hist, double* __restrict__ out, int n) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < n) out[i] = (double)hist[i];
}

// mask[j + n*d] = 1 for the columns whose stable rank within row j lies in [lo, hi): composite (value, column) at or
// after the element of rank lo (sel[2j]) and before the element of rank hi (sel[2j+1]; no upper limit when hi == N)
__global__ __launch_bounds__(256) void k_ga_mask(const double* __restrict__ keys, const GaSel* __restrict__ sel, int d,
                                                 int64_t N, int has_hi, uint8_t* __restrict__ mask, unsigned int col_off) {
    const int64_t total = (int64_t)d * N, stride = (int64_t)gridDim.x * 256;
    for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < total; e += stride) {
        const int64_t j = e / N, n = e - j * N;
        const unsigned long long u = ga_sortable(keys[e]);
        const GaSel a = sel[2 * j], b = sel[2 * j + 1];
        const unsigned int ng = (unsigned int)n + col_off;
        const bool ge_lo = u > a.pkey || (u == a.pkey && ng >= a.pidx);
        const bool lt_hi = !has_hi || u < b.pkey || (u == b.pkey && ng < b.pidx);
        mask[n * d + j] = (ge_lo && lt_hi) ? 1 : 0;
    }
}
// s[j] = sign(w[m]) * U[j, m],  m = the column at sorted position N/2 (1-based) of row j            (:357-358)
// (column shards: the rank that owns column m delivers the value, the others zero - a sum all-reduce follows)
__global__ __launch_bounds__(256) void k_ga_pick(const GaSel* __restrict__ sel, const double* __restrict__ w,
                                                 const double* __restrict__ U, int d, int64_t N,
                                                 double* __restrict__ sbuf, const GaState* __restrict__ st,
                                                 unsigned int col_off) {
    if (st && st->converged) return;
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j < d) {
        const int64_t m = (int64_t)sel[j].pidx - (int64_t)col_off;
        sbuf[j] = (m >= 0 && m < N) ? ga_sign(w[m]) * U[m * d + j] : 0.0;
    }
}

// ---- small problems: the whole of rpca_ga in ONE workgroup ------------------------------------------------------
// The reference's own uses are small (10 x 40 ... 10 x 1000, test/runtests.jl:446-520): there a kernel launch and a
// host round trip per iteration cost more than the arithmetic.  When U and the norms fit in LDS (N (d+1) <= 18000
// doubles, d <= 64) one block of 512 threads runs every component and every iteration by itself: U lives in LDS,
// X (only needed for the deflation) stays in global memory, nothing returns to the host until all r components are
// done.  Same statements in the same order as the grid path (:263-271, :289-306, :312-320); the sums are again
// ordered (lane-group registers -> fixed-order LDS reduction), but partitioned differently from the grid path.
struct SoloOut {      // per component
    double dq;
    int32_t iters, status;
};
template <int G>
__global__ __launch_bounds__(512) void k_ga_solo(double* __restrict__ X, int d, int N, int r,
                                                 const double* __restrict__ q0, double tol, int iters,
                                                 double* __restrict__ Q, int64_t ldq, SoloOut* __restrict__ out,
                                                 double* __restrict__ hist, int hist_cap) {
    constexpr int GPW = 64 / G, NG = 8 * GPW;
    extern __shared__ double lds[];
    double* U = lds;                       // [N][d]
    double* nrm = U + (size_t)N * d;       // [N]
    double* red = nrm + N;                 // [NG][G]
    double* redw = red + NG * G;           // [NG]
    double* q = redw + NG;                 // [64]
    double* qold = q + 64;                 // [64]
    double* qprev = qold + 64;             // [64]
    double* sv = qprev + 64;               // [64] column sums
    double* sh = sv + 64;                  // [16] + [0]=ws at sh[16], flag at sh[17]
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, g = lane / G, gl = lane % G;
    const int gi = wave * GPW + g;
    const bool rowok = gl < d;
    const int glc = rowok ? gl : d - 1;
    const int ncol = (N + NG - 1) / NG;    // columns per lane group (the same trip count for every lane: DPP sums)
    for (int i = 0; i < r; ++i) {
        // ---- :263-266, and :270-271 of the previous component
        for (int c = 0; c < ncol; ++c) {
            const int n = gi + c * NG;
            const bool valid = n < N;
            const int nc = valid ? n : N - 1;
            double x = X[(size_t)nc * d + glc];
            x = (valid && rowok) ? x : 0.0;
            if (i > 0) {
                const double qp = rowok ? qprev[gl] : 0.0;
                const double t = group_sum<G>(x * qp);
                x = x - qp * t;
                if (valid && rowok) X[(size_t)n * d + gl] = x;
            }
            const double nn = sqrt(group_sum<G>(x * x));
            if (valid) {
                if (gl == 0) nrm[n] = nn;
                if (rowok) U[(size_t)n * d + gl] = x / nn;
            }
        }
        // ---- :289-291
        {
            const double v = (threadIdx.x < d) ? q0[(size_t)i * d + threadIdx.x] : 0.0;
            const double n2 = block_sum(v * v, sh);
            if (threadIdx.x < d) {
                const double qn = v / sqrt(n2);
                q[threadIdx.x] = qn;
                qold[threadIdx.x] = qn;
            }
        }
        __syncthreads();
        int it = 0, conv = 0;
        double dq = 0.0;
        while (it < iters) {
            const double qr = rowok ? q[gl] : 0.0;
            double acc = 0.0, wsum = 0.0;
            for (int c = 0; c < ncol; ++c) {
                const int n = gi + c * NG;
                const bool valid = n < N;
                const int nc = valid ? n : N - 1;
                double u = U[(size_t)nc * d + glc];
                u = (valid && rowok) ? u : 0.0;
                const double dot = group_sum<G>(u * qr);
                double w = ga_sign(dot) * nrm[nc];                 // :295
                w = valid ? w : 0.0;
                acc += w * u;                                      // :317
                wsum += w;                                         // :316
            }
            red[gi * G + gl] = acc;
            if (gl == 0) redw[gi] = wsum;
            __syncthreads();
            if (threadIdx.x < d) {
                double t = 0.0;
                for (int k = 0; k < NG; ++k) t += red[k * G + threadIdx.x];
                sv[threadIdx.x] = t;
            } else if (threadIdx.x == 64) {
                double t = 0.0;
                for (int k = 0; k < NG; ++k) t += redw[k];
                sh[16] = t;
            }
            __syncthreads();
            if (wave == 0) {                                       // :319, :298-301 on one wave
                const double ws = sh[16];
                const double m = (lane < d) ? sv[lane] / ws : 0.0;
                const double n2 = group_sum<64>(m * m);
                const double qn = (lane < d) ? m / sqrt(n2) : 0.0;
                const double df = (lane < d) ? qn - qold[lane] : 0.0;
                const double d2 = group_sum<64>(df * df);
                if (lane < d) {
                    q[lane] = qn;
                    qold[lane] = qn;
                }
                if (lane == 0) {
                    const double v = sqrt(d2);
                    sh[17] = v;
                    if (hist && it < hist_cap) hist[(size_t)i * hist_cap + it] = v;
                }
            }
            __syncthreads();
            dq = sh[17];
            ++it;
            if (dq < tol) {                                        // :301
                conv = 1;
                break;
            }
        }
        if (threadIdx.x < d) {
            Q[(size_t)i * ldq + threadIdx.x] = q[threadIdx.x];    // :268
            qprev[threadIdx.x] = q[threadIdx.x];
        }
        if (threadIdx.x == 0) {
            out[i].dq = dq;
            out[i].iters = it;
            out[i].status = conv ? 0 : 1;
        }
        __syncthreads();
    }
}

// ---- launch helpers --------------------------------------------------------------------------------------------

inline int group_lanes(int64_t d) { return d <= 4 ? 4 : d <= 8 ? 8 : d <= 16 ? 16 : d <= 32 ? 32 : 64; }
inline int rows_per_lane(int64_t d) {
    const int64_t need = (d + 63) / 64;
    int r = 1;
    while (r < need) r *= 2;
    return r;
}
inline int pass_blocks(int64_t N, int64_t d) {
    const int G = group_lanes(d);
    const int64_t gpb = 4 * (64 / G);
    int64_t nb = (N + gpb * 8 - 1) / (gpb * 8);   // >= 8 columns per lane group
    // two blocks per CU: measured best for every column length (256 / 1024 / 2048 / 4096 blocks are slower) — each
    // block costs a partial row in k_ga_reduce, and the columns in flight per lane group already cover the latency
    if (nb < 1) nb = 1;
    if (nb > 512) nb = 512;
    return (int)nb;
}

template <int G>
int prepare_g(Handle* h, const double* src, int64_t lds, int64_t d, int64_t N, const double* q, double* Xw, double* U,
              double* norms) {
    const int64_t gpb = 4 * (64 / G);
    int64_t nb = (N + gpb - 1) / gpb;
    if (nb > 8192) nb = 8192;
    hipLaunchKernelGGL(k_ga_prepare<G>, dim3((int)nb), dim3(256), 0, h->stream, src, lds, (int)d, N, q, Xw, U, norms);
    TLSQ_HIP(h, hipGetLastError());
    return TLSQ_OK;
}
template <int G, int RPL>
int prepare_reg(Handle* h, const double* src, int64_t lds, int64_t d, int64_t N, const double* q, double* Xw, double* U,
                double* norms) {
    const int64_t gpb = 4 * (64 / G);
    int64_t nb = (N + gpb * 2 - 1) / (gpb * 2);
    const int64_t cap = RPL <= 8 ? 2048 : 512;
    if (nb < 1) nb = 1;
    if (nb > cap) nb = cap;
    hipLaunchKernelGGL((k_ga_prepare_reg<G, RPL>), dim3((int)nb), dim3(256), 0, h->stream, src, lds, (int)d, N, q, Xw, U,
                       norms);
    TLSQ_HIP(h, hipGetLastError());
    return TLSQ_OK;
}
int launch_prepare(Handle* h, const double* src, int64_t lds, int64_t d, int64_t N, const double* q, double* Xw,
                   double* U, double* norms) {
    if (d > kGaFusedMaxD) return prepare_g<64>(h, src, lds, d, N, q, Xw, U, norms);
    switch (group_lanes(d)) {
        case 4: return prepare_reg<4, 1>(h, src, lds, d, N, q, Xw, U, norms);
        case 8: return prepare_reg<8, 1>(h, src, lds, d, N, q, Xw, U, norms);
        case 16: return prepare_reg<16, 1>(h, src, lds, d, N, q, Xw, U, norms);
        case 32: return prepare_reg<32, 1>(h, src, lds, d, N, q, Xw, U, norms);
        default: break;
    }
    switch (rows_per_lane(d)) {
        case 1: return prepare_reg<64, 1>(h, src, lds, d, N, q, Xw, U, norms);
        case 2: return prepare_reg<64, 2>(h, src, lds, d, N, q, Xw, U, norms);
        case 4: return prepare_reg<64, 4>(h, src, lds, d, N, q, Xw, U, norms);
        case 8: return prepare_reg<64, 8>(h, src, lds, d, N, q, Xw, U, norms);
        case 16: return prepare_reg<64, 16>(h, src, lds, d, N, q, Xw, U, norms);
        default: return prepare_reg<64, 32>(h, src, lds, d, N, q, Xw, U, norms);
    }
}

struct PassArgs {
    const double* U;
    int64_t d, N;
    const double* norms;
    const double* w_in;
    const double* q;
    const uint8_t* mask;   // non-null = trimmed mean
    double* partial;
    int pstride;
    const GaState* st;
};

template <int G, int RPL>
int pass_gr(Handle* h, const PassArgs& a, int nblk) {
    const size_t lds = (size_t)(4 * (64 / G)) * (G * RPL + 1) * 8;
    if (a.mask)
        hipLaunchKernelGGL((k_ga_pass<G, RPL, true>), dim3(nblk), dim3(256), lds, h->stream, a.U, (int)a.d, a.N, a.norms,
                           a.w_in, a.q, a.mask, a.partial, a.pstride, a.st);
    else
        hipLaunchKernelGGL((k_ga_pass<G, RPL, false>), dim3(nblk), dim3(256), lds, h->stream, a.U, (int)a.d, a.N,
                           a.norms, a.w_in, a.q, a.mask, a.partial, a.pstride, a.st);
    TLSQ_HIP(h, hipGetLastError());
    return TLSQ_OK;
}
int launch_pass(Handle* h, const PassArgs& a, int nblk) {
    const int G = group_lanes(a.d);
    if (G < 64) {
        switch (G) {
            case 4: return pass_gr<4, 1>(h, a, nblk);
            case 8: return pass_gr<8, 1>(h, a, nblk);
            case 16: return pass_gr<16, 1>(h, a, nblk);
            default: return pass_gr<32, 1>(h, a, nblk);
        }
    }
    switch (rows_per_lane(a.d)) {
        case 1: return pass_gr<64, 1>(h, a, nblk);
        case 2: return pass_gr<64, 2>(h, a, nblk);
        case 4: return pass_gr<64, 4>(h, a, nblk);
        case 8: return pass_gr<64, 8>(h, a, nblk);
        case 16: return pass_gr<64, 16>(h, a, nblk);
        default: return pass_gr<64, 32>(h, a, nblk);
    }
}

// device buffers of one rpca_ga / average call
struct GaBuffers {
    double *Xw = nullptr, *U = nullptr;
    double *norms = nullptr, *w = nullptr, *q = nullptr, *qold = nullptr, *sbuf = nullptr, *q0 = nullptr, *hist = nullptr;
    GaState* st = nullptr;
    double* partial = nullptr;
    int pstride = 0, nblk = 0;
    uint8_t* mask = nullptr;
    double* keys_in = nullptr;
    GaSel* sel = nullptr;            // selection state, d x (1 or 2) targets
    unsigned int* sel_hist = nullptr;   // d x targets x 256 counters (kept zero between passes)
    // column shards (a communicator on the handle): this rank holds the columns [col_off, col_off + N) of N_glob
    int64_t col_off = 0, N_glob = 0;
    double* hist_f64 = nullptr;      // the histograms as doubles for the all-reduce of a sharded selection
};

inline size_t align256(size_t b) { return (b + 255) & ~(size_t)255; }

int ga_alloc(Handle* h, int64_t d, int64_t N, int mode, int64_t hist_cap, bool need_x, GaBuffers* b) {
    void* p;
    const size_t pn = (size_t)d * N * 8;
    if (need_x) {
        TLSQ_TRY(ws_get(h, WS_GA_X, pn, &p));
        b->Xw = (double*)p;
    }
    TLSQ_TRY(ws_get(h, WS_GA_U, pn, &p));
    b->U = (double*)p;
    // small block: norms | w | q | qold | q0 | sbuf (2d+2) | state | hist
    const size_t oN = 0, oW = oN + align256((size_t)N * 8), oQ = oW + align256((size_t)N * 8),
                 oQo = oQ + align256((size_t)d * 8), oQ0 = oQo + align256((size_t)d * 8),
                 oS = oQ0 + align256((size_t)d * 8), oSt = oS + align256((size_t)(2 * d + 2) * 8),
                 oH = oSt + 256, oEnd = oH + align256((size_t)(hist_cap > 0 ? hist_cap : 1) * 8);
    TLSQ_TRY(ws_get(h, WS_GA_AUX, oEnd, &p));
    char* c = (char*)p;
    b->norms = (double*)(c + oN);
    b->w = (double*)(c + oW);
    b->q = (double*)(c + oQ);
    b->qold = (double*)(c + oQo);
    b->q0 = (double*)(c + oQ0);
    b->sbuf = (double*)(c + oS);
    b->st = (GaState*)(c + oSt);
    b->hist = (double*)(c + oH);
    b->pstride = (int)(2 * d + 2);
    if (d <= kGaFusedMaxD) {
        b->nblk = pass_blocks(N, d);
    } else {
        int64_t nc = (N + 255) / 256;   // >= 256 columns per chunk
        if (nc < 1) nc = 1;
        if (nc > 256) nc = 256;
        b->nblk = (int)nc;
    }
    TLSQ_TRY(ws_get(h, WS_GA_PART, (size_t)b->nblk * b->pstride * 8, &p));
    b->partial = (double*)p;
    if (mode != TLSQ_GA_MEAN) {
        if (N >= (int64_t)1 << 32)
            return set_err(h, TLSQ_ERR_UNSUPPORTED, "rpca_ga: the entrywise averages need N < 2^32 columns");
        if (mode == TLSQ_GA_TRIMMED_MEAN) {
            TLSQ_TRY(ws_get(h, WS_GA_MASK, (size_t)d * N, &p));
            b->mask = (uint8_t*)p;
        }
        TLSQ_TRY(ws_get(h, WS_GA_KEYS, pn, &p));
        b->keys_in = (double*)p;
        const size_t sb = align256((size_t)d * 2 * sizeof(GaSel));
        const size_t hb = (size_t)d * 2 * 256 * 4;
        TLSQ_TRY(ws_get(h, WS_GA_IDX, sb + hb + (h->comm ? 2 * hb : 0), &p));
        b->sel = (GaSel*)p;
        b->sel_hist = (unsigned int*)((char*)p + sb);
        if (h->comm) b->hist_f64 = (double*)((char*)p + sb + hb);
        TLSQ_HIP(h, hipMemsetAsync(b->sel_hist, 0, (size_t)d * 2 * 256 * 4, h->stream));
    }
    return TLSQ_OK;
}

// The elements of stable rank r0 (and r1 when nt == 2) of every row of the key matrix, as composite keys in b->sel:
// twelve histogram + pick passes (see the head of the file).  Ranks are 0-based and < N.
int ga_select_rows(Handle* h, GaBuffers* b, int64_t d, int64_t N, int nt, int64_t r0, int64_t r1, const GaState* st) {
    hipLaunchKernelGGL(k_ga_sel_init, dim3((int)((d * nt + 255) / 256)), dim3(256), 0, h->stream, b->sel, (int)(d * nt), nt,
                       (unsigned long long)r0, (unsigned long long)r1, st);
    int64_t gx = (N + 256 * 16 - 1) / (256 * 16);   // >= 16 elements per thread
    if (gx < 1) gx = 1;
    const int64_t cap = std::max<int64_t>(1, 4096 / std::max<int64_t>(d, 1));
    if (gx > cap) gx = cap;                           // ~4096 workgroups over all rows
    // Column shards: the composite key carries the column index within the WHOLE row, every rank histograms its own
    // columns, the histograms are summed over the ranks (d x nt x 256 counts per pass) and every rank picks the same digit:
    // the selected element is the one the stable sortperm of the whole row would put at that rank.
    const unsigned int off = (unsigned int)b->col_off;
    const int nh = (int)(d * nt * 256);
    for (int pass = 0; pass < 12; ++pass) {
        if (nt == 2)
            hipLaunchKernelGGL(k_ga_sel_hist<2>, dim3((unsigned)gx, (unsigned)d), dim3(256), 0, h->stream, b->keys_in, N, b->sel,
                               b->sel_hist, pass, st, off);
        else
            hipLaunchKernelGGL(k_ga_sel_hist<1>, dim3((unsigned)gx, (unsigned)d), dim3(256), 0, h->stream, b->keys_in, N, b->sel,
                               b->sel_hist, pass, st, off);
        const double* tot = nullptr;
        if (h->comm) {
            hipLaunchKernelGGL(k_ga_hist_f64, dim3((unsigned)((nh + 255) / 256)), dim3(256), 0, h->stream, b->sel_hist,
                               b->hist_f64, nh);
            TLSQ_HIP(h, hipGetLastError());
            TLSQ_TRY(comm_allreduce(h, b->hist_f64, (size_t)nh, ncclSum));
            tot = b->hist_f64;
        }
        hipLaunchKernelGGL(k_ga_sel_pick, dim3((unsigned)(d * nt)), dim3(256), 0, h->stream, b->sel_hist, b->sel, pass, st, tot);
    }
    TLSQ_HIP(h, hipGetLastError());
    return TLSQ_OK;
}

int ga_keys(Handle* h, GaBuffers* b, const double* w, int64_t d, int64_t N, const GaState* st) {
    int64_t g = ((int64_t)d * N + 255) / 256;
    if (g > 8192) g = 8192;
    hipLaunchKernelGGL(k_ga_keys, dim3((int)g), dim3(256), 0, h->stream, b->U, w, (int)d, N, b->keys_in, st);
    TLSQ_HIP(h, hipGetLastError());
    return TLSQ_OK;
}

// trimmed mean: mark the entries of U whose rank inside their row lies in `range` (:329); U is fixed per component
int ga_build_mask(Handle* h, GaBuffers* b, int64_t d, int64_t N, double P) {
    const int64_t Ng = b->N_glob > 0 ? b->N_glob : N;   // (the ranks of :329 are ranks within the whole row)
    const int64_t lo = (int64_t)std::floor(P * (double)Ng), hi = (int64_t)std::floor((1.0 - P) * (double)Ng);
    if (hi <= lo) {
        TLSQ_HIP(h, hipMemsetAsync(b->mask, 0, (size_t)d * N, h->stream));
        return TLSQ_OK;
    }
    TLSQ_TRY(ga_keys(h, b, nullptr, d, N, nullptr));
    const int has_hi = hi < Ng ? 1 : 0;
    TLSQ_TRY(ga_select_rows(h, b, d, N, 2, lo, has_hi ? hi : lo, nullptr));
    int64_t g = (d * N + 255) / 256;
    if (g > 8192) g = 8192;
    hipLaunchKernelGGL(k_ga_mask, dim3((int)g), dim3(256), 0, h->stream, (const double*)b->keys_in, (const GaSel*)b->sel, (int)d,
                       N, has_hi, b->mask, (unsigned int)b->col_off);
    TLSQ_HIP(h, hipGetLastError());
    return TLSQ_OK;
}

// the weighted sums of one iteration into b->sbuf (no finish): w from q (w_in == nullptr) or given
int ga_sums(Handle* h, GaBuffers* b, int64_t d, int64_t N, int mode, const double* w_in, const GaState* st) {
    if (mode == TLSQ_GA_MEDIAN) {
        const double* w = w_in;
        if (!w) {
            int64_t g = (N + 3) / 4;
            if (g > 4096) g = 4096;
            hipLaunchKernelGGL(k_ga_dots, dim3((int)g), dim3(256), 0, h->stream, b->U, (int)d, N, b->norms, b->q, b->w, st);
            TLSQ_HIP(h, hipGetLastError());
            w = b->w;
        }
        TLSQ_TRY(ga_keys(h, b, w, d, N, st));
        const int64_t Ng = b->N_glob > 0 ? b->N_glob : N;
        TLSQ_TRY(ga_select_rows(h, b, d, N, 1, Ng / 2 - 1, 0, st));
        hipLaunchKernelGGL(k_ga_pick, dim3((int)((d + 255) / 256)), dim3(256), 0, h->stream, (const GaSel*)b->sel, w, b->U,
                           (int)d, N, b->sbuf, st, (unsigned int)b->col_off);
        TLSQ_HIP(h, hipGetLastError());
        if (h->comm) TLSQ_TRY(comm_allreduce(h, b->sbuf, (size_t)d, ncclSum));
        return TLSQ_OK;
    }
    const uint8_t* mask = (mode == TLSQ_GA_TRIMMED_MEAN) ? b->mask : nullptr;
    if (d <= kGaFusedMaxD) {
        PassArgs a{b->U, d, N, b->norms, w_in, b->q, mask, b->partial, b->pstride, st};
        TLSQ_TRY(launch_pass(h, a, b->nblk));
    } else {
        const double* w = w_in;
        if (!w) {
            int64_t g = (N + 3) / 4;
            if (g > 4096) g = 4096;
            hipLaunchKernelGGL(k_ga_dots, dim3((int)g), dim3(256), 0, h->stream, b->U, (int)d, N, b->norms, b->q, b->w, st);
            TLSQ_HIP(h, hipGetLastError());
            w = b->w;
        }
        const dim3 grid((unsigned)((d + 255) / 256), (unsigned)b->nblk);
        if (mask)
            hipLaunchKernelGGL(k_ga_wsum_rows<true>, grid, dim3(256), 0, h->stream, b->U, (int)d, N, w, mask, b->partial,
                               b->pstride, st);
        else
            hipLaunchKernelGGL(k_ga_wsum_rows<false>, grid, dim3(256), 0, h->stream, b->U, (int)d, N, w, mask, b->partial,
                               b->pstride, st);
        TLSQ_HIP(h, hipGetLastError());
    }
    return TLSQ_OK;
}

inline int ga_entries(int64_t d, int mode) { return mode == TLSQ_GA_TRIMMED_MEAN ? (int)(2 * d) : (int)(d + 1); }

// one queued iteration of rpca_ga_1: sums, (all-reduce,) finish
int ga_iteration(Handle* h, GaBuffers* b, int64_t d, int64_t N, int mode, double tol, int hist_cap) {
    TLSQ_TRY(ga_sums(h, b, d, N, mode, nullptr, b->st));
    const bool sharded = h->comm != nullptr;
    if (mode == TLSQ_GA_MEDIAN) {
        hipLaunchKernelGGL(k_ga_finalize, dim3(1), dim3(256), 0, h->stream, b->sbuf, (int)d, 2, b->q, b->qold, tol, b->st,
                           b->hist, hist_cap);
        TLSQ_HIP(h, hipGetLastError());
        return TLSQ_OK;
    }
    const int ne = ga_entries(d, mode), fmode = (mode == TLSQ_GA_TRIMMED_MEAN) ? 1 : 0;
    hipLaunchKernelGGL(k_ga_reduce, dim3((ne + 63) / 64), dim3(1024), 0, h->stream, b->partial, b->nblk, b->pstride, ne,
                       (int)d, fmode, b->sbuf, sharded ? 0 : 1, b->q, b->qold, tol, b->st, b->hist, hist_cap);
    TLSQ_HIP(h, hipGetLastError());
    if (sharded) {
        // column shards: the weighted sums add up over the ranks; q and the flag then evolve identically everywhere
        TLSQ_TRY(comm_allreduce(h, b->sbuf, (size_t)ne, ncclSum));
        hipLaunchKernelGGL(k_ga_finalize, dim3(1), dim3(256), 0, h->stream, b->sbuf, (int)d, fmode, b->q, b->qold, tol,
                           b->st, b->hist, hist_cap);
        TLSQ_HIP(h, hipGetLastError());
    }
    return TLSQ_OK;
}

int read_state(Handle* h, const GaState* dev, GaState* host) {
    TLSQ_HIP(h, hipMemcpyAsync(h->pinned, dev, sizeof(GaState), hipMemcpyDeviceToHost, h->stream));
    TLSQ_HIP(h, hipStreamSynchronize(h->stream));
    memcpy(host, h->pinned, sizeof(GaState));
    return TLSQ_OK;
}

}  // namespace

}  // namespace tlsq


using namespace tlsq;

// the single-workgroup path for small problems (k_ga_solo)
static size_t solo_lds_bytes(int64_t d, int64_t N, int G) {
    const int NG = 8 * (64 / G);
    return ((size_t)N * d + N + (size_t)NG * G + NG + 4 * 64 + 18) * 8;
}
static int run_solo(Handle* h, const double* X, int64_t d, int64_t N, int64_t ldX, int64_t r, bool dev, double tol,
                    int64_t iters, const double* dq0, double* dQ, int64_t ldq, tlsq_ga_info* info, int hist_cap,
                    int64_t* passes, int* rc) {
    const int G = group_lanes(d);
    const size_t lds = solo_lds_bytes(d, N, G);
    void* p;
    TLSQ_TRY(ws_get(h, WS_GA_X, (size_t)d * N * 8, &p));
    double* Xw = (double*)p;
    TLSQ_TRY(copy2d(h, Xw, d, X, ldX, d, N, 8, dev ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice));   // :257
    const size_t ob = (size_t)r * sizeof(SoloOut), hb = (size_t)r * (hist_cap > 0 ? hist_cap : 0) * 8;
    TLSQ_TRY(ws_get(h, WS_GA_AUX, ob + hb + 256, &p));
    SoloOut* out = (SoloOut*)p;
    double* hist = hb ? (double*)((char*)p + ((ob + 255) & ~(size_t)255)) : nullptr;
    if (hb) TLSQ_HIP(h, hipMemsetAsync(hist, 0xff, hb, h->stream));   // NaN fill
#define SOLO_LAUNCH(GG)                                                                                              \
    do {                                                                                                             \
        TLSQ_HIP(h, hipFuncSetAttribute(reinterpret_cast<const void*>(k_ga_solo<GG>),                                \
                                        hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));                      \
        hipLaunchKernelGGL(k_ga_solo<GG>, dim3(1), dim3(512), lds, h->stream, Xw, (int)d, (int)N, (int)r, dq0, tol,   \
                           (int)std::min<int64_t>(iters, 1 << 30), dQ, ldq, out, hist, hist_cap);                    \
    } while (0)
    switch (G) {
        case 4: SOLO_LAUNCH(4); break;
        case 8: SOLO_LAUNCH(8); break;
        case 16: SOLO_LAUNCH(16); break;
        case 32: SOLO_LAUNCH(32); break;
        default: SOLO_LAUNCH(64); break;
    }
#undef SOLO_LAUNCH
    TLSQ_HIP(h, hipGetLastError());
    std::vector<SoloOut> ho((size_t)r);
    std::vector<double> hh(hb / 8);
    TLSQ_HIP(h, hipMemcpyAsync(ho.data(), out, ob, hipMemcpyDeviceToHost, h->stream));
    if (hb) TLSQ_HIP(h, hipMemcpyAsync(hh.data(), hist, hb, hipMemcpyDeviceToHost, h->stream));
    TLSQ_HIP(h, hipStreamSynchronize(h->stream));
    for (int64_t i = 0; i < r; ++i) {
        *passes += ho[(size_t)i].iters;
        if (ho[(size_t)i].status) *rc = TLSQ_MAXITER;
        if (!info) continue;
        if (info->iters) info->iters[i] = ho[(size_t)i].iters;
        if (info->status) info->status[i] = ho[(size_t)i].status;
        if (info->dq) info->dq[i] = ho[(size_t)i].dq;
        if (hist_cap > 0) {
            memcpy(info->dq_hist + (size_t)i * info->hist_capacity, hh.data() + (size_t)i * hist_cap, (size_t)hist_cap * 8);
            for (int64_t k = hist_cap; k < info->hist_capacity; ++k)
                info->dq_hist[(size_t)i * info->hist_capacity + k] = std::numeric_limits<double>::quiet_NaN();
        }
    }
    return TLSQ_OK;
}

extern "C" {

void tlsq_ga_opts_default(tlsq_ga_opts* o) {
    if (!o) return;
    memset(o, 0, sizeof(*o));
    o->tol = std::numeric_limits<double>::quiet_NaN();
    o->iters = 0;
    o->average = TLSQ_GA_MEAN;
    o->memory = TLSQ_MEM_HOST;
    o->trim = std::numeric_limits<double>::quiet_NaN();
    o->seed = 0;
}

int tlsq_rpca_ga_f64(tlsq_handle h, const double* X, int64_t d, int64_t N, int64_t ldX, int64_t r,
                     const tlsq_ga_opts* opts, const double* q0, int64_t ldq0, double* Q, int64_t ldQ,
                     tlsq_ga_info* info) {
    TLSQ_TRY(check_handle(h));
    if (is_multi_call(h) && X && Q && d > 0 && r > 0 && ldX >= d && ldQ >= d && N >= 64 * (int64_t)h->multi_n &&
        !(opts && opts->memory == TLSQ_MEM_DEVICE) && !(opts && opts->average == TLSQ_GA_CALLBACK)) {
        // single-process multi-GPU group: contiguous blocks of the observations (columns of the host matrix) per
        // rank, the same start vectors everywhere; q and every decision evolve identically on all ranks, rank 0 delivers Q and
        // the report.  (Fewer than 64 columns per GPU, device pointers: the first GPU alone, below.)
        const int nr = h->multi_n;
        std::vector<std::vector<double>> qs((size_t)nr);
        std::vector<tlsq_ga_opts> ro((size_t)nr);
        std::vector<double> q0s;
        if (!q0) {   // (the library's own normals are drawn per handle: draw them once, on the host side of rank 0's stream)
            q0s.resize((size_t)d * r);
            TLSQ_HIP(h, hipSetDevice(h->device));
            void* p;
            TLSQ_TRY(ws_get(h, WS_GA_Q, (size_t)d * r * 8 * 2, &p));
            const uint64_t seed = opts ? opts->seed : 0;
            TLSQ_TRY(launch_fill_gauss(h, (double*)p, d * r, (unsigned int)(seed * 2654435761ull + 0x6a09e667u)));
            TLSQ_HIP(h, hipMemcpyAsync(q0s.data(), p, (size_t)d * r * 8, hipMemcpyDeviceToHost, h->stream));
            TLSQ_HIP(h, hipStreamSynchronize(h->stream));
        }
        const double* q0u = q0 ? q0 : q0s.data();
        const int64_t ldq0u = q0 ? ldq0 : d;
        for (int k = 0; k < nr; ++k) {
            if (opts) ro[(size_t)k] = *opts; else tlsq_ga_opts_default(&ro[(size_t)k]);
            ro[(size_t)k].memory = TLSQ_MEM_HOST;
            if (k > 0) qs[(size_t)k].resize((size_t)d * r);
        }
        const int64_t base = N / nr, rem = N % nr;
        return multi_run(h, [&](Handle* hr, int k, int) -> int {
            const int64_t c0 = k * base + std::min<int64_t>(k, rem), nc = base + (k < rem ? 1 : 0);
            return tlsq_rpca_ga_f64(static_cast<tlsq_handle>(hr), X + (size_t)c0 * ldX, d, nc, ldX, r, &ro[(size_t)k], q0u, ldq0u,
                                    k == 0 ? Q : qs[(size_t)k].data(), k == 0 ? ldQ : d, k == 0 ? info : nullptr);
        });
    }
    if (!X || !Q || d <= 0 || N <= 0 || ldX < d || ldQ < d || r < 0 || (q0 && ldq0 < d))
        return set_err(h, TLSQ_ERR_ARG, "rpca_ga: bad argument");
    if (d > (int64_t)1 << 30) return set_err(h, TLSQ_ERR_UNSUPPORTED, "rpca_ga: d too large");
    const double tol = (opts && opts->tol == opts->tol) ? opts->tol : 1e-7;            // :286
    const int64_t iters = (opts && opts->iters > 0) ? opts->iters : 1000;              // :286
    const int mode = opts ? opts->average : TLSQ_GA_MEAN;
    const double P = (opts && opts->trim == opts->trim) ? opts->trim : 0.1;           // :327
    const bool dev = opts && opts->memory == TLSQ_MEM_DEVICE;
    const uint64_t seed = opts ? opts->seed : 0;
    const bool cb_mode = mode == TLSQ_GA_CALLBACK;
    if (cb_mode && !(opts && opts->avg_cb)) return set_err(h, TLSQ_ERR_ARG, "rpca_ga: TLSQ_GA_CALLBACK without a callback");
    if (cb_mode && h->comm)
        return set_err(h, TLSQ_ERR_UNSUPPORTED, "rpca_ga: a caller's average needs all observations on one GPU (not column shards)");
    if (mode != TLSQ_GA_MEAN && mode != TLSQ_GA_TRIMMED_MEAN && mode != TLSQ_GA_MEDIAN && !cb_mode)
        return set_err(h, TLSQ_ERR_ARG, "rpca_ga: unknown average %d", mode);
    if (mode == TLSQ_GA_MEDIAN && N < 2)
        return set_err(h, TLSQ_ERR_ARG, "rpca_ga: entrywise_median needs at least 2 columns (I[end÷2])");
    if (mode == TLSQ_GA_TRIMMED_MEAN && !(P >= 0.0 && P < 1.0))
        return set_err(h, TLSQ_ERR_ARG, "rpca_ga: trim fraction outside [0,1)");
    if (info) {
        info->ms_total = info->ms_loop = 0.0;
        info->passes = 0;
    }
    if (r == 0) return TLSQ_OK;
    TLSQ_HIP(h, hipSetDevice(h->device));
    const double t_begin = now_ms();
    const int hist_cap = (info && info->dq_hist && info->hist_capacity > 0)
                             ? (int)std::min<int64_t>(info->hist_capacity, iters) : 0;
    // small problems run in one workgroup (k_ga_solo)
    const bool solo = mode == TLSQ_GA_MEAN && !h->comm && d <= 64 && N * (d + 1) <= 18000;
    GaBuffers b;
    // (a caller's average: buffers of the plain mean - w, q, sbuf, state are all it needs)
    if (!solo) TLSQ_TRY(ga_alloc(h, d, N, cb_mode ? TLSQ_GA_MEAN : mode, hist_cap, true, &b));
    std::vector<double> cbU, cbW, cbS;
    if (cb_mode) {
        cbU.resize((size_t)d * N);
        cbW.resize((size_t)N);
        cbS.resize((size_t)d);
    }
    if (h->comm && mode != TLSQ_GA_MEAN) {
        // column shards: the entrywise averages rank the entries of whole rows (:329, :357) - this rank's place in them
        int64_t off = 0, tot = 0;
        for (int k = 0; k < h->nranks; ++k) {
            double v = (k == h->rank) ? (double)N : 0.0;
            TLSQ_TRY(comm_allreduce_host_scalar(h, &v, ncclSum));
            if (k < h->rank) off += (int64_t)v;
            tot += (int64_t)v;
        }
        if (tot >= (int64_t)1 << 32)
            return set_err(h, TLSQ_ERR_UNSUPPORTED, "rpca_ga: the entrywise averages need N < 2^32 columns");
        b.col_off = off;
        b.N_glob = tot;
    }
    // inputs
    const double* src = X;
    int64_t lds = ldX;
    void* p;
    if (!dev && !solo) {
        TLSQ_TRY(ws_get(h, WS_GA_IO, (size_t)d * N * 8, &p));
        TLSQ_TRY(copy2d(h, p, d, X, ldX, d, N, 8, hipMemcpyHostToDevice));
        src = (const double*)p;
        lds = d;
    }
    double* dQ = Q;
    int64_t ldq = ldQ;
    double* dq0 = nullptr;
    {
        TLSQ_TRY(ws_get(h, WS_GA_Q, (size_t)d * r * 8 * 2, &p));
        double* blk = (double*)p;
        if (!dev) {
            dQ = blk;
            ldq = d;
        }
        dq0 = blk + (size_t)d * r;
        if (q0) {
            TLSQ_TRY(copy2d(h, dq0, d, q0, ldq0, d, r, 8, dev ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice));
        } else {
            // randn(d) of :289 — the library's own seeded normals (Julia's global RNG stream cannot be reproduced)
            TLSQ_TRY(launch_fill_gauss(h, dq0, d * r, (unsigned int)(seed * 2654435761ull + 0x6a09e667u)));
        }
    }
    std::vector<double> hist_host;
    int rc = TLSQ_OK;
    TLSQ_HIP(h, hipStreamSynchronize(h->stream));   // uploads done: ms_loop is the component loop alone
    const double t_loop = now_ms();
    int64_t passes = 0;
    if (solo) TLSQ_TRY(run_solo(h, X, d, N, ldX, r, dev, tol, iters, dq0, dQ, ldq, info, hist_cap, &passes, &rc));
    for (int64_t i = 0; i < r && !solo; ++i) {
        // :263-266 (and the deflation :270-271 of the previous component, fused into the same sweep)
        TLSQ_TRY(launch_prepare(h, i == 0 ? src : b.Xw, i == 0 ? lds : d, d, N, i == 0 ? nullptr : dQ + (i - 1) * ldq,
                                b.Xw, b.U, b.norms));
        if (mode == TLSQ_GA_TRIMMED_MEAN) TLSQ_TRY(ga_build_mask(h, &b, d, N, P));
        hipLaunchKernelGGL(k_ga_start, dim3(1), dim3(256), 0, h->stream, dq0 + (size_t)i * d, (int)d, b.q, b.qold, b.st);
        TLSQ_HIP(h, hipGetLastError());
        if (hist_cap > 0) TLSQ_HIP(h, hipMemsetAsync(b.hist, 0xff, (size_t)hist_cap * 8, h->stream));   // NaN fill
        GaState st{};
        int64_t queued = 0;
        // kernels of iterations queued past the converged one return at once (a few microseconds each), a host round
        // trip costs more: queue 8 at a time.  The median's sort cannot be gated by the flag.
        const int64_t burst = (mode == TLSQ_GA_MEDIAN) ? 1 : 8;
        if (cb_mode) {
            // the caller's own average (src/robustPCA.jl:297 with a user closure): U visits the host once per component, then every
            // iteration is weights down (:294-296 on the device), `μ(q, w, U)` on the calling thread, average up, the
            // normalisation and the change dq (:298-304) on the device again
            TLSQ_HIP(h, hipMemcpyAsync(cbU.data(), b.U, (size_t)d * N * 8, hipMemcpyDeviceToHost, h->stream));
            int64_t g = (N + 3) / 4;
            if (g > 4096) g = 4096;
            while (queued < iters) {
                hipLaunchKernelGGL(k_ga_dots, dim3((int)g), dim3(256), 0, h->stream, b.U, (int)d, N, b.norms, b.q, b.w, b.st);
                TLSQ_HIP(h, hipGetLastError());
                TLSQ_HIP(h, hipMemcpyAsync(cbW.data(), b.w, (size_t)N * 8, hipMemcpyDeviceToHost, h->stream));
                TLSQ_HIP(h, hipMemcpyAsync(cbS.data(), b.q, (size_t)d * 8, hipMemcpyDeviceToHost, h->stream));
                TLSQ_HIP(h, hipStreamSynchronize(h->stream));
                const int cst = opts->avg_cb(cbS.data(), cbW.data(), cbU.data(), d, N, d, opts->user);
                if (cst != 0) return set_err(h, TLSQ_ERR_ARG, "rpca_ga: the average callback failed (status %d)", cst);
                TLSQ_HIP(h, hipMemcpyAsync(b.sbuf, cbS.data(), (size_t)d * 8, hipMemcpyHostToDevice, h->stream));
                hipLaunchKernelGGL(k_ga_finalize, dim3(1), dim3(256), 0, h->stream, b.sbuf, (int)d, 2, b.q, b.qold, tol, b.st,
                                   b.hist, hist_cap);
                TLSQ_HIP(h, hipGetLastError());
                ++queued;
                TLSQ_TRY(read_state(h, b.st, &st));
                if (st.converged) break;
            }
        }
        while (queued < iters && !cb_mode) {
            const int64_t nq = std::min<int64_t>(burst, iters - queued);
            for (int64_t k = 0; k < nq; ++k) TLSQ_TRY(ga_iteration(h, &b, d, N, mode, tol, hist_cap));
            queued += nq;
            TLSQ_TRY(read_state(h, b.st, &st));
            if (st.converged) break;
        }
        passes += st.iters;
        if (info) {
            if (info->iters) info->iters[i] = st.iters;
            if (info->status) info->status[i] = st.converged ? 0 : 1;      // 1 = the @warn of :306
            if (info->dq) info->dq[i] = st.dq;
            if (hist_cap > 0) {
                hist_host.resize((size_t)hist_cap);
                TLSQ_HIP(h, hipMemcpyAsync(hist_host.data(), b.hist, (size_t)hist_cap * 8, hipMemcpyDeviceToHost, h->stream));
                TLSQ_HIP(h, hipStreamSynchronize(h->stream));
                memcpy(info->dq_hist + (size_t)i * info->hist_capacity, hist_host.data(), (size_t)hist_cap * 8);
                for (int64_t k = hist_cap; k < info->hist_capacity; ++k)
                    info->dq_hist[(size_t)i * info->hist_capacity + k] = std::numeric_limits<double>::quiet_NaN();
            }
        }
        if (!st.converged) rc = TLSQ_MAXITER;
        TLSQ_HIP(h, hipMemcpyAsync(dQ + (size_t)i * ldq, b.q, (size_t)d * 8, hipMemcpyDeviceToDevice, h->stream));   // :268
    }
    TLSQ_HIP(h, hipStreamSynchronize(h->stream));
    const double t_loop_end = now_ms();
    if (!dev) TLSQ_TRY(copy2d(h, Q, ldQ, dQ, d, d, r, 8, hipMemcpyDeviceToHost));
    TLSQ_HIP(h, hipStreamSynchronize(h->stream));
    if (info) {
        info->ms_loop = t_loop_end - t_loop;
        info->ms_total = now_ms() - t_begin;
        info->passes = passes;
    }
    return rc;
}

// Float32 observations (`rpca_ga(X::Matrix{Float32})`: the reference's method is generic in the element type, src/robustPCA.jl:255):
// the panel travels and lives as fp32 on its way in (half the PCIe bytes of a host-side conversion), is widened once on the
// device, and the iteration runs in the fp64 kernels above - the library's small-arithmetic convention, as for ComplexF32 data;
// Q is rounded to fp32 on the way out.  q0 (optional) is fp32 as well.  A group handle splits the columns like the fp64 entry
// (the conversion then happens on the host: every rank needs its own block).
int tlsq_rpca_ga_f32(tlsq_handle h, const float* X, int64_t d, int64_t N, int64_t ldX, int64_t r, const tlsq_ga_opts* opts,
                     const float* q0, int64_t ldq0, float* Q, int64_t ldQ, tlsq_ga_info* info) {
    TLSQ_TRY(check_handle(h));
    if (!X || !Q || d <= 0 || N <= 0 || ldX < d || ldQ < d || r < 0 || (q0 && ldq0 < d))
        return set_err(h, TLSQ_ERR_ARG, "rpca_ga: bad argument");
    const bool dev = opts && opts->memory == TLSQ_MEM_DEVICE;
    tlsq_ga_opts o;
    if (opts) o = *opts; else tlsq_ga_opts_default(&o);
    std::vector<double> q0d;
    if (q0) {
        std::vector<float> q0h((size_t)d * r);
        if (dev) {
            TLSQ_HIP(h, hipSetDevice(h->device));
            TLSQ_HIP(h, hipMemcpy2D(q0h.data(), (size_t)d * 4, q0, (size_t)ldq0 * 4, (size_t)d * 4, (size_t)r, hipMemcpyDeviceToHost));
        } else {
            for (int64_t c = 0; c < r; ++c) memcpy(q0h.data() + (size_t)c * d, q0 + (size_t)c * ldq0, (size_t)d * 4);
        }
        q0d.assign(q0h.begin(), q0h.end());
    }
    std::vector<double> Qd((size_t)d * std::max<int64_t>(r, 1));
    int st;
    if (is_multi_call(h) && !dev) {
        std::vector<double> Xd((size_t)d * N);
        for (int64_t c = 0; c < N; ++c)
            for (int64_t i = 0; i < d; ++i) Xd[(size_t)(i + c * d)] = (double)X[i + c * ldX];
        o.memory = TLSQ_MEM_HOST;
        st = tlsq_rpca_ga_f64(h, Xd.data(), d, N, d, r, &o, q0 ? q0d.data() : nullptr, d, Qd.data(), d, info);
    } else {
        TLSQ_HIP(h, hipSetDevice(h->device));
        void *xf, *xd, *qd;
        TLSQ_TRY(ws_get(h, WS_GA_F32, (size_t)d * N * 4, &xf));
        TLSQ_TRY(ws_get(h, WS_GA_X64, (size_t)d * N * 8, &xd));
        TLSQ_TRY(ws_get(h, WS_GA_Q64, (size_t)d * std::max<int64_t>(r, 1) * 8 * 2, &qd));
        TLSQ_TRY(copy2d(h, xf, d, X, ldX, d, N, 4, dev ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice));
        TLSQ_TRY((launch_convert<float, double>(h, (const float*)xf, (double*)xd, d * N)));
        double* q0dev = nullptr;
        if (q0) {
            q0dev = (double*)qd + (size_t)d * std::max<int64_t>(r, 1);
            TLSQ_HIP(h, hipMemcpyAsync(q0dev, q0d.data(), (size_t)d * r * 8, hipMemcpyHostToDevice, h->stream));
            TLSQ_HIP(h, hipStreamSynchronize(h->stream));
        }
        o.memory = TLSQ_MEM_DEVICE;
        st = tlsq_rpca_ga_f64(h, (const double*)xd, d, N, d, r, &o, q0dev, d, (double*)qd, d, info);
        if (st >= 0 && r > 0) {
            TLSQ_HIP(h, hipMemcpyAsync(Qd.data(), qd, (size_t)d * r * 8, hipMemcpyDeviceToHost, h->stream));
            TLSQ_HIP(h, hipStreamSynchronize(h->stream));
        }
    }
    if (st < 0) return st;
    std::vector<float> Qf((size_t)d * std::max<int64_t>(r, 1));
    for (size_t i = 0; i < (size_t)d * r; ++i) Qf[i] = (float)Qd[i];
    if (r > 0) {
        if (dev) TLSQ_HIP(h, hipMemcpy2D(Q, (size_t)ldQ * 4, Qf.data(), (size_t)d * 4, (size_t)d * 4, (size_t)r, hipMemcpyHostToDevice));
        else
            for (int64_t c = 0; c < r; ++c) memcpy(Q + (size_t)c * ldQ, Qf.data() + (size_t)c * d, (size_t)d * 4);
    }
    return st;
}

int tlsq_ga_average_f64(tlsq_handle h, int average, double trim, const double* w, const double* U, int64_t d, int64_t N,
                        int64_t ldU, double* s, int memory) {
    TLSQ_TRY(check_handle(h));
    if (!w || !U || !s || d <= 0 || N <= 0 || ldU < d) return set_err(h, TLSQ_ERR_ARG, "ga_average: bad argument");
    if (average != TLSQ_GA_MEAN && average != TLSQ_GA_TRIMMED_MEAN && average != TLSQ_GA_MEDIAN)
        return set_err(h, TLSQ_ERR_ARG, "ga_average: unknown average %d", average);
    if (average == TLSQ_GA_MEDIAN && N < 2)
        return set_err(h, TLSQ_ERR_ARG, "ga_average: entrywise_median needs at least 2 columns (I[end÷2])");
    const double P = (trim == trim) ? trim : 0.1;
    if (average == TLSQ_GA_TRIMMED_MEAN && !(P >= 0.0 && P < 1.0))
        return set_err(h, TLSQ_ERR_ARG, "ga_average: trim fraction outside [0,1)");
    if (h->nranks > 1) return set_err(h, TLSQ_ERR_UNSUPPORTED, "ga_average: single GPU only");
    TLSQ_HIP(h, hipSetDevice(h->device));
    const bool dev = memory == TLSQ_MEM_DEVICE;
    GaBuffers b;
    TLSQ_TRY(ga_alloc(h, d, N, average, 0, false, &b));
    TLSQ_TRY(copy2d(h, b.U, d, U, ldU, d, N, 8, dev ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice));
    TLSQ_HIP(h, hipMemcpyAsync(b.w, w, (size_t)N * 8, dev ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, h->stream));
    if (average == TLSQ_GA_TRIMMED_MEAN) TLSQ_TRY(ga_build_mask(h, &b, d, N, P));
    TLSQ_TRY(ga_sums(h, &b, d, N, average, b.w, nullptr));
    const int ne = average == TLSQ_GA_MEDIAN ? (int)d : ga_entries(d, average);
    if (average != TLSQ_GA_MEDIAN) {
        // borrow the state block for the (unused) flag; k_ga_reduce reads st->converged
        TLSQ_HIP(h, hipMemsetAsync(b.st, 0, sizeof(GaState), h->stream));
        hipLaunchKernelGGL(k_ga_reduce, dim3((ne + 63) / 64), dim3(1024), 0, h->stream, b.partial, b.nblk, b.pstride, ne,
                           (int)d, 0, b.sbuf, 0, b.q, b.qold, 0.0, b.st, (double*)nullptr, 0);
        TLSQ_HIP(h, hipGetLastError());
    }
    std::vector<double> hs((size_t)ne);
    TLSQ_HIP(h, hipMemcpyAsync(hs.data(), b.sbuf, (size_t)ne * 8, hipMemcpyDeviceToHost, h->stream));
    TLSQ_HIP(h, hipStreamSynchronize(h->stream));
    std::vector<double> out((size_t)d);
    for (int64_t j = 0; j < d; ++j) {
        if (average == TLSQ_GA_MEAN) out[(size_t)j] = hs[(size_t)j] / hs[(size_t)d];                 // :319
        else if (average == TLSQ_GA_TRIMMED_MEAN) out[(size_t)j] = hs[(size_t)j] / hs[(size_t)(d + j)];   // :333
        else out[(size_t)j] = hs[(size_t)j];                                                          // :359
    }
    if (dev) {
        TLSQ_HIP(h, hipMemcpyAsync(s, out.data(), (size_t)d * 8, hipMemcpyHostToDevice, h->stream));
        TLSQ_HIP(h, hipStreamSynchronize(h->stream));
    } else {
        memcpy(s, out.data(), (size_t)d * 8);
    }
    return TLSQ_OK;
}

}  // extern "C"
