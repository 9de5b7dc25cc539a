// flts — fast least trimmed squares (src/flts.jl), on the device.
//
// Reference (paths relative to the reference package):
//     flts           src/flts.jl:42-89     h rule (:53-61), N initial subsets, two C-steps, top 10, a third C-step, winner
//     optimize_H     src/flts.jl:92-105    every iteration restarts from the INITIAL theta: one distinct C-step per call
//     get_initial_H  src/flts.jl:108-124   p-subset, redrawn with p+i rows while rank(A[J,:]) < p, theta_J = A[J,:] \ y[J]
//     C_step         src/flts.jl:127-138   r = A theta - y, H = sortperm(abs.(r))[1:h], theta' = A[H,:] \ y[H], Q
//
// Layout of one call (all subsets of a stage at once, "slots" = the subsets of the stage):
//   k_flts_init      one wave per initial subset: the draw (flts_draw, shared with the host's tlsq_flts_subset), Julia's rank
//                    rule through a one-sided Jacobi SVD of A[J,:], the redraws, theta_J (LU with partial pivoting for a
//                    square J, minimum norm from the SVD for a tall one).
//   C-step           H_s is never materialised: it is (theta_old_s, cut_s), cut_s = the h-th smallest composite key
//                    (bits of |r_i|, i) - distinct for every row, so "key <= cut" is exactly the first h entries of the
//                    stable sortperm.  The cut comes from an MSD radix select (10-bit digits, k_flts_hist + k_flts_pick)
//                    until the bucket holding rank h-1 has at most kCap rows, which are gathered and sorted in LDS
//                    (k_flts_gather, k_flts_cut).  Then the masked moments G = sum_H a a', b = sum_H a y in a fixed order
//                    (k_flts_moments: per-chunk partials, k_flts_reduce: chunks summed in order), the p x p solve
//                    (k_flts_solve: cyclic Jacobi eigensolve of G, eigenvalues below 10 p eps lambda_max dropped - the
//                    minimum-norm solution of a rank-deficient A_H), and Q for the new theta (k_flts_q + k_flts_reduce).
//                    Every pass computes residuals with the one function flts_resid, so membership agrees bit for bit.
//   bookkeeping      k_flts_rank: the stable order of Q over the subsets (ties by subset index) on the device; the winner's
//                    H in sortperm order by a stable radix sort of its (|r| bits, row) pairs.
//
// fp32 data: residuals and keys in float (what the reference computes for Float32 arrays), moments, solves and Q in double.

#include <cstring>

#include <rocprim/rocprim.hpp>

#include "internal.hpp"

#pragma clang fp contract(off)

namespace tlsq {

namespace {

typedef unsigned __int128 u128;

constexpr int kMaxP = 64;      // largest p
constexpr int kSB = 8;         // subsets per workgroup of the key passes
constexpr int kDig = 10;       // bits per radix digit
constexpr int kNB = 1 << kDig;
constexpr int kCap = 2048;     // a bucket this small is gathered and sorted
constexpr int kTileR = 64;     // rows per LDS tile of the moments kernel
constexpr int kAcc = 12;       // moment accumulators per thread
enum { SEL_MORE = 0, SEL_GATHER = 1 };

struct FltsSel {
    u128 prefix;               // key bits fixed so far (bits >= shift)
    unsigned long long rank;   // rank still to be found among the keys that match them
    unsigned long long count;  // how many keys match them
    int shift, status;
};

// ---- the draw: Floyd's algorithm on a counter-based hash (host and device) -------------------------------------------
__host__ __device__ inline uint64_t flts_mix(uint64_t x) {   // splitmix64 finaliser
    x ^= x >> 30;
    x *= 0xBF58476D1CE4E5B9ull;
    x ^= x >> 27;
    x *= 0x94D049BB133111EBull;
    x ^= x >> 31;
    return x;
}
__host__ __device__ inline uint64_t flts_hash(uint64_t seed, uint64_t s, uint64_t attempt, uint64_t t) {
    uint64_t x = flts_mix(seed + 0x9E3779B97F4A7C15ull);
    x = flts_mix(x ^ (s * 0xD1B54A32D192ED03ull + 0x2545F4914F6CDD1Dull));
    x = flts_mix(x ^ (attempt * 0xABC98388FB8FAC03ull + 0x8CB92BA72F3D8DD7ull));
    return flts_mix(x ^ t);
}
__host__ __device__ inline uint64_t flts_mulhi(uint64_t a, uint64_t b) {
#ifdef __HIP_DEVICE_COMPILE__
    return __umul64hi(a, b);
#else
    return (uint64_t)(((unsigned __int128)a * b) >> 64);
#endif
}
// J[0..k) = k distinct indices of [0, n) in draw order
__host__ __device__ inline void flts_draw(uint64_t seed, int64_t s, int64_t attempt, int64_t n, int64_t k, int64_t* J) {
    int64_t m = 0;
    for (int64_t jj = n - k; jj < n; ++jj) {
        const int64_t t = (int64_t)flts_mulhi(flts_hash(seed, (uint64_t)s, (uint64_t)attempt, (uint64_t)jj), (uint64_t)jj + 1);
        bool seen = false;
        for (int64_t q = 0; q < m; ++q)
            if (J[q] == t) {
                seen = true;
                break;
            }
        J[m++] = seen ? jj : t;
    }
}

// ---- keys -----------------------------------------------------------------------------------------------------------
template <typename T>
struct FK;
template <>
struct FK<double> {
    static constexpr int KB = 63 + 32;   // key bits: |r| (sign bit dropped) then the row index
    static constexpr double eps = 2.220446049250313e-16;
    __device__ static unsigned long long vbits(double r) {
        const double a = fabs(r);
        return a != a ? 0x7FF8000000000000ull : (unsigned long long)__double_as_longlong(a);
    }
};
template <>
struct FK<float> {
    static constexpr int KB = 31 + 32;
    static constexpr double eps = 1.1920928955078125e-7;
    __device__ static unsigned long long vbits(float r) {
        const float a = fabsf(r);
        return a != a ? 0x7FC00000ull : (unsigned long long)__float_as_uint(a);
    }
};
template <typename T>
__device__ inline u128 flts_key(T r, int64_t i) {
    return ((u128)FK<T>::vbits(r) << 32) | (u128)(uint32_t)i;
}

// THE residual of every pass: r[s] = (sum_j a_j theta_s[j]) - y_i for the kSB thetas th[j*kSB + s], j in order.
// a points at the row's first element (global A or an LDS tile), element j at a[j * lda].
template <typename T>
__device__ inline void flts_resid(const T* a, int64_t lda, int p, const T* th, T yi, T* r) {
    T acc[kSB];
#pragma unroll
    for (int s = 0; s < kSB; ++s) acc[s] = (T)0;
    for (int j = 0; j < p; ++j) {
        const T x = a[(int64_t)j * lda];
#pragma unroll
        for (int s = 0; s < kSB; ++s) acc[s] = acc[s] + x * th[j * kSB + s];
    }
#pragma unroll
    for (int s = 0; s < kSB; ++s) r[s] = acc[s] - yi;
}

// theta (double, slot-major, p per slot) of slots s0..s0+kSB-1 -> LDS as T, zero for slots past nslots
template <typename T>
__device__ inline void flts_load_theta(T* th, const double* theta, int p, int s0, int nslots, int ns) {
    for (int e = threadIdx.x; e < p * kSB; e += blockDim.x) {
        const int j = e / kSB, s = e % kSB;
        th[e] = (s < ns && s0 + s < nslots) ? (T)theta[(size_t)(s0 + s) * p + j] : (T)0;
    }
}

// ---- initial subsets ------------------------------------------------------------------------------------------------
// round-robin pairing of P2 (even) columns: round rd, pair k
__device__ inline void flts_pair(int rd, int k, int P2, int* a, int* b) {
    auto idx = [&](int q) { return q == 0 ? 0 : 1 + (q - 1 + rd) % (P2 - 1); };
    int x = idx(k), y = idx(P2 - 1 - k);
    *a = x < y ? x : y;
    *b = x < y ? y : x;
}

// one-sided Jacobi SVD of W (m x p, ld m) by one wave: W <- W V, V (p x p) accumulates the rotations
__device__ void flts_svd_wave(double* W, int64_t m, int p, double* V, int* flag) {
    const int l = threadIdx.x, P2 = p + (p & 1);
    for (int sweep = 0; sweep < 60 && P2 > 1; ++sweep) {
        if (l == 0) *flag = 0;
        __syncthreads();
        for (int rd = 0; rd < P2 - 1; ++rd) {
            if (l < P2 / 2) {
                int a, b;
                flts_pair(rd, l, P2, &a, &b);
                if (b < p) {
                    double al = 0.0, be = 0.0, ga = 0.0;
                    for (int64_t r = 0; r < m; ++r) {
                        const double x = W[r + a * m], z = W[r + b * m];
                        al = al + x * x;
                        be = be + z * z;
                        ga = ga + x * z;
                    }
                    if (ga != 0.0 && fabs(ga) > 2.220446049250313e-16 * sqrt(al * be)) {
                        const double zeta = (be - al) / (2.0 * ga);
                        const double t = (zeta >= 0.0 ? 1.0 : -1.0) / (fabs(zeta) + sqrt(1.0 + zeta * zeta));
                        const double c = 1.0 / sqrt(1.0 + t * t), sn = c * t;
                        for (int64_t r = 0; r < m; ++r) {
                            const double x = W[r + a * m], z = W[r + b * m];
                            W[r + a * m] = c * x - sn * z;
                            W[r + b * m] = sn * x + c * z;
                        }
                        for (int r = 0; r < p; ++r) {
                            const double x = V[r + a * p], z = V[r + b * p];
                            V[r + a * p] = c * x - sn * z;
                            V[r + b * p] = sn * x + c * z;
                        }
                        *flag = 1;
                    }
                }
            }
            __syncthreads();
        }
        const int more = *flag;
        __syncthreads();
        if (!more) break;
    }
}

// status: 0 ok, 1 the draw outgrew the scratch (cap rows), 2 singular square subset (LU zero pivot)
template <typename T>
__global__ __launch_bounds__(64) void k_flts_init(const T* __restrict__ A, int64_t lda, const T* __restrict__ y, int64_t n,
                                                  int p, uint64_t seed, int64_t s0, int64_t nsub, int64_t cap,
                                                  double* __restrict__ Wb, double* __restrict__ Vb, int64_t* __restrict__ Jb,
                                                  double* __restrict__ yb, double* __restrict__ theta,
                                                  int64_t* __restrict__ rows, int* __restrict__ status) {
    const int64_t s = s0 + blockIdx.x;
    if (s >= nsub) return;
    const int l = threadIdx.x;
    double* W = Wb + (size_t)blockIdx.x * cap * p;
    double* V = Vb + (size_t)blockIdx.x * p * p;
    int64_t* J = Jb + (size_t)blockIdx.x * cap;
    double* yJ = yb + (size_t)blockIdx.x * cap;
    __shared__ double sig[kMaxP], cc[kMaxP];
    __shared__ int flag, rk;
    __shared__ double tol_s;
    __shared__ int bad;
    int64_t m = p;
    for (;;) {
        if (m > cap) {
            if (l == 0) {
                status[s] = 1;
                rows[s] = m;
            }
            return;
        }
        if (l == 0) flts_draw(seed, s, m - p, n, m, J);   // attempt a draws p + a rows (:110, :115)
        __syncthreads();
        for (int64_t e = l; e < m * p; e += 64) {
            const int64_t r = e % m, c = e / m;
            W[r + c * m] = (double)A[J[r] + c * lda];
        }
        for (int e = l; e < p * p; e += 64) V[e] = (e % p == e / p) ? 1.0 : 0.0;
        __syncthreads();
        flts_svd_wave(W, m, p, V, &flag);
        if (l < p) {
            double acc = 0.0;
            for (int64_t r = 0; r < m; ++r) acc = acc + W[r + l * m] * W[r + l * m];
            sig[l] = sqrt(acc);
        }
        __syncthreads();
        if (l == 0) {   // Julia's rank: count(sigma > min(m, p) eps(T) sigma_1)
            double s1 = 0.0;
            for (int j = 0; j < p; ++j) s1 = fmax(s1, sig[j]);
            const double tol = (double)(m < p ? m : p) * FK<T>::eps * s1;
            int c = 0;
            for (int j = 0; j < p; ++j) c += sig[j] > tol ? 1 : 0;
            rk = c;
            tol_s = tol;
        }
        __syncthreads();
        if (rk < p && m + 2 < n) {   // while (p+i+1) < n && rank(A[J,:]) < p  (:114), with m = p + i - 1
            ++m;
            __syncthreads();
            continue;
        }
        break;
    }
    for (int64_t r = l; r < m; r += 64) yJ[r] = (double)y[J[r]];
    __syncthreads();
    if (m == p) {
        // square: LU with partial pivoting on a fresh copy of A[J,:] (Julia's `\` for a square matrix)
        for (int64_t e = l; e < m * p; e += 64) {
            const int64_t r = e % m, c = e / m;
            W[r + c * m] = (double)A[J[r] + c * lda];
        }
        if (l == 0) bad = 0;
        __syncthreads();
        for (int k = 0; k < p; ++k) {
            if (l == 0) {
                int pv = k;
                double best = fabs(W[k + k * p]);
                for (int r = k + 1; r < p; ++r)
                    if (fabs(W[r + k * p]) > best) {
                        best = fabs(W[r + k * p]);
                        pv = r;
                    }
                if (best == 0.0) bad = 1;
                if (pv != k) {
                    for (int c = 0; c < p; ++c) {
                        const double t = W[k + c * p];
                        W[k + c * p] = W[pv + c * p];
                        W[pv + c * p] = t;
                    }
                    const double t = yJ[k];
                    yJ[k] = yJ[pv];
                    yJ[pv] = t;
                }
            }
            __syncthreads();
            if (bad) break;
            if (l > k && l < p) {
                const double f = W[l + k * p] / W[k + k * p];
                W[l + k * p] = f;
                for (int c = k + 1; c < p; ++c) W[l + c * p] = W[l + c * p] - f * W[k + c * p];
                yJ[l] = yJ[l] - f * yJ[k];
            }
            __syncthreads();
        }
        if (l == 0) {
            if (bad) {
                status[s] = 2;
            } else {
                for (int k = p - 1; k >= 0; --k) {
                    double t = yJ[k];
                    for (int c = k + 1; c < p; ++c) t = t - W[k + c * p] * cc[c];
                    cc[k] = t / W[k + k * p];
                }
                status[s] = 0;
            }
        }
        __syncthreads();
        if (l < p) theta[(size_t)s * p + l] = cc[l];
    } else {
        // tall: minimum-norm least squares from the SVD, singular values above min(m, p) eps sigma_1 (pivoted QR's rcond)
        if (l < p) {
            double t = 0.0;
            for (int64_t r = 0; r < m; ++r) t = t + W[r + l * m] * yJ[r];
            cc[l] = sig[l] > tol_s ? (t / sig[l]) / sig[l] : 0.0;
        }
        __syncthreads();
        if (l < p) {
            double t = 0.0;
            for (int j = 0; j < p; ++j) t = t + V[l + j * p] * cc[j];
            theta[(size_t)s * p + l] = t;
        }
        if (l == 0) status[s] = 0;
    }
    if (l == 0) rows[s] = m;
}

// ---- C-step: radix select of the cut ---------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(256) void k_flts_sel_init(FltsSel* __restrict__ sel, int nslots, int64_t n, int64_t h) {
    const int s = blockIdx.x * 256 + threadIdx.x;
    if (s >= nslots) return;
    FltsSel st;
    st.prefix = 0;
    st.rank = (unsigned long long)(h - 1);
    st.count = (unsigned long long)n;
    st.shift = FK<T>::KB;
    st.status = n <= kCap ? SEL_GATHER : SEL_MORE;
    sel[s] = st;
}

template <typename T>
__global__ __launch_bounds__(256) void k_flts_hist(const T* __restrict__ A, int64_t lda, const T* __restrict__ y, int64_t n,
                                                   int p, const double* __restrict__ theta, int nslots,
                                                   const FltsSel* __restrict__ sel, unsigned* __restrict__ ghist,
                                                   int64_t rpc) {
    __shared__ unsigned hs[kSB * kNB];
    __shared__ T th[kMaxP * kSB];
    __shared__ u128 pre[kSB];
    __shared__ int sh[kSB], act[kSB], any;
    const int s0 = blockIdx.y * kSB, tid = threadIdx.x;
    for (int e = tid; e < kSB * kNB; e += 256) hs[e] = 0u;
    flts_load_theta(th, theta, p, s0, nslots, kSB);
    if (tid < kSB) {
        const bool on = s0 + tid < nslots && sel[s0 + tid].status == SEL_MORE;
        act[tid] = on ? 1 : 0;
        if (on) {
            pre[tid] = sel[s0 + tid].prefix;
            sh[tid] = sel[s0 + tid].shift;
        } else {
            pre[tid] = 0;
            sh[tid] = FK<T>::KB;
        }
    }
    __syncthreads();
    if (tid == 0) {
        int a = 0;
        for (int s = 0; s < kSB; ++s) a |= act[s];
        any = a;
    }
    __syncthreads();
    if (!any) return;
    const int64_t r0 = (int64_t)blockIdx.x * rpc, r1 = r0 + rpc < n ? r0 + rpc : n;
    for (int64_t i = r0 + tid; i < r1; i += 256) {
        T r[kSB];
        flts_resid(A + i, lda, p, th, y[i], r);
#pragma unroll
        for (int s = 0; s < kSB; ++s) {
            if (!act[s]) continue;
            const u128 key = flts_key(r[s], i);
            const int shf = sh[s];
            if ((key >> shf) != (pre[s] >> shf)) continue;
            const int lo = shf > kDig ? shf - kDig : 0;
            const unsigned d = (unsigned)(key >> lo) & ((1u << (shf - lo)) - 1u);
            atomicAdd(&hs[s * kNB + d], 1u);
        }
    }
    __syncthreads();
    for (int e = tid; e < kSB * kNB; e += 256)
        if (hs[e] && act[e / kNB]) atomicAdd(&ghist[(size_t)(s0 + e / kNB) * kNB + (e % kNB)], hs[e]);
}

// one thread per slot: the bucket of the digit below `shift` that holds the rank; clears the histogram
__global__ __launch_bounds__(64) void k_flts_pick(unsigned* __restrict__ ghist, FltsSel* __restrict__ sel, int nslots,
                                                  int* __restrict__ flags) {
    const int s = blockIdx.x * 64 + threadIdx.x;
    if (s >= nslots) return;
    FltsSel st = sel[s];
    if (st.status != SEL_MORE) return;
    unsigned* hh = ghist + (size_t)s * kNB;
    const int lo = st.shift > kDig ? st.shift - kDig : 0, nb = 1 << (st.shift - lo);
    unsigned long long cum = 0, before = 0, cnt = 0;
    int found = -1;
    for (int b = 0; b < nb; ++b) {
        const unsigned long long c = hh[b];
        if (found < 0 && st.rank < cum + c) {
            found = b;
            before = cum;
            cnt = c;
        }
        cum += c;
        hh[b] = 0u;
    }
    if (found < 0 || cum != st.count) {   // cannot happen: the counts of one pass add up to the bucket's count
        atomicAdd(&flags[1], 1);
        found = found < 0 ? 0 : found;
    }
    st.prefix |= (u128)(unsigned)found << lo;
    st.rank -= before;
    st.count = cnt;
    st.shift = lo;
    st.status = (cnt <= (unsigned long long)kCap || lo == 0) ? SEL_GATHER : SEL_MORE;
    if (st.status == SEL_MORE) atomicAdd(&flags[0], 1);
    sel[s] = st;
}

// the (at most kCap) keys of each slot that match its prefix
template <typename T>
__global__ __launch_bounds__(256) void k_flts_gather(const T* __restrict__ A, int64_t lda, const T* __restrict__ y, int64_t n,
                                                     int p, const double* __restrict__ theta, int nslots,
                                                     const FltsSel* __restrict__ sel, u128* __restrict__ cand,
                                                     unsigned* __restrict__ ccount, int64_t rpc) {
    __shared__ T th[kMaxP * kSB];
    __shared__ u128 pre[kSB];
    __shared__ int sh[kSB], act[kSB];
    const int s0 = blockIdx.y * kSB, tid = threadIdx.x;
    flts_load_theta(th, theta, p, s0, nslots, kSB);
    if (tid < kSB) {
        const bool on = s0 + tid < nslots;
        act[tid] = on ? 1 : 0;
        pre[tid] = on ? sel[s0 + tid].prefix : (u128)0;
        sh[tid] = on ? sel[s0 + tid].shift : FK<T>::KB;
    }
    __syncthreads();
    const int64_t r0 = (int64_t)blockIdx.x * rpc, r1 = r0 + rpc < n ? r0 + rpc : n;
    for (int64_t i = r0 + tid; i < r1; i += 256) {
        T r[kSB];
        flts_resid(A + i, lda, p, th, y[i], r);
#pragma unroll
        for (int s = 0; s < kSB; ++s) {
            if (!act[s]) continue;
            const u128 key = flts_key(r[s], i);
            const int shf = sh[s];
            if ((key >> shf) != (pre[s] >> shf)) continue;
            const unsigned q = atomicAdd(&ccount[s0 + s], 1u);
            if (q < (unsigned)kCap) cand[(size_t)(s0 + s) * kCap + q] = key;
        }
    }
}

// one workgroup per slot: sort the gathered keys, cut = the one at the remaining rank
__global__ __launch_bounds__(256) void k_flts_cut(const u128* __restrict__ cand, const unsigned* __restrict__ ccount,
                                                  const FltsSel* __restrict__ sel, u128* __restrict__ cut,
                                                  int* __restrict__ flags) {
    __shared__ u128 ks[kCap];
    const int s = blockIdx.x, tid = threadIdx.x;
    const FltsSel st = sel[s];
    const unsigned cnt0 = ccount[s];
    const int cnt = cnt0 < (unsigned)kCap ? (int)cnt0 : kCap;
    int np2 = 1;
    while (np2 < cnt) np2 <<= 1;
    for (int i = tid; i < np2; i += 256) ks[i] = i < cnt ? cand[(size_t)s * kCap + i] : ~(u128)0;
    __syncthreads();
    for (int k = 2; k <= np2; k <<= 1) {
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int i = tid; i < np2; i += 256) {
                const int ixj = i ^ j;
                if (ixj > i) {
                    const u128 a = ks[i], b = ks[ixj];
                    const bool up = (i & k) == 0;
                    if ((a > b) == up) {
                        ks[i] = b;
                        ks[ixj] = a;
                    }
                }
            }
            __syncthreads();
        }
    }
    if (tid == 0) {
        if ((unsigned long long)cnt0 != st.count || st.rank >= (unsigned long long)cnt) {
            atomicAdd(&flags[1], 1);
            cut[s] = ~(u128)0;
        } else {
            cut[s] = ks[st.rank];
        }
    }
}

// ---- C-step: masked moments, solve, Q --------------------------------------------------------------------------------
// part[(chunk * nslots + slot) * M + f]:  f < npairs: G[j][k] (j <= k, row by row), then b[j], then the member count
template <typename T>
__global__ __launch_bounds__(256) void k_flts_moments(const T* __restrict__ A, int64_t lda, const T* __restrict__ y, int64_t n,
                                                      int p, const double* __restrict__ theta, int nslots, int sbm,
                                                      const u128* __restrict__ cut, double* __restrict__ part, int64_t rpc,
                                                      int M) {
    __shared__ T As[kMaxP * kTileR];
    __shared__ T ys[kTileR];
    __shared__ T th[kMaxP * kSB];
    __shared__ unsigned char mk[kTileR * kSB];
    __shared__ u128 cs[kSB];
    const int s0 = blockIdx.y * sbm, tid = threadIdx.x;
    flts_load_theta(th, theta, p, s0, nslots, sbm);
    if (tid < kSB) cs[tid] = (tid < sbm && s0 + tid < nslots) ? cut[s0 + tid] : (u128)0;
    const int npairs = p * (p + 1) / 2;
    // the entries this thread owns: e = tid + 256 q over (slot, f)
    int es[kAcc], ej[kAcc], ek[kAcc];   // ek: -1 b_j, -2 count, -3 none
    double acc[kAcc];
#pragma unroll
    for (int q = 0; q < kAcc; ++q) {
        acc[q] = 0.0;
        const int e = tid + 256 * q;
        es[q] = 0;
        ej[q] = 0;
        ek[q] = -3;
        if (e < sbm * M && s0 + e / M < nslots) {
            es[q] = e / M;
            int f = e % M;
            if (f < npairs) {
                int j = 0;
                while (f >= p - j) {
                    f -= p - j;
                    ++j;
                }
                ej[q] = j;
                ek[q] = j + f;
            } else if (f < npairs + p) {
                ej[q] = f - npairs;
                ek[q] = -1;
            } else {
                ek[q] = -2;
            }
        }
    }
    const int64_t r0 = (int64_t)blockIdx.x * rpc, r1 = r0 + rpc < n ? r0 + rpc : n;
    for (int64_t t0 = r0; t0 < r1; t0 += kTileR) {
        const int rows = (int)(r1 - t0 < kTileR ? r1 - t0 : kTileR);
        __syncthreads();
        for (int e = tid; e < p * kTileR; e += 256) {
            const int j = e / kTileR, r = e % kTileR;
            As[e] = r < rows ? A[t0 + r + (int64_t)j * lda] : (T)0;
        }
        if (tid < kTileR) ys[tid] = tid < rows ? y[t0 + tid] : (T)0;
        __syncthreads();
        if (tid < rows) {
            T r[kSB];
            flts_resid(As + tid, kTileR, p, th, ys[tid], r);
#pragma unroll
            for (int s = 0; s < kSB; ++s) mk[tid * kSB + s] = (s < sbm && flts_key(r[s], t0 + tid) <= cs[s]) ? 1 : 0;
        }
        __syncthreads();
#pragma unroll
        for (int q = 0; q < kAcc; ++q) {
            if (ek[q] == -3) continue;
            const int s = es[q], j = ej[q], k = ek[q];
            double a = acc[q];
            if (k >= 0) {
                for (int r = 0; r < rows; ++r)
                    if (mk[r * kSB + s]) a = a + (double)As[j * kTileR + r] * (double)As[k * kTileR + r];
            } else if (k == -1) {
                for (int r = 0; r < rows; ++r)
                    if (mk[r * kSB + s]) a = a + (double)As[j * kTileR + r] * (double)ys[r];
            } else {
                for (int r = 0; r < rows; ++r)
                    if (mk[r * kSB + s]) a = a + 1.0;
            }
            acc[q] = a;
        }
    }
#pragma unroll
    for (int q = 0; q < kAcc; ++q) {
        if (ek[q] == -3) continue;
        const int e = tid + 256 * q;
        part[((size_t)blockIdx.x * nslots + s0 + es[q]) * M + e % M] = acc[q];
    }
}

// out[i] = sum over c (in order) of part[c * stride + i]
__global__ __launch_bounds__(256) void k_flts_reduce(const double* __restrict__ part, int64_t stride, int nchunks,
                                                     double* __restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= stride) return;
    double a = 0.0;
    for (int c = 0; c < nchunks; ++c) a = a + part[(size_t)c * stride + i];
    out[i] = a;
}

// one wave per slot: theta_new = minimum-norm solution of G theta = b by a cyclic Jacobi eigensolve of G
__global__ __launch_bounds__(64) void k_flts_solve(const double* __restrict__ mom, int M, int p, int64_t h,
                                                   double* __restrict__ Vb, double* __restrict__ theta_new,
                                                   int* __restrict__ flags) {
    __shared__ double G[kMaxP * kMaxP];
    __shared__ double bb[kMaxP], cc[kMaxP], rc[kMaxP / 2], rs[kMaxP / 2];
    __shared__ int ra[kMaxP / 2], rb[kMaxP / 2], flag;
    const int s = blockIdx.x, l = threadIdx.x, P2 = p + (p & 1);
    const double* m = mom + (size_t)s * M;
    double* V = Vb + (size_t)s * p * p;
    {
        int f = 0;
        for (int j = 0; j < p; ++j)
            for (int k = j; k < p; ++k, ++f)
                if ((f & 63) == l) {
                    G[j * p + k] = m[f];
                    G[k * p + j] = m[f];
                }
    }
    if (l < p) bb[l] = m[p * (p + 1) / 2 + l];
    for (int e = l; e < p * p; e += 64) V[e] = (e % p == e / p) ? 1.0 : 0.0;
    if (l == 0 && m[M - 1] != (double)h) atomicAdd(&flags[2], 1);   // members counted != h
    __syncthreads();
    for (int sweep = 0; sweep < 60 && P2 > 1; ++sweep) {
        if (l == 0) flag = 0;
        __syncthreads();
        for (int rd = 0; rd < P2 - 1; ++rd) {
            if (l < P2 / 2) {
                int a, b;
                flts_pair(rd, l, P2, &a, &b);
                double c = 1.0, sn = 0.0;
                if (b < p) {
                    const double al = G[a * p + a], be = G[b * p + b], ga = G[a * p + b];
                    if (ga != 0.0 && fabs(ga) > 2.220446049250313e-16 * sqrt(fabs(al * be))) {
                        const double zeta = (be - al) / (2.0 * ga);
                        const double t = (zeta >= 0.0 ? 1.0 : -1.0) / (fabs(zeta) + sqrt(1.0 + zeta * zeta));
                        c = 1.0 / sqrt(1.0 + t * t);
                        sn = c * t;
                        flag = 1;
                    }
                }
                ra[l] = a;
                rb[l] = b < p ? b : a;
                rc[l] = c;
                rs[l] = b < p ? sn : 0.0;
            }
            __syncthreads();
            // G <- G J and V <- V J (columns a, b of every pair)
            for (int e = l; e < (P2 / 2) * p; e += 64) {
                const int q = e / p, r = e % p;
                if (rs[q] == 0.0) continue;
                const int a = ra[q], b = rb[q];
                const double c = rc[q], sn = rs[q];
                const double x = G[r * p + a], z = G[r * p + b];
                G[r * p + a] = c * x - sn * z;
                G[r * p + b] = sn * x + c * z;
                const double vx = V[r + a * p], vz = V[r + b * p];
                V[r + a * p] = c * vx - sn * vz;
                V[r + b * p] = sn * vx + c * vz;
            }
            __syncthreads();
            // G <- J' G (rows a, b)
            for (int e = l; e < (P2 / 2) * p; e += 64) {
                const int q = e / p, r = e % p;
                if (rs[q] == 0.0) continue;
                const int a = ra[q], b = rb[q];
                const double c = rc[q], sn = rs[q];
                const double x = G[a * p + r], z = G[b * p + r];
                G[a * p + r] = c * x - sn * z;
                G[b * p + r] = sn * x + c * z;
            }
            __syncthreads();
        }
        const int more = flag;
        __syncthreads();
        if (!more) break;
    }
    __shared__ double tol_s;
    if (l == 0) {
        double lmax = 0.0;
        for (int j = 0; j < p; ++j) lmax = fmax(lmax, G[j * p + j]);
        tol_s = 10.0 * (double)p * 2.220446049250313e-16 * lmax;
    }
    __syncthreads();
    if (l < p) {
        const double lam = G[l * p + l];
        double t = 0.0;
        for (int k = 0; k < p; ++k) t = t + V[k + l * p] * bb[k];
        cc[l] = lam > tol_s ? t / lam : 0.0;
    }
    __syncthreads();
    if (l < p) {
        double t = 0.0;
        for (int j = 0; j < p; ++j) t = t + V[l + j * p] * cc[j];
        theta_new[(size_t)s * p + l] = t;
    }
}

// part[chunk * nslots + slot] = sum over the chunk's members (theta_old, cut) of (a' theta_new - y)^2
template <typename T>
__global__ __launch_bounds__(256) void k_flts_q(const T* __restrict__ A, int64_t lda, const T* __restrict__ y, int64_t n, int p,
                                                const double* __restrict__ theta_old, const double* __restrict__ theta_new,
                                                int nslots, const u128* __restrict__ cut, double* __restrict__ part,
                                                int64_t rpc) {
    __shared__ T th[kMaxP * kSB], tn[kMaxP * kSB];
    __shared__ u128 cs[kSB];
    __shared__ double red[256 * kSB];
    const int s0 = blockIdx.y * kSB, tid = threadIdx.x;
    flts_load_theta(th, theta_old, p, s0, nslots, kSB);
    flts_load_theta(tn, theta_new, p, s0, nslots, kSB);
    if (tid < kSB) cs[tid] = s0 + tid < nslots ? cut[s0 + tid] : (u128)0;
    __syncthreads();
    double acc[kSB];
#pragma unroll
    for (int s = 0; s < kSB; ++s) acc[s] = 0.0;
    const int64_t r0 = (int64_t)blockIdx.x * rpc, r1 = r0 + rpc < n ? r0 + rpc : n;
    for (int64_t i = r0 + tid; i < r1; i += 256) {
        T r[kSB], rn[kSB];
        flts_resid(A + i, lda, p, th, y[i], r);
        flts_resid(A + i, lda, p, tn, y[i], rn);
#pragma unroll
        for (int s = 0; s < kSB; ++s)
            if (flts_key(r[s], i) <= cs[s]) acc[s] = acc[s] + (double)rn[s] * (double)rn[s];
    }
#pragma unroll
    for (int s = 0; s < kSB; ++s) red[s * 256 + tid] = acc[s];
    __syncthreads();
    if (tid < kSB && s0 + tid < nslots) {
        double a = 0.0;
        for (int t = 0; t < 256; ++t) a = a + red[tid * 256 + t];
        part[(size_t)blockIdx.x * nslots + s0 + tid] = a;
    }
}

// order[rank] = s: the stable order of Q (Julia's isless: NaN last), ties by subset index
__global__ __launch_bounds__(256) void k_flts_rank(const double* __restrict__ Q, int N, int64_t* __restrict__ order) {
    const int s = blockIdx.x * 256 + threadIdx.x;
    if (s >= N) return;
    auto key = [](double q) -> unsigned long long {
        unsigned long long u = (unsigned long long)__double_as_longlong(q);
        if (q != q) u = 0x7FF8000000000000ull;
        return (u >> 63) ? ~u : (u | 0x8000000000000000ull);
    };
    const unsigned long long ks = key(Q[s]);
    int r = 0;
    for (int t = 0; t < N; ++t) {
        const unsigned long long kt = key(Q[t]);
        r += (kt < ks || (kt == ks && t < s)) ? 1 : 0;
    }
    order[r] = s;
}

// theta_dst[i] = theta_src[ids[i]] (p each)
__global__ __launch_bounds__(256) void k_flts_take(const double* __restrict__ src, const int64_t* __restrict__ ids, int cnt, int p,
                                                   double* __restrict__ dst) {
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e < cnt * p) dst[e] = src[(size_t)ids[e / p] * p + e % p];
}

// the winner's (|r| bits, row) pairs for the stable sort that yields H in sortperm order
template <typename T>
__global__ __launch_bounds__(256) void k_flts_hkeys(const T* __restrict__ A, int64_t lda, const T* __restrict__ y, int64_t n, int p,
                                                    const double* __restrict__ theta, unsigned long long* __restrict__ keys,
                                                    unsigned* __restrict__ idx) {
    __shared__ T th[kMaxP * kSB];
    flts_load_theta(th, theta, p, 0, 1, 1);
    __syncthreads();
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        T r[kSB];
        flts_resid(A + i, lda, p, th, y[i], r);
        keys[i] = FK<T>::vbits(r[0]);
        idx[i] = (unsigned)i;
    }
}

template <typename T>
__global__ __launch_bounds__(256) void k_flts_finite(const T* __restrict__ A, int64_t lda, const T* __restrict__ y, int64_t n, int p,
                                                     int* __restrict__ flags) {
    int bad = 0;
    const int64_t tot = n * (int64_t)(p + 1), stride = (int64_t)gridDim.x * 256;
    for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < tot; e += stride) {
        const int64_t j = e / n, i = e % n;
        const T v = j < p ? A[i + j * lda] : y[i];
        bad |= (v - v != v - v) ? 1 : 0;   // Inf or NaN
    }
    if (bad) atomicOr(&flags[3], 1);
}

// ---- host side --------------------------------------------------------------------------------------------------------
struct FltsCtx {
    Handle* h;
    int64_t n, p, lda, hh;
    const void* A;
    const void* y;
    int f32;
    int* flags;                // device: [0] more, [1] select inconsistency, [2] h mismatch, [3] non-finite
    FltsSel* sel;
    unsigned* hist;
    u128* cand;
    unsigned* ccount;
    u128* cut;
    double* part;
    size_t part_bytes;
    double* mom;
    double* Vs;
    int64_t passes = 0;
};

inline int64_t chunks_for(int64_t n, int64_t blocks_y, int64_t min_rows) {
    int64_t c = (2048 + blocks_y - 1) / blocks_y;
    const int64_t cmax = (n + min_rows - 1) / min_rows;
    if (c > cmax) c = cmax;
    return c < 1 ? 1 : c;
}

template <typename T>
int flts_cstep(FltsCtx& c, int nslots, const double* th_old, double* th_new, double* Qout) {
    Handle* h = c.h;
    const T* A = (const T*)c.A;
    const T* y = (const T*)c.y;
    const int p = (int)c.p;
    const int64_t n = c.n;
    const int by = (nslots + kSB - 1) / kSB;
    hipLaunchKernelGGL(k_flts_sel_init<T>, dim3((nslots + 255) / 256), dim3(256), 0, h->stream, c.sel, nslots, n, c.hh);
    TLSQ_HIP(h, hipGetLastError());
    const int64_t kc = chunks_for(n, by, 4096);
    const int64_t rpc = (n + kc - 1) / kc;
    if (n > kCap) {
        for (int pass = 0; pass < 16; ++pass) {
            TLSQ_HIP(h, hipMemsetAsync(c.flags, 0, 4, h->stream));
            hipLaunchKernelGGL(k_flts_hist<T>, dim3((unsigned)kc, (unsigned)by), dim3(256), 0, h->stream, A, c.lda, y, n, p, th_old,
                               nslots, c.sel, c.hist, rpc);
            hipLaunchKernelGGL(k_flts_pick, dim3((nslots + 63) / 64), dim3(64), 0, h->stream, c.hist, c.sel, nslots, c.flags);
            TLSQ_HIP(h, hipGetLastError());
            int more = 0;
            TLSQ_HIP(h, hipMemcpyAsync(&more, c.flags, 4, hipMemcpyDeviceToHost, h->stream));
            TLSQ_HIP(h, hipStreamSynchronize(h->stream));
            ++c.passes;
            if (!more) break;
        }
    }
    TLSQ_HIP(h, hipMemsetAsync(c.ccount, 0, (size_t)nslots * 4, h->stream));
    hipLaunchKernelGGL(k_flts_gather<T>, dim3((unsigned)kc, (unsigned)by), dim3(256), 0, h->stream, A, c.lda, y, n, p, th_old, nslots,
                       c.sel, c.cand, c.ccount, rpc);
    hipLaunchKernelGGL(k_flts_cut, dim3((unsigned)nslots), dim3(256), 0, h->stream, c.cand, c.ccount, c.sel, c.cut, c.flags);
    TLSQ_HIP(h, hipGetLastError());
    // masked moments
    const int M = p * (p + 1) / 2 + p + 1;
    int sbm = (256 * kAcc) / M;
    sbm = sbm < 1 ? 1 : (sbm > kSB ? kSB : sbm);
    const int bym = (nslots + sbm - 1) / sbm;
    int64_t mc = chunks_for(n, bym, 8 * kTileR);
    const size_t per_chunk = (size_t)nslots * M * 8;
    if ((size_t)mc * per_chunk > c.part_bytes) mc = (int64_t)(c.part_bytes / per_chunk);
    if (mc < 1) mc = 1;
    const int64_t mrpc = (n + mc - 1) / mc;
    hipLaunchKernelGGL(k_flts_moments<T>, dim3((unsigned)mc, (unsigned)bym), dim3(256), 0, h->stream, A, c.lda, y, n, p, th_old, nslots,
                       sbm, c.cut, c.part, mrpc, M);
    const int64_t stride = (int64_t)nslots * M;
    hipLaunchKernelGGL(k_flts_reduce, dim3((unsigned)((stride + 255) / 256)), dim3(256), 0, h->stream, c.part, stride, (int)mc, c.mom);
    hipLaunchKernelGGL(k_flts_solve, dim3((unsigned)nslots), dim3(64), 0, h->stream, c.mom, M, p, c.hh, c.Vs, th_new, c.flags);
    TLSQ_HIP(h, hipGetLastError());
    if (Qout) {
        hipLaunchKernelGGL(k_flts_q<T>, dim3((unsigned)kc, (unsigned)by), dim3(256), 0, h->stream, A, c.lda, y, n, p, th_old, th_new,
                           nslots, c.cut, c.part, rpc);
        hipLaunchKernelGGL(k_flts_reduce, dim3((unsigned)((nslots + 255) / 256)), dim3(256), 0, h->stream, c.part, (int64_t)nslots,
                           (int)kc, Qout);
        TLSQ_HIP(h, hipGetLastError());
    }
    return TLSQ_OK;
}

template <typename T>
int flts_entry(tlsq_handle hd, const T* A, int64_t n, int64_t p, int64_t ldA, const T* y, int64_t ny, const tlsq_flts_opts* opts,
               T* theta, int64_t* Hout, double* Qout, tlsq_flts_info* info) {
    TLSQ_TRY(check_handle(hd));
    Handle* h = hd;
    tlsq_flts_opts o;
    if (opts) o = *opts; else tlsq_flts_opts_default(&o);
    if (!A || !y || !theta || n < 1 || p < 1 || ldA < n)
        return set_err(h, TLSQ_ERR_ARG, "flts: bad argument (NULL pointer or size)");
    if (ny != n) return set_err(h, TLSQ_ERR_ARG, "DimensionMismatch: Both inputs A and y should have the same number of rows");
    if (o.nsub < 10) return set_err(h, TLSQ_ERR_ARG, "DomainError: N needs to be >= 10");
    if (o.maxiter < 1) return set_err(h, TLSQ_ERR_ARG, "flts: maxiter must be >= 1 (the reference's optimize_H leaves `opt` undefined)");
    if (p > kMaxP) return set_err(h, TLSQ_ERR_UNSUPPORTED, "flts: p = %lld regressors, at most %d supported", (long long)p, kMaxP);
    if (n >= ((int64_t)1 << 31)) return set_err(h, TLSQ_ERR_UNSUPPORTED, "flts: n must be below 2^31");
    if (o.nsub > ((int64_t)1 << 24)) return set_err(h, TLSQ_ERR_UNSUPPORTED, "flts: N too large");
    int64_t hh = 0;
    if (tlsq_flts_resolve_h(n, p, o.h, o.outliers, &hh) < 0) return set_err(h, TLSQ_ERR_ARG, "flts: bad argument");
    if (p > n) return set_err(h, TLSQ_ERR_ARG, "flts: p = %lld regressors but only n = %lld rows", (long long)p, (long long)n);
    if (hh > n || hh < 1)
        return set_err(h, TLSQ_ERR_ARG, "BoundsError: h = %lld outside 1:%lld (n too small for p = %lld)", (long long)hh,
                       (long long)n, (long long)p);
    const bool dev = o.memory == TLSQ_MEM_DEVICE;
    const int N = (int)o.nsub;
    TLSQ_HIP(h, hipSetDevice(h->device));
    const double t0 = now_ms();
    FltsCtx c;
    c.h = h;
    c.n = n;
    c.p = p;
    c.hh = hh;
    c.f32 = std::is_same<T, float>::value ? 1 : 0;
    void* q;
    // the data: device pointers are used in place; host arrays are uploaded (contiguous)
    if (dev) {
        c.A = A;
        c.y = y;
        c.lda = ldA;
    } else {
        TLSQ_TRY(ws_get(h, WS_FL_A, (size_t)n * p * sizeof(T), &q));
        TLSQ_TRY(copy2d(h, q, n, A, ldA, n, p, sizeof(T), hipMemcpyHostToDevice));
        c.A = q;
        c.lda = n;
        TLSQ_TRY(ws_get(h, WS_FL_Y, (size_t)n * sizeof(T), &q));
        TLSQ_HIP(h, hipMemcpyAsync(q, y, (size_t)n * sizeof(T), hipMemcpyHostToDevice, h->stream));
        c.y = q;
    }
    const T* dA = (const T*)c.A;
    const T* dy = (const T*)c.y;
    // small buffers
    TLSQ_TRY(ws_get(h, WS_FL_MISC, 64 + (size_t)N * (8 + 4 + 8 + 8) + 64 * 8, &q));
    c.flags = (int*)q;
    int64_t* rows_d = (int64_t*)((char*)q + 64);
    int* status_d = (int*)(rows_d + N);
    double* Q2_d = (double*)((char*)status_d + (((size_t)N * 4 + 7) & ~(size_t)7));
    int64_t* order_d = (int64_t*)(Q2_d + N);
    double* Q3_d = (double*)(order_d + N);   // 10 (+ room)
    TLSQ_HIP(h, hipMemsetAsync(c.flags, 0, 64, h->stream));
    hipLaunchKernelGGL(k_flts_finite<T>, dim3(1024), dim3(256), 0, h->stream, dA, c.lda, dy, n, (int)p, c.flags);
    TLSQ_HIP(h, hipGetLastError());
    int hflags[4] = {0, 0, 0, 0};
    TLSQ_HIP(h, hipMemcpyAsync(hflags, c.flags, 16, hipMemcpyDeviceToHost, h->stream));
    TLSQ_HIP(h, hipStreamSynchronize(h->stream));
    if (hflags[3]) return set_err(h, TLSQ_ERR_NONFINITE, "flts: A or y contains Infs or NaNs");
    // theta buffers: stage 0 (theta_J), 1, 2 for all subsets, then the candidates' old / new
    TLSQ_TRY(ws_get(h, WS_FL_TH, (size_t)(3 * N + 40) * p * 8, &q));
    double* th0 = (double*)q;
    double* th1 = th0 + (size_t)N * p;
    double* th2 = th1 + (size_t)N * p;
    double* thc = th2 + (size_t)N * p;        // 10 candidates: theta_2
    double* th3 = thc + (size_t)10 * p;       // their theta_3
    // ---- initial subsets (:70-71)
    std::vector<int64_t> rows((size_t)N);
    std::vector<int> status((size_t)N);
    {
        int64_t cap = std::min<int64_t>(n, std::max<int64_t>(4 * p, 64));
        std::vector<int64_t> todo((size_t)N);
        std::iota(todo.begin(), todo.end(), 0);
        int64_t first = 0, count = N;
        while (true) {
            const size_t per = (size_t)cap * p * 8 + (size_t)p * p * 8 + (size_t)cap * 16;
            const int64_t batch = std::max<int64_t>(1, std::min<int64_t>(count, (int64_t)((size_t)256 << 20) / (int64_t)per));
            TLSQ_TRY(ws_get(h, WS_FL_INIT, per * (size_t)batch, &q));
            double* Wb = (double*)q;
            double* Vb = Wb + (size_t)batch * cap * p;
            int64_t* Jb = (int64_t*)(Vb + (size_t)batch * p * p);
            double* yb = (double*)(Jb + (size_t)batch * cap);
            for (int64_t b0 = first; b0 < first + count; b0 += batch) {
                const int64_t nb = std::min<int64_t>(batch, first + count - b0);
                hipLaunchKernelGGL(k_flts_init<T>, dim3((unsigned)nb), dim3(64), 0, h->stream, dA, c.lda, dy, n, (int)p, o.seed, b0,
                                   b0 + nb, cap, Wb, Vb, Jb, yb, th0, rows_d, status_d);
                TLSQ_HIP(h, hipGetLastError());
            }
            TLSQ_HIP(h, hipMemcpyAsync(status.data(), status_d, (size_t)N * 4, hipMemcpyDeviceToHost, h->stream));
            TLSQ_HIP(h, hipStreamSynchronize(h->stream));
            // subsets whose draw outgrew the scratch start over with a larger one (the draws are counter based: same result)
            int64_t lo = -1, hi = -1;
            for (int64_t s = 0; s < N; ++s)
                if (status[(size_t)s] == 1) {
                    if (lo < 0) lo = s;
                    hi = s;
                }
            if (lo < 0) break;
            if (cap >= n) return set_err(h, TLSQ_ERR_HIP, "flts: initial subset scratch inconsistency");
            cap = std::min<int64_t>(n, cap * 4);
            first = lo;
            count = hi - lo + 1;
        }
        for (int64_t s = 0; s < N; ++s)
            if (status[(size_t)s] == 2)
                return set_err(h, TLSQ_ERR_ARG, "SingularException: the square p-subset %lld is singular (n <= p + 2 leaves no room to "
                                                "redraw it)", (long long)s);
        TLSQ_HIP(h, hipMemcpyAsync(rows.data(), rows_d, (size_t)N * 8, hipMemcpyDeviceToHost, h->stream));
    }
    // ---- C-step buffers
    TLSQ_TRY(ws_get(h, WS_FL_SEL, (size_t)N * sizeof(FltsSel) + (size_t)N * 16 + (size_t)N * 4 + 64, &q));
    c.sel = (FltsSel*)q;
    c.cut = (u128*)((char*)q + (size_t)N * sizeof(FltsSel));
    c.ccount = (unsigned*)((char*)c.cut + (size_t)N * 16);
    TLSQ_TRY(ws_get(h, WS_FL_HIST, (size_t)N * kNB * 4, &q));
    c.hist = (unsigned*)q;
    TLSQ_HIP(h, hipMemsetAsync(c.hist, 0, (size_t)N * kNB * 4, h->stream));
    TLSQ_TRY(ws_get(h, WS_FL_CAND, (size_t)N * kCap * 16, &q));
    c.cand = (u128*)q;
    const int M = (int)(p * (p + 1) / 2 + p + 1);
    c.part_bytes = std::max<size_t>((size_t)N * M * 8 * 4, (size_t)128 << 20);
    c.part_bytes = std::max(c.part_bytes, (size_t)N * 8 * 2048);   // Q partials
    TLSQ_TRY(ws_get(h, WS_FL_PART, c.part_bytes, &q));
    c.part = (double*)q;
    TLSQ_TRY(ws_get(h, WS_FL_MOM, (size_t)N * M * 8 + (size_t)N * p * p * 8, &q));
    c.mom = (double*)q;
    c.Vs = c.mom + (size_t)N * M;
    // ---- stage 1 (:71, the C-step of get_initial_H) and stage 2 (:73: optimize_H with maxiter 2 = one more C-step)
    TLSQ_TRY(flts_cstep<T>(c, N, th0, th1, nullptr));
    TLSQ_TRY(flts_cstep<T>(c, N, th1, th2, Q2_d));
    // ---- the 10 best in stable order (:74-75), a third C-step (:79), the winner (:80-83)
    hipLaunchKernelGGL(k_flts_rank, dim3((N + 255) / 256), dim3(256), 0, h->stream, Q2_d, N, order_d);
    hipLaunchKernelGGL(k_flts_take, dim3((10 * (int)p + 255) / 256), dim3(256), 0, h->stream, th2, order_d, 10, (int)p, thc);
    TLSQ_HIP(h, hipGetLastError());
    TLSQ_TRY(flts_cstep<T>(c, 10, thc, th3, Q3_d));
    int64_t cand[10];
    double q3[10];
    std::vector<double> th3h((size_t)10 * p);
    TLSQ_HIP(h, hipMemcpyAsync(cand, order_d, 80, hipMemcpyDeviceToHost, h->stream));
    TLSQ_HIP(h, hipMemcpyAsync(q3, Q3_d, 80, hipMemcpyDeviceToHost, h->stream));
    TLSQ_HIP(h, hipMemcpyAsync(th3h.data(), th3, (size_t)10 * p * 8, hipMemcpyDeviceToHost, h->stream));
    TLSQ_HIP(h, hipMemcpyAsync(hflags, c.flags, 16, hipMemcpyDeviceToHost, h->stream));
    TLSQ_HIP(h, hipStreamSynchronize(h->stream));
    if (hflags[1]) return set_err(h, TLSQ_ERR_HIP, "flts: radix select inconsistency (%d)", hflags[1]);
    int w = 0;   // sort!(results, by = Q) is stable: the first of the smallest
    for (int k = 1; k < 10; ++k) {
        auto key = [](double v) { return v != v ? std::numeric_limits<double>::infinity() : v; };
        if (key(q3[k]) < key(q3[w]) || (q3[w] != q3[w] && q3[k] == q3[k])) w = k;
    }
    // ---- outputs
    if (std::is_same<T, double>::value) {
        if (dev) TLSQ_HIP(h, hipMemcpy(theta, th3h.data() + (size_t)w * p, (size_t)p * 8, hipMemcpyHostToDevice));
        else memcpy(theta, th3h.data() + (size_t)w * p, (size_t)p * 8);
    } else {
        std::vector<T> tf((size_t)p);
        for (int64_t j = 0; j < p; ++j) tf[(size_t)j] = (T)th3h[(size_t)w * p + j];
        if (dev) TLSQ_HIP(h, hipMemcpy(theta, tf.data(), (size_t)p * sizeof(T), hipMemcpyHostToDevice));
        else memcpy(theta, tf.data(), (size_t)p * sizeof(T));
    }
    if (Qout) {
        if (dev) TLSQ_HIP(h, hipMemcpy(Qout, &q3[w], 8, hipMemcpyHostToDevice));
        else *Qout = q3[w];
    }
    if (Hout) {
        // sortperm(abs.(A theta_2 - y))[1:h] of the winner: a stable radix sort of (|r| bits, row) in row order
        const size_t nn = (size_t)n;
        size_t tmp_bytes = 0;
        TLSQ_HIP(h, rocprim::radix_sort_pairs(nullptr, tmp_bytes, (unsigned long long*)nullptr, (unsigned long long*)nullptr,
                                              (unsigned*)nullptr, (unsigned*)nullptr, nn, 0, c.f32 ? 32 : 64, h->stream));
        TLSQ_TRY(ws_get(h, WS_FL_SORT, nn * 24 + tmp_bytes + 256 + nn * 8, &q));
        unsigned long long* k0 = (unsigned long long*)q;
        unsigned long long* k1 = k0 + nn;
        unsigned* i0 = (unsigned*)(k1 + nn);
        unsigned* i1 = i0 + nn;
        int64_t* H64 = (int64_t*)(((uintptr_t)(i1 + nn) + 255) & ~(uintptr_t)255);
        void* tmp = (void*)(H64 + nn);
        hipLaunchKernelGGL(k_flts_hkeys<T>, dim3((unsigned)std::min<int64_t>((n + 255) / 256, 4096)), dim3(256), 0, h->stream, dA, c.lda,
                           dy, n, (int)p, thc + (size_t)w * p, k0, i0);
        TLSQ_HIP(h, hipGetLastError());
        TLSQ_HIP(h, rocprim::radix_sort_pairs(tmp, tmp_bytes, k0, k1, i0, i1, nn, 0, c.f32 ? 32 : 64, h->stream));
        std::vector<unsigned> hi((size_t)hh);
        TLSQ_HIP(h, hipMemcpyAsync(hi.data(), i1, (size_t)hh * 4, hipMemcpyDeviceToHost, h->stream));
        TLSQ_HIP(h, hipStreamSynchronize(h->stream));
        std::vector<int64_t> H((size_t)hh);
        for (int64_t i = 0; i < hh; ++i) H[(size_t)i] = (int64_t)hi[(size_t)i];
        if (dev) TLSQ_HIP(h, hipMemcpy(Hout, H.data(), (size_t)hh * 8, hipMemcpyHostToDevice));
        else memcpy(Hout, H.data(), (size_t)hh * 8);
    }
    if (info) {
        info->h = hh;
        info->p = p;
        info->winner = cand[w];
        int64_t ext = 0, mx = 0;
        for (int64_t s = 0; s < N; ++s) {
            ext += rows[(size_t)s] > p ? 1 : 0;
            mx = std::max(mx, rows[(size_t)s]);
        }
        info->rank_extended_draws = ext;
        info->max_subset_rows = mx;
        info->csteps_done = 2 * (int64_t)N + 10;
        info->h_mismatch = hflags[2];
        info->select_passes = c.passes;
        info->chance = (1.0 - std::pow(1.0 - std::pow((double)hh / (double)n, (double)p), (double)N)) * 100.0;
        if (info->subset_rows) memcpy(info->subset_rows, rows.data(), (size_t)N * 8);
        if (info->q_stage2) TLSQ_HIP(h, hipMemcpy(info->q_stage2, Q2_d, (size_t)N * 8, hipMemcpyDeviceToHost));
        if (info->candidates) memcpy(info->candidates, cand, 80);
        if (info->q_final) memcpy(info->q_final, q3, 80);
        info->ms_total = now_ms() - t0;
    }
    return TLSQ_OK;
}

}  // namespace

}  // namespace tlsq

using namespace tlsq;

extern "C" {

void tlsq_flts_opts_default(tlsq_flts_opts* o) {
    if (!o) return;
    memset(o, 0, sizeof(*o));
    o->h = 0;
    o->outliers = -1.0;
    o->nsub = 500;
    o->maxiter = 100;
    o->memory = TLSQ_MEM_HOST;
    o->dQmin = 1e-4;
    o->seed = 0;
}

int tlsq_flts_resolve_h(int64_t n, int64_t p, int64_t h, double outliers, int64_t* h_out) {
    if (n < 1 || p < 1 || !h_out) return TLSQ_ERR_ARG;
    const double dflt = std::nearbyint(0.5 * (double)(n + p + 1));   // round(0.5(n + p + 1)), ties to even
    if (dflt <= (double)h && h <= n) {
        *h_out = h;
        return 0;
    }
    if (0.0 <= outliers && outliers <= 0.5) {
        *h_out = (int64_t)std::nearbyint((1.0 - outliers) * (double)n);
        return 1;
    }
    *h_out = (int64_t)dflt;
    return 2;
}

int tlsq_flts_subset(uint64_t seed, int64_t s, int32_t attempt, int64_t n, int64_t k, int64_t* J) {
    if (!J || n < 1 || k < 0 || k > n || s < 0 || attempt < 0) return TLSQ_ERR_ARG;
    flts_draw(seed, s, attempt, n, k, J);
    return TLSQ_OK;
}

int tlsq_flts_f64(tlsq_handle h, const double* A, int64_t n, int64_t p, int64_t ldA, const double* y, int64_t ny,
                  const tlsq_flts_opts* opts, double* theta, int64_t* H, double* Q, tlsq_flts_info* info) {
    return flts_entry<double>(h, A, n, p, ldA, y, ny, opts, theta, H, Q, info);
}

int tlsq_flts_f32(tlsq_handle h, const float* A, int64_t n, int64_t p, int64_t ldA, const float* y, int64_t ny,
                  const tlsq_flts_opts* opts, float* theta, int64_t* H, double* Q, tlsq_flts_info* info) {
    return flts_entry<float>(h, A, n, p, ldA, y, ny, opts, theta, H, Q, info);
}

}  // extern "C"
