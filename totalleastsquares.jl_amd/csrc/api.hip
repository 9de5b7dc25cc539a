// C ABI of include/tlsq.h (everything except the handle / communicator entry points, which live in runtime.hip):
// argument checks, staging between caller memory and the device workspace, and the calls into solver.hip and the
// kernel launchers.  lowrankfilter (src/robustPCA.jl:119-128), tls!/rtls (src/TotalLeastSquares.jl:63-69,152-156),
// the Hankel family, the batched and complex entry points, and the kernel-level entry points used by the tests.
#include <dlfcn.h>
#include <rccl/rccl.h>

#include <algorithm>
#include <chrono>
#include <cstdlib>
#include <cmath>
#include <limits>
#include <numeric>

#include "internal.hpp"

using namespace tlsq;

// ---- Hankel family ------------------------------------------------------------------------------
template <typename T>
static int hankel_impl(tlsq_handle h, const T* x, int64_t Nx, int64_t Dch, int64_t ldx, int64_t L,
                       int64_t lag, T* X, int64_t ldX, int memory) {
    TLSQ_TRY(check_handle(h));
    if (!x || !X || Nx <= 0 || Dch <= 0 || L <= 0 || lag <= 0 || ldx < Nx)
        return set_err(h, TLSQ_ERR_ARG, "hankel: bad argument");
    if (!(2 * L <= Nx))  // @assert L <= N/2   src/robustPCA.jl:79
        return set_err(h, TLSQ_ERR_ARG, "L has to be less than N/2 = %g", Nx / 2.0);
    if (!(lag <= L))     // @assert lag <= L   src/robustPCA.jl:80
        return set_err(h, TLSQ_ERR_ARG, "lag must be <= L");
    const int64_t K = (Nx - L) / lag + 1;
    if (ldX < K) return set_err(h, TLSQ_ERR_ARG, "hankel: ldX < K");
    TLSQ_HIP(h, hipSetDevice(h->device));
    if (memory == TLSQ_MEM_DEVICE) {
        TLSQ_TRY(launch_hankel<T>(h, x, Nx, Dch, ldx, L, lag, X, ldX));
        TLSQ_HIP(h, hipStreamSynchronize(h->stream));
        return TLSQ_OK;
    }
    void *dx, *dX;
    TLSQ_TRY(ws_get(h, WS_AUX3, (size_t)Nx * Dch * sizeof(T), &dx));
    TLSQ_TRY(ws_get(h, WS_D, (size_t)K * L * Dch * sizeof(T), &dX));
    TLSQ_TRY(copy2d(h, dx, Nx, x, ldx, Nx, Dch, sizeof(T), hipMemcpyHostToDevice));
    TLSQ_TRY(launch_hankel<T>(h, (const T*)dx, Nx, Dch, Nx, L, lag, (T*)dX, K));
    TLSQ_TRY(copy2d(h, X, ldX, dX, K, K, L * Dch, sizeof(T), hipMemcpyDeviceToHost));
    TLSQ_HIP(h, hipStreamSynchronize(h->stream));
    return TLSQ_OK;
}

template <typename T>
static int unhankel_impl(tlsq_handle h, const T* A, int64_t K, int64_t LD, int64_t ldA, int64_t lag,
                         int64_t Nx, int64_t Dch, T* y, int64_t ldy, int memory) {
    TLSQ_TRY(check_handle(h));
    if (!A || !y || K <= 0 || LD <= 0 || Dch <= 0 || lag <= 0 || ldA < K || Nx <= 0 || ldy < Nx ||
        LD % Dch != 0)
        return set_err(h, TLSQ_ERR_ARG, "unhankel: bad argument");
    const int64_t L = LD / Dch;
    TLSQ_HIP(h, hipSetDevice(h->device));
    if (memory == TLSQ_MEM_DEVICE) {
        TLSQ_TRY(launch_unhankel<T>(h, A, K, L, Dch, ldA, lag, Nx, y, ldy));
        TLSQ_HIP(h, hipStreamSynchronize(h->stream));
        return TLSQ_OK;
    }
    void *dA, *dy;
    TLSQ_TRY(ws_get(h, WS_A, (size_t)K * LD * sizeof(T), &dA));
    TLSQ_TRY(ws_get(h, WS_AUX3, (size_t)Nx * Dch * sizeof(T), &dy));
    TLSQ_TRY(copy2d(h, dA, K, A, ldA, K, LD, sizeof(T), hipMemcpyHostToDevice));
    TLSQ_TRY(launch_unhankel<T>(h, (const T*)dA, K, L, Dch, K, lag, Nx, (T*)dy, Nx));
    TLSQ_TRY(copy2d(h, y, ldy, dy, Nx, Nx, Dch, sizeof(T), hipMemcpyDeviceToHost));
    TLSQ_HIP(h, hipStreamSynchronize(h->stream));
    return TLSQ_OK;
}

template <typename T>
static int soft_hankel_impl(tlsq_handle h, T* A, int64_t K, int64_t L, int64_t ldA, T eps, int memory) {
    TLSQ_TRY(check_handle(h));
    if (!A || K <= 0 || L <= 0 || ldA < K) return set_err(h, TLSQ_ERR_ARG, "soft_hankel: bad argument");
    TLSQ_HIP(h, hipSetDevice(h->device));
    void* mws;
    TLSQ_TRY(ws_get(h, WS_AUX1, (size_t)(K + L) * sizeof(T), &mws));
    if (memory == TLSQ_MEM_DEVICE) {
        TLSQ_TRY(launch_soft_hankel<T>(h, A, K, L, ldA, eps, (T*)mws));
        TLSQ_HIP(h, hipStreamSynchronize(h->stream));
        return TLSQ_OK;
    }
    void* dA;
    TLSQ_TRY(ws_get(h, WS_A, (size_t)K * L * sizeof(T), &dA));
    TLSQ_TRY(copy2d(h, dA, K, A, ldA, K, L, sizeof(T), hipMemcpyHostToDevice));
    TLSQ_TRY(launch_soft_hankel<T>(h, (T*)dA, K, L, K, eps, (T*)mws));
    TLSQ_TRY(copy2d(h, A, ldA, dA, K, K, L, sizeof(T), hipMemcpyDeviceToHost));
    TLSQ_HIP(h, hipStreamSynchronize(h->stream));
    return TLSQ_OK;
}


// ---- lowrankfilter: src/robustPCA.jl:119-128 (fp64 and fp32) ------------------------------------------------------
template <typename T>
static int lowrankfilter_impl(tlsq_handle h, const T* y, int64_t Nx, int64_t Dch, int64_t ldy, int64_t n, int64_t lag,
                              int64_t sv, const tlsq_rpca_opts* opts, T* yf, int64_t ldyf, tlsq_rpca_info* info) {
    constexpr size_t ES = sizeof(T);
    TLSQ_TRY(check_handle(h));
    if (!y || !yf || Nx <= 0 || Dch <= 0 || ldy < Nx || ldyf < Nx)
        return set_err(h, TLSQ_ERR_ARG, "lowrankfilter: bad argument");
    if (n <= 0) n = std::min<int64_t>(Nx / 20, 2000);  // :119
    if (lag <= 0) lag = 1;
    if (!(2 * n <= Nx)) return set_err(h, TLSQ_ERR_ARG, "L has to be less than N/2 = %g", Nx / 2.0);
    if (!(lag <= n)) return set_err(h, TLSQ_ERR_ARG, "lag must be <= L");
    if (is_multi_call(h)) {
        // single-process multi-GPU group: every rank receives the whole series (host memory) and owns a block of the
        // Hankel rows; ranks > 0 write their (identical) filtered series to scratch.  What the sharded form does not
        // cover (plain SSA truncation, short series) runs on the first GPU alone.
        const bool dev_mem = opts && opts->memory == TLSQ_MEM_DEVICE;
        if (dev_mem) return set_err(h, TLSQ_ERR_UNSUPPORTED, "lowrankfilter: a multi-GPU handle takes host vectors");
        const int64_t Kall = (Nx - n) / lag + 1;
        const bool hook_cb = opts && (opts->svd_mode == TLSQ_SVD_CALLBACK || opts->opnorm_mode == TLSQ_OPNORM_CALLBACK);
        if (sv <= 0 && !hook_cb && Kall >= 64 * (int64_t)h->multi_n) {
            const int nr = h->multi_n;
            std::vector<std::vector<T>> scratch((size_t)nr);
            std::vector<tlsq_rpca_info> ri((size_t)nr);
            std::vector<tlsq_rpca_opts> ro((size_t)nr);
            std::vector<std::vector<double>> chv((size_t)nr);
            std::vector<std::vector<int64_t>> shv((size_t)nr);
            for (int r = 0; r < nr; ++r) {
                if (opts) ro[(size_t)r] = *opts; else tlsq_rpca_opts_default(&ro[(size_t)r]);
                ro[(size_t)r].memory = TLSQ_MEM_HOST;
                memset(&ri[(size_t)r], 0, sizeof(tlsq_rpca_info));
                if (r == 0) {
                    if (info) ri[0] = *info;
                    continue;
                }
                scratch[(size_t)r].resize((size_t)Nx * Dch);
                if (ro[(size_t)r].on_iter) ro[(size_t)r].on_iter = [](int64_t, double, int64_t, void*) {};
                if (info && info->cost_hist) {
                    chv[(size_t)r].resize((size_t)std::max<int64_t>(info->hist_capacity, 1));
                    ri[(size_t)r].cost_hist = chv[(size_t)r].data();
                }
                if (info && info->svp_hist) {
                    shv[(size_t)r].resize((size_t)std::max<int64_t>(info->hist_capacity, 1));
                    ri[(size_t)r].svp_hist = shv[(size_t)r].data();
                }
                ri[(size_t)r].hist_capacity = info ? info->hist_capacity : 0;
            }
            const int st = multi_run(h, [&](Handle* hr, int r, int) -> int {
                return lowrankfilter_impl<T>(static_cast<tlsq_handle>(hr), y, Nx, Dch, ldy, n, lag, sv, &ro[(size_t)r],
                                             r == 0 ? yf : scratch[(size_t)r].data(), r == 0 ? ldyf : Nx, &ri[(size_t)r]);
            });
            if (info) *info = ri[0];
            return st;
        }
    }
    TLSQ_HIP(h, hipSetDevice(h->device));
    if (info) {
        double* ch = info->cost_hist;
        int64_t* sh = info->svp_hist;
        int64_t cap = info->hist_capacity;
        memset(info, 0, sizeof(*info));
        info->cost_hist = ch;
        info->svp_hist = sh;
        info->hist_capacity = cap;
    }
    h->kern_hankel_gram = 0;
    const double t0 = now_ms();
    const bool dev = opts && opts->memory == TLSQ_MEM_DEVICE;
    const int64_t Kg = (Nx - n) / lag + 1, LD = n * Dch;   // rows of the whole Hankel matrix
    // With a communicator every rank passes the WHOLE series and owns a contiguous block of the rows of H, i.e. a time
    // window of y with an (n-1)-sample halo: rows [r0, r1) use the samples [r0*lag, (r1-1)*lag + n).
    const bool sharded = h->comm != nullptr;
    int64_t r0 = 0, r1 = Kg;
    if (sharded) {
        const int64_t base = Kg / h->nranks, rem = Kg % h->nranks;
        r0 = h->rank * base + std::min<int64_t>(h->rank, rem);
        r1 = r0 + base + (h->rank < rem ? 1 : 0);
        if (r1 <= r0) return set_err(h, TLSQ_ERR_ARG, "lowrankfilter: fewer Hankel rows (%lld) than ranks", (long long)Kg);
    }
    const int64_t K = r1 - r0, s0 = r0 * lag, Nw = (K - 1) * lag + n;   // local rows, window start and length
    // zero pad rows up to a multiple of 16 so that every panel column is 128-byte aligned (see rpca_entry); the
    // hankel option of rpca works on the exact shape
    // (a caller's hook sees the panel; a wide Hankel matrix goes through rpca_entry in place: same workspace slots)
    const bool exact_shape = (opts && (opts->hankel || opts->svd_mode == TLSQ_SVD_CALLBACK ||
                                       opts->opnorm_mode == TLSQ_OPNORM_CALLBACK)) || (K < LD && !sharded);
    const int64_t Kp = exact_shape ? K : (K + 15) / 16 * 16;
    // robust mode - the Hankel matrix is never stored.  The big fused sweep, the residual and the set-up of
    // rpca_core read H[k, l Dch + d] = y[k lag + l, d] from the series (ResolvedOpts::hankel_lazy, any lag and number of
    // channels: src/robustPCA.jl:81-90 is arithmetic indexing): seven resident panels instead of eight, six panel passes per
    // iteration instead of seven.
    const bool implicit_ok = !dev_is(DEV_IMPLICIT_HANKEL, '0');
    const bool lazy_ok = !dev_is(DEV_LAZY_HANKEL, '0');
    const bool implicit = implicit_ok && LD <= 65535;
    const bool lazy = implicit && lazy_ok && sv <= 0 && !exact_shape;
    // ... and neither is A (one channel, lag 1): the loop keeps it in factors, the anti-diagonal means are taken from them
    // (unhankel_factors), and the panel only exists if some iteration needed it in memory (rank above 32): four resident
    // panels (E, Y, Z, R)
    const bool factors_out = lazy && !sharded && Dch == 1 && lag == 1 && (size_t)n * 32 * 8 <= 64 * 1024;
    // The plain truncation branch (sv > 0, :123-126) on the series itself (round 6, hankelop.hip): the Gram matrix of H from n
    // lagged autocorrelation sums, the factor H V[:, 1:sv] as sv FIR filters, the anti-diagonal means from the factors - neither H
    // nor A is ever stored (one channel, lag 1, one GPU; otherwise the panels as before).  HANKEL_STRUCT=0: the panel form.
    const int64_t r_sv = std::min<int64_t>(sv, std::min(Kg, LD));
    const bool structured = sv > 0 && !sharded && Dch == 1 && lag == 1 && hankel_structured_ok(K, n, r_sv) &&
                            (size_t)n * (size_t)r_sv * 8 <= 64 * 1024 && !dev_is(DEV_HANKEL_STRUCT, '0');
    void *dy, *H = nullptr, *A = nullptr, *E;
    TLSQ_TRY(ws_get(h, WS_AUX3, (size_t)Nx * Dch * ES, &dy));
    if (!lazy && !structured) TLSQ_TRY(ws_get(h, WS_D, (size_t)Kp * LD * ES, &H));
    if (!factors_out && !structured) TLSQ_TRY(ws_get(h, WS_A, (size_t)Kp * LD * ES, &A));
    if (!lazy && !structured && Kp != K) TLSQ_HIP(h, hipMemsetAsync(H, 0, (size_t)Kp * LD * ES, h->stream));
    TLSQ_TRY(copy2d(h, dy, Nx, y, ldy, Nx, Dch, ES, dev ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice));
    const T* yw = (const T*)dy + s0;                                                // this rank's window
    if (!lazy && !structured) TLSQ_TRY(launch_hankel<T>(h, yw, Nw, Dch, Nx, n, lag, (T*)H, Kp));     // :120
    int status = TLSQ_OK;
    if (sv <= 0) {                                                                            // :121-122
        TLSQ_TRY(ws_get(h, WS_E, (size_t)Kp * LD * ES, &E));
        tlsq_rpca_opts oo;
        if (opts) oo = *opts; else tlsq_rpca_opts_default(&oo);
        oo.m_global = Kg;
        ResolvedOpts ro = resolve(&oo, K, LD, 1e-3);  // tol defaults to 1e-3 here (:119)
        ro.m_global = Kg;
        if (implicit) {
            ro.hankel_y = yw;
            ro.hankel_K = K;
            ro.hankel_geom.lag = (int32_t)lag;
            ro.hankel_geom.Dch = (int32_t)Dch;
            ro.hankel_geom.ldx = Nx;
            ro.hankel_lazy = lazy;
            ro.factors_out = factors_out;
        }
        if (std::min(Kg, LD) > kGramMaxN)
            return set_err(h, TLSQ_ERR_UNSUPPORTED, "lowrankfilter: min(K, n*D) = %lld exceeds %lld, the largest Gram "
                           "dimension of this release", (long long)std::min(Kg, LD), (long long)kGramMaxN);
        if (K < LD && !sharded) {
            // a wide Hankel matrix (several channels / lag > 1 with a long window): the Gram of the panel would be
            // structurally rank deficient - go through the general entry, which solves the transposed problem
            oo.memory = TLSQ_MEM_DEVICE;
            tlsq_rpca_info inner;
            memset(&inner, 0, sizeof(inner));
            if (info) inner = *info;
            if (std::isnan(oo.tol)) oo.tol = 1e-3;   // the lowrankfilter default (:119)
            // (on a group handle this is the first GPU working alone on its own device panel: the general entry must not
            //  take the call for a group call with device pointers - found by tools/fuzz_lrf.py)
            const bool was_in_multi = h->in_multi;
            h->in_multi = true;
            status = rpca_entry<T>(h, (const T*)H, K, LD, Kp, &oo, (T*)A, Kp, (T*)E, Kp, nullptr, K, nullptr, nullptr,
                                   std::min(K, LD), nullptr, info ? &inner : nullptr);
            h->in_multi = was_in_multi;
            if (info) *info = inner;
        } else {
            status = rpca_core<T>(h, (const T*)H, Kp, LD, ro, &oo, (T*)A, (T*)E, nullptr, nullptr, nullptr, 0, nullptr, info);
        }
        if (status < 0) return status;
    } else if (structured) {                                                                  // :123-126, H never stored
        SmallSvd s;
        double* V = nullptr;
        int64_t sweeps = 0;
        void *G, *Vs, *Tm;
        TLSQ_TRY(ws_get(h, WS_G, (size_t)n * n * 8, &G));
        TLSQ_TRY(hankel_gram<T>(h, yw, K, n, (double*)G));
        // (only the leading sv vectors are used: the Cholesky route - zero columns for numerically zero eigenvalues - serves)
        TLSQ_TRY(eig_full(h, (const double*)G, n, &V, s, &sweeps, false, WS_V, false));
        TLSQ_TRY(ws_get(h, WS_VS, (size_t)n * r_sv * 8, &Vs));
        TLSQ_TRY(ws_get(h, WS_T, (size_t)Kp * r_sv * 8, &Tm));
        SelWeights sw;
        for (int64_t i = 0; i < 32; ++i) {
            sw.sel[i] = i < r_sv ? s.order[(size_t)i] : 0;
            sw.w[i] = 1.0;
        }
        TLSQ_TRY(launch_gather_scale_arg(h, V, n, sw, r_sv, nullptr, (double*)Vs));
        TLSQ_TRY(hankel_times<T>(h, yw, K, Kp, n, (const double*)Vs, n, r_sv, (double*)Tm, Kp));
        TLSQ_TRY(launch_unhankel_factors<T>(h, (const double*)Tm, Kp, (const double*)Vs, n, r_sv, K, n, Nx, (T*)dy));
        if (info) {
            info->jacobi_sweeps = sweeps;
            info->kern_hankel_gram = h->kern_hankel_gram;
        }
    } else {                                                                                  // :123-126
        SmallSvd s;
        double* V = nullptr;
        int64_t sweeps = 0;
        TLSQ_TRY(svd_via_gram<T>(h, (const T*)H, Kp, LD, Kp, &V, s, &sweeps, nullptr));
        const int64_t r = std::min<int64_t>(sv, std::min(Kg, LD));
        std::vector<int32_t> sel((size_t)r);
        std::vector<double> g((size_t)r, 1.0);
        for (int64_t p2 = 0; p2 < r; ++p2) sel[p2] = s.order[p2];
        TLSQ_TRY(rebuild_lowrank<T>(h, (const T*)H, Kp, LD, Kp, V, sel, g, (T*)A, Kp));
        if (info) info->jacobi_sweeps = sweeps;
    }
    // :127  (dy is reused for the filtered signal)
    if (structured) {
        // (the filtered series is in dy already)
    } else if (!sharded && factors_out && sv <= 0 && h->out_factors) {
        TLSQ_TRY(launch_unhankel_factors<T>(h, h->out_Tm, Kp, h->out_Vs, LD, h->out_r, K, n, Nx, (T*)dy));
    } else if (!sharded) {
        if (!A) A = h->ws[WS_A].p;   // (allocated inside the loop: some iteration needed the panel)
        if (!A) return set_err(h, TLSQ_ERR_UNSUPPORTED, "lowrankfilter: the low-rank panel was never formed");
        TLSQ_TRY(launch_unhankel<T>(h, (const T*)A, K, n, Dch, Kp, lag, Nx, (T*)dy, Nx));
    } else {
        // anti-diagonals that straddle a shard boundary get their partial sums and counts from both neighbours: one
        // sum all-reduce over [sums | counts], then the division; every rank ends up with the whole filtered series
        void* sc;
        const size_t nn = (size_t)Nx * Dch;
        TLSQ_TRY(ws_get(h, WS_AUX4, 2 * nn * 8, &sc));
        double* sum = (double*)sc;
        double* cnt = sum + nn;
        TLSQ_HIP(h, hipMemsetAsync(sc, 0, 2 * nn * 8, h->stream));
        TLSQ_TRY(launch_unhankel_partial<T>(h, (const T*)A, K, n, Dch, Kp, lag, Nw, s0, sum, cnt, Nx));
        TLSQ_TRY(comm_allreduce(h, sum, 2 * nn, ncclSum));
        TLSQ_TRY(launch_unhankel_finish<T>(h, sum, cnt, (int64_t)nn, (T*)dy));
    }
    TLSQ_TRY(copy2d(h, yf, ldyf, dy, Nx, Nx, Dch, ES, dev ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost));
    TLSQ_HIP(h, hipStreamSynchronize(h->stream));
    if (info) info->ms_total = now_ms() - t0;
    return status;
}

extern "C" {

int tlsq_rpca_f64(tlsq_handle h, const double* D, int64_t M, int64_t N, int64_t ldD,
                  const tlsq_rpca_opts* opts, double* A, int64_t ldA, double* E, int64_t ldE, double* U,
                  int64_t ldU, double* S, double* Vt, int64_t ldVt, int64_t* sv, tlsq_rpca_info* info) {
    TLSQ_TRY(ws_poison_all(h));
    return rpca_entry<double>(h, D, M, N, ldD, opts, A, ldA, E, ldE, U, ldU, S, Vt, ldVt, sv, info);
}

int tlsq_rpca_f32(tlsq_handle h, const float* D, int64_t M, int64_t N, int64_t ldD,
                  const tlsq_rpca_opts* opts, float* A, int64_t ldA, float* E, int64_t ldE, float* U,
                  int64_t ldU, float* S, float* Vt, int64_t ldVt, int64_t* sv, tlsq_rpca_info* info) {
    TLSQ_TRY(ws_poison_all(h));
    return rpca_entry<float>(h, D, M, N, ldD, opts, A, ldA, E, ldE, U, ldU, S, Vt, ldVt, sv, info);
}

// ---- Hankel family (templates hankel_impl/unhankel_impl/soft_hankel_impl live above extern "C") ----
int tlsq_hankel_f64(tlsq_handle h, const double* x, int64_t Nx, int64_t Dch, int64_t ldx, int64_t L,
                    int64_t lag, double* X, int64_t ldX, int memory) {
    return hankel_impl<double>(h, x, Nx, Dch, ldx, L, lag, X, ldX, memory);
}
int tlsq_hankel_f32(tlsq_handle h, const float* x, int64_t Nx, int64_t Dch, int64_t ldx, int64_t L,
                    int64_t lag, float* X, int64_t ldX, int memory) {
    return hankel_impl<float>(h, x, Nx, Dch, ldx, L, lag, X, ldX, memory);
}
int tlsq_unhankel_f64(tlsq_handle h, const double* A, int64_t K, int64_t LD, int64_t ldA, int64_t lag,
                      int64_t Nx, int64_t Dch, double* y, int64_t ldy, int memory) {
    return unhankel_impl<double>(h, A, K, LD, ldA, lag, Nx, Dch, y, ldy, memory);
}
int tlsq_unhankel_f32(tlsq_handle h, const float* A, int64_t K, int64_t LD, int64_t ldA, int64_t lag,
                      int64_t Nx, int64_t Dch, float* y, int64_t ldy, int memory) {
    return unhankel_impl<float>(h, A, K, LD, ldA, lag, Nx, Dch, y, ldy, memory);
}
int tlsq_soft_hankel_f64(tlsq_handle h, double* A, int64_t K, int64_t L, int64_t ldA, double eps,
                         int memory) {
    return soft_hankel_impl<double>(h, A, K, L, ldA, eps, memory);
}
int tlsq_soft_hankel_f32(tlsq_handle h, float* A, int64_t K, int64_t L, int64_t ldA, float eps,
                         int memory) {
    return soft_hankel_impl<float>(h, A, K, L, ldA, eps, memory);
}

// ---- lowrankfilter: src/robustPCA.jl:119-128 -----------------------------------------------------
int tlsq_lowrankfilter_f64(tlsq_handle h, const double* y, int64_t Nx, int64_t Dch, int64_t ldy, int64_t n, int64_t lag,
                           int64_t sv, const tlsq_rpca_opts* opts, double* yf, int64_t ldyf, tlsq_rpca_info* info) {
    TLSQ_TRY(ws_poison_all(h));
    return lowrankfilter_impl<double>(h, y, Nx, Dch, ldy, n, lag, sv, opts, yf, ldyf, info);
}
int tlsq_lowrankfilter_f32(tlsq_handle h, const float* y, int64_t Nx, int64_t Dch, int64_t ldy, int64_t n, int64_t lag,
                           int64_t sv, const tlsq_rpca_opts* opts, float* yf, int64_t ldyf, tlsq_rpca_info* info) {
    TLSQ_TRY(ws_poison_all(h));
    return lowrankfilter_impl<float>(h, y, Nx, Dch, ldy, n, lag, sv, opts, yf, ldyf, info);
}

// ---- tls! / rtls ---------------------------------------------------------------------------------
int tlsq_tls_from_vt_f64(const double* Vt, int64_t ncols, int64_t ldVt, int64_t n, double* x,
                         int64_t ldx) {
    if (!Vt || !x || ncols <= 0 || n <= 0 || n >= ncols || ldVt < ncols || ldx < n) return TLSQ_ERR_ARG;
    return tls_partition_solve(Vt, ncols, ldVt, n, x, ldx);
}

}  // extern "C"

// full right-singular basis of a device matrix (M x nc, ld; fp64 or fp32) as Vt on the host (nc x nc, fp64)
template <typename T>
static int vt_of(tlsq_handle h, const T* dAy, int64_t M, int64_t nc, int64_t ld, std::vector<double>& Vt) {
    SmallSvd s;
    double* V = nullptr;
    int64_t sweeps = 0;
    // TSQR route: tls! takes the right singular vectors of the SMALLEST singular values (V[:, n+1:end],
    // src/TotalLeastSquares.jl:66-68), which the Gram route only resolves to eps * cond(Ay)^2
    if (M >= nc && nc <= kFullEigMaxN && !h->comm) TLSQ_TRY(svd_via_r<T>(h, dAy, M, nc, ld, &V, s, &sweeps));
    else TLSQ_TRY(svd_via_gram<T>(h, dAy, M, nc, ld, &V, s, &sweeps, nullptr));
    std::vector<double> hv((size_t)nc * nc);
    TLSQ_HIP(h, hipMemcpyAsync(hv.data(), V, (size_t)nc * nc * 8, hipMemcpyDeviceToHost, h->stream));
    TLSQ_HIP(h, hipStreamSynchronize(h->stream));
    Vt.resize((size_t)nc * nc);
    for (int64_t p2 = 0; p2 < nc; ++p2)
        for (int64_t j = 0; j < nc; ++j) Vt[p2 + j * nc] = hv[(size_t)s.order[p2] * nc + j];
    return TLSQ_OK;
}

// x (n x q, ldx, type T) <- the fp64 solution hx (n x q, ld n), to host or device memory
template <typename T>
static int put_x(tlsq_handle h, const std::vector<double>& hx, int64_t n, int64_t q, T* x, int64_t ldx, bool dev) {
    std::vector<T> tx((size_t)n * q);
    for (size_t i = 0; i < tx.size(); ++i) tx[i] = (T)hx[i];
    if (dev) {
        TLSQ_TRY(copy2d(h, x, ldx, tx.data(), n, n, q, sizeof(T), hipMemcpyHostToDevice));
        TLSQ_HIP(h, hipStreamSynchronize(h->stream));
    } else {
        for (int64_t a = 0; a < q; ++a)
            for (int64_t i = 0; i < n; ++i) x[i + a * ldx] = tx[(size_t)(i + a * n)];
    }
    return TLSQ_OK;
}

template <typename T>
static int tls_impl(tlsq_handle h, const T* Ay, int64_t M, int64_t ncols, int64_t ldAy, int64_t n, T* x, int64_t ldx,
                    int memory) {
    TLSQ_TRY(check_handle(h));
    if (!Ay || !x || M <= 0 || ncols <= 1 || n <= 0 || n >= ncols || ldAy < M || ldx < n)
        return set_err(h, TLSQ_ERR_ARG, "tls: bad argument");
    TLSQ_HIP(h, hipSetDevice(h->device));
    const T* dAy = Ay;
    int64_t ld = ldAy;
    if (memory != TLSQ_MEM_DEVICE) {
        void* p;
        TLSQ_TRY(ws_get(h, WS_D, (size_t)M * ncols * sizeof(T), &p));
        TLSQ_TRY(copy2d(h, p, M, Ay, ldAy, M, ncols, sizeof(T), hipMemcpyHostToDevice));
        dAy = (const T*)p;
        ld = M;
    }
    // svd! of the reference goes through LAPACK's chkfinite and throws ArgumentError("matrix contains Infs or NaNs") before it
    // decomposes anything (src/TotalLeastSquares.jl:63): one max-abs pass over the panel (k_maxabs maps NaN to Inf) settles it
    // on every route - the decomposition's own NaN propagation is not a contract
    if (ld == M) {
        double mx = 0.0;
        TLSQ_TRY(launch_maxabs<T>(h, dAy, M * ncols, &mx));
        if (!std::isfinite(mx)) return set_err(h, TLSQ_ERR_NONFINITE, "matrix contains Infs or NaNs");
    } else {
        for (int64_t c = 0; c < ncols; ++c) {
            double mx = 0.0;
            TLSQ_TRY(launch_maxabs<T>(h, dAy + (size_t)c * ld, M, &mx));
            if (!std::isfinite(mx)) return set_err(h, TLSQ_ERR_NONFINITE, "matrix contains Infs or NaNs");
        }
    }
    std::vector<double> Vt;
    TLSQ_TRY(vt_of<T>(h, dAy, M, ncols, ld, Vt));
    for (double v : Vt)   // (an assertion only: finite input never gives a non-finite V)
        if (!std::isfinite(v)) return set_err(h, TLSQ_ERR_NONFINITE, "matrix contains Infs or NaNs");
    const int64_t q = ncols - n;
    std::vector<double> hx((size_t)n * q);
    const int st = tls_partition_solve(Vt.data(), ncols, ncols, n, hx.data(), n);   // :65-69
    if (st < 0) return set_err(h, st, "tls: partition solve failed");
    return put_x<T>(h, hx, n, q, x, ldx, memory == TLSQ_MEM_DEVICE);
}

template <typename T>
static int rtls_impl(tlsq_handle h, const T* A, int64_t M, int64_t n, int64_t ldA, const T* y, int64_t q, int64_t ldy,
                     const tlsq_rpca_opts* opts, T* x, int64_t ldx, tlsq_rpca_info* info) {
    TLSQ_TRY(check_handle(h));
    if (!A || !y || !x || M <= 0 || n <= 0 || q <= 0 || ldA < M || ldy < M || ldx < n)
        return set_err(h, TLSQ_ERR_ARG, "rtls: bad argument");
    TLSQ_HIP(h, hipSetDevice(h->device));
    reset_info(info);
    const bool dev = opts && opts->memory == TLSQ_MEM_DEVICE;
    const int64_t nc = n + q;
    void *AA, *Ah, *Eh;
    TLSQ_TRY(ws_get(h, WS_D, (size_t)M * nc * sizeof(T), &AA));
    TLSQ_TRY(ws_get(h, WS_A, (size_t)M * nc * sizeof(T), &Ah));
    TLSQ_TRY(ws_get(h, WS_E, (size_t)M * nc * sizeof(T), &Eh));
    const hipMemcpyKind kin = dev ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice;
    TLSQ_TRY(copy2d(h, AA, M, A, ldA, M, n, sizeof(T), kin));                          // AA = [A y]  :153
    TLSQ_TRY(copy2d(h, (T*)AA + (size_t)M * n, M, y, ldy, M, q, sizeof(T), kin));
    ResolvedOpts ro = resolve(opts, M, nc, std::sqrt((double)std::numeric_limits<T>::epsilon()));
    ro.nukeA = false;                                                                 // :154
    std::vector<double> Vt((size_t)nc * nc, 0.0);
    const int64_t d = std::min(ro.m_global, nc);
    if (d < nc) return set_err(h, TLSQ_ERR_ARG, "rtls: needs M >= n+q");
    const int status = rpca_core<T>(h, (const T*)AA, M, nc, ro, opts, (T*)Ah, (T*)Eh, nullptr, nullptr, Vt.data(), nc,
                                    nullptr, info);
    if (status < 0) return status;
    std::vector<double> hx((size_t)n * q);
    const int st = tls_partition_solve(Vt.data(), nc, nc, n, hx.data(), n);           // :155
    if (st < 0) return set_err(h, st, "rtls: partition solve failed");
    TLSQ_TRY(put_x<T>(h, hx, n, q, x, ldx, dev));
    return status;
}

extern "C" {

int tlsq_tls_f64(tlsq_handle h, const double* Ay, int64_t M, int64_t ncols, int64_t ldAy, int64_t n,
                 double* x, int64_t ldx, int memory) {
    TLSQ_TRY(ws_poison_all(h));
    return tls_impl<double>(h, Ay, M, ncols, ldAy, n, x, ldx, memory);
}
int tlsq_tls_f32(tlsq_handle h, const float* Ay, int64_t M, int64_t ncols, int64_t ldAy, int64_t n,
                 float* x, int64_t ldx, int memory) {
    TLSQ_TRY(ws_poison_all(h));
    return tls_impl<float>(h, Ay, M, ncols, ldAy, n, x, ldx, memory);
}
int tlsq_rtls_f64(tlsq_handle h, const double* A, int64_t M, int64_t n, int64_t ldA, const double* y,
                  int64_t q, int64_t ldy, const tlsq_rpca_opts* opts, double* x, int64_t ldx,
                  tlsq_rpca_info* info) {
    TLSQ_TRY(ws_poison_all(h));
    return rtls_impl<double>(h, A, M, n, ldA, y, q, ldy, opts, x, ldx, info);
}
int tlsq_rtls_f32(tlsq_handle h, const float* A, int64_t M, int64_t n, int64_t ldA, const float* y,
                  int64_t q, int64_t ldy, const tlsq_rpca_opts* opts, float* x, int64_t ldx,
                  tlsq_rpca_info* info) {
    TLSQ_TRY(ws_poison_all(h));
    return rtls_impl<float>(h, A, M, n, ldA, y, q, ldy, opts, x, ldx, info);
}

// ---- ComplexF64 rpca ---------------------------------------------------------------------------------------
int tlsq_rpca_c64(tlsq_handle h, const double* D, int64_t M, int64_t N, int64_t ldD, const tlsq_rpca_opts* opts,
                  double* A, int64_t ldA, double* E, int64_t ldE, double* S, int64_t* sv, tlsq_rpca_info* info) {
    return tlsq_rpca_c64_svd(h, D, M, N, ldD, opts, A, ldA, E, ldE, nullptr, 0, S, nullptr, 0, sv, info);
}

int tlsq_rpca_c64_svd(tlsq_handle h, const double* D, int64_t M, int64_t N, int64_t ldD, const tlsq_rpca_opts* opts,
                      double* A, int64_t ldA, double* E, int64_t ldE, double* U, int64_t ldU, double* S, double* Vt,
                      int64_t ldVt, int64_t* sv, tlsq_rpca_info* info) {
    TLSQ_TRY(check_handle(h));
    if ((U && ldU < M) || (Vt && ldVt < std::min(M, N)))
        return set_err(h, TLSQ_ERR_ARG, "rpca_c64: ldU < M or ldVt < min(M,N)");
    if (!D || !A || !E || M <= 0 || N <= 0 || ldD < M || ldA < M || ldE < M)
        return set_err(h, TLSQ_ERR_ARG, "rpca_c64: bad argument (M=%lld N=%lld)", (long long)M, (long long)N);
    if (opts && (opts->nonnegA || opts->nonnegE || opts->hankel))
        return set_err(h, TLSQ_ERR_UNSUPPORTED, "rpca_c64: nonnegA / nonnegE / hankel are not defined for complex data "
                       "(the reference's max.(A, 0) / soft_hankel! have no complex method)");
    if (opts && (opts->svd_mode != TLSQ_SVD_FULL || opts->opnorm_mode != TLSQ_OPNORM_EXACT))
        return set_err(h, TLSQ_ERR_UNSUPPORTED, "rpca_c64: hook modes are not available for complex data");
    if (h->comm || (opts && opts->m_global > 0 && opts->m_global != M))
        return set_err(h, TLSQ_ERR_UNSUPPORTED, "rpca_c64: row sharding is not available for complex data");
    if (2 * N > kFullEigMaxN)
        return set_err(h, TLSQ_ERR_UNSUPPORTED, "rpca_c64: N = %lld; the complex path handles N <= %lld", (long long)N,
                       (long long)(kFullEigMaxN / 2));
    TLSQ_HIP(h, hipSetDevice(h->device));
    const double t0 = now_ms();
    reset_info(info);
    const ResolvedOpts ro = resolve(opts, M, N, std::sqrt(std::numeric_limits<double>::epsilon()));
    const bool dev = opts && opts->memory == TLSQ_MEM_DEVICE;
    const int64_t n = M * N;
    const double* dD = D;
    double *dA = A, *dE = E;
    void* p;
    if (!dev || ldD != M) {
        TLSQ_TRY(ws_get(h, WS_D, (size_t)n * 16, &p));
        TLSQ_TRY(copy2d(h, p, M, D, ldD, M, N, 16, dev ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice));
        dD = (const double*)p;
    }
    if (!dev || ldA != M) {
        TLSQ_TRY(ws_get(h, WS_A, (size_t)n * 16, &p));
        dA = (double*)p;
    }
    if (!dev || ldE != M) {
        TLSQ_TRY(ws_get(h, WS_E, (size_t)n * 16, &p));
        dE = (double*)p;
    }
    const int64_t d = std::min(M, N);
    std::vector<double> hS((size_t)(S ? d : 0));
    std::vector<double> hVt((size_t)(Vt ? 2 * d * N : 0));
    double* dU = nullptr;
    if (U) {
        TLSQ_TRY(ws_get(h, WS_UT, (size_t)M * d * 16, &p));
        dU = (double*)p;
    }
    const int status = rpca_core_complex(h, dD, M, N, ro, opts, dA, dE, S ? hS.data() : nullptr, sv, info, dU,
                                         Vt ? hVt.data() : nullptr, d);
    if (status < 0) return status;
    const hipMemcpyKind back = dev ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost;
    if (dA != A) TLSQ_TRY(copy2d(h, A, ldA, dA, M, M, N, 16, back));
    if (dE != E) TLSQ_TRY(copy2d(h, E, ldE, dE, M, M, N, 16, back));
    if (U) TLSQ_TRY(copy2d(h, U, ldU, dU, M, M, d, 16, back));
    if (Vt) TLSQ_TRY(copy2d(h, Vt, ldVt, hVt.data(), d, d, N, 16, dev ? hipMemcpyHostToDevice : hipMemcpyHostToHost));
    if (S) TLSQ_HIP(h, hipMemcpyAsync(S, hS.data(), (size_t)d * 8, dev ? hipMemcpyHostToDevice : hipMemcpyHostToHost,
                                      h->stream));
    TLSQ_HIP(h, hipStreamSynchronize(h->stream));
    if (info) info->ms_total = now_ms() - t0;
    return status;
}

// ---- ComplexF32 rpca: widened on the device, solved by the ComplexF64 path, rounded on the way out ------------------------
int tlsq_rpca_c32_svd(tlsq_handle h, const float* D, int64_t M, int64_t N, int64_t ldD, const tlsq_rpca_opts* opts,
                      float* A, int64_t ldA, float* E, int64_t ldE, float* U, int64_t ldU, float* S, float* Vt,
                      int64_t ldVt, int64_t* sv, tlsq_rpca_info* info) {
    TLSQ_TRY(check_handle(h));
    const int64_t d = std::min(M, N);
    if ((U && ldU < M) || (Vt && ldVt < d))
        return set_err(h, TLSQ_ERR_ARG, "rpca_c32: ldU < M or ldVt < min(M,N)");
    if (!D || !A || !E || M <= 0 || N <= 0 || ldD < M || ldA < M || ldE < M)
        return set_err(h, TLSQ_ERR_ARG, "rpca_c32: bad argument (M=%lld N=%lld)", (long long)M, (long long)N);
    TLSQ_HIP(h, hipSetDevice(h->device));
    const bool dev = opts && opts->memory == TLSQ_MEM_DEVICE;
    tlsq_rpca_opts o;
    if (opts) o = *opts; else tlsq_rpca_opts_default(&o);
    if (std::isnan(o.tol)) o.tol = std::sqrt((double)std::numeric_limits<float>::epsilon());   // :160 with T = ComplexF32
    o.memory = TLSQ_MEM_DEVICE;
    const int64_t n = M * N;
    // float staging (contiguous, ld M) and the fp64 panels of the inner call: slots the ComplexF64 path does not take itself
    void *f32v, *D64, *A64, *E64, *U64 = nullptr, *S64 = nullptr, *V64 = nullptr;
    TLSQ_TRY(ws_get(h, WS_C32_F, (size_t)std::max(n, M * d) * 8, &f32v));
    TLSQ_TRY(ws_get(h, WS_C32_D, (size_t)n * 16, &D64));
    TLSQ_TRY(ws_get(h, WS_C32_A, (size_t)n * 16, &A64));
    TLSQ_TRY(ws_get(h, WS_C32_E, (size_t)n * 16, &E64));
    if (U) TLSQ_TRY(ws_get(h, WS_C32_U, (size_t)M * d * 16, &U64));
    if (S) TLSQ_TRY(ws_get(h, WS_C32_S, (size_t)d * 8, &S64));
    if (Vt) TLSQ_TRY(ws_get(h, WS_C32_V, (size_t)d * N * 16, &V64));
    float* f32 = (float*)f32v;
    TLSQ_TRY(copy2d(h, f32, M, D, ldD, M, N, 8, dev ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice));
    TLSQ_TRY((launch_convert<float, double>(h, f32, (double*)D64, 2 * n)));
    const int status = tlsq_rpca_c64_svd(h, (const double*)D64, M, N, M, &o, (double*)A64, M, (double*)E64, M, (double*)U64, M,
                                         (double*)S64, (double*)V64, d, sv, info);
    if (status < 0) return status;
    const hipMemcpyKind back = dev ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost;
    auto out = [&](const void* src64, int64_t rows, int64_t cols, float* dst, int64_t ldd) -> int {
        TLSQ_TRY((launch_convert<double, float>(h, (const double*)src64, f32, 2 * rows * cols)));
        TLSQ_TRY(copy2d(h, dst, ldd, f32, rows, rows, cols, 8, back));
        TLSQ_HIP(h, hipStreamSynchronize(h->stream));   // (the staging panel is reused by the next output)
        return TLSQ_OK;
    };
    TLSQ_TRY(out(A64, M, N, A, ldA));
    TLSQ_TRY(out(E64, M, N, E, ldE));
    if (U) TLSQ_TRY(out(U64, M, d, U, ldU));
    if (Vt) TLSQ_TRY(out(V64, d, N, Vt, ldVt));
    if (S) {
        TLSQ_TRY((launch_convert<double, float>(h, (const double*)S64, f32, d)));
        TLSQ_HIP(h, hipMemcpyAsync(S, f32, (size_t)d * 4, back, h->stream));
        TLSQ_HIP(h, hipStreamSynchronize(h->stream));
    }
    return status;
}

// ---- batched tiny problems (batched.hip) ---------------------------------------------------------------
// validates the options shared by the two batched entry points
static int batched_opts(tlsq_handle h, const tlsq_rpca_opts* opts, int64_t M, int64_t N, const char* who, ResolvedOpts* ro,
                        double default_tol) {
    if (N > 32)
        return set_err(h, TLSQ_ERR_UNSUPPORTED, "%s: N = %lld columns; the batched kernel handles N <= 32 (use the "
                       "per-problem entry point)", who, (long long)N);
    if (M < N) return set_err(h, TLSQ_ERR_UNSUPPORTED, "%s: needs M >= N (tall problems)", who);
    if (opts && (opts->hankel || opts->svd_mode != TLSQ_SVD_FULL || opts->opnorm_mode != TLSQ_OPNORM_EXACT ||
                 opts->on_iter || (opts->m_global > 0 && opts->m_global != M)))
        return set_err(h, TLSQ_ERR_UNSUPPORTED, "%s: hankel / hook modes / on_iter / row sharding are not available "
                       "in the batched kernel", who);
    if (h->comm) return set_err(h, TLSQ_ERR_UNSUPPORTED, "%s: not available on a row-sharded handle", who);
    *ro = resolve(opts, M, N, default_tol);
    return TLSQ_OK;
}

}  // extern "C" (templates below)

template <typename T>
static int rpca_batched_impl(tlsq_handle h, const T* D, int64_t M, int64_t N, int64_t batch,
                             const tlsq_rpca_opts* opts, T* A, T* E, T* S, T* Vt, int64_t* sv,
                             int32_t* iters, int32_t* status, T* cost) {
    constexpr size_t ES = sizeof(T);
    TLSQ_TRY(check_handle(h));
    if (!D || !A || !E || M <= 0 || N <= 0 || batch < 0)
        return set_err(h, TLSQ_ERR_ARG, "rpca_batched: bad argument");
    if (batch == 0) return TLSQ_OK;
    TLSQ_HIP(h, hipSetDevice(h->device));
    ResolvedOpts ro;
    TLSQ_TRY(batched_opts(h, opts, M, N, "rpca_batched", &ro, std::sqrt((double)std::numeric_limits<T>::epsilon())));
    const bool dev = opts && opts->memory == TLSQ_MEM_DEVICE;
    const size_t pn = (size_t)M * N * batch * ES;
    bool in_lds;
    (void)rpca_small_lds_bytes(M, N, &in_lds, ES);
    void* scratch = nullptr;
    if (!in_lds) TLSQ_TRY(ws_get(h, WS_BATCH4, 5 * pn, &scratch));
    const T* dD = D;
    T *dA = A, *dE = E, *dS = S, *dVt = Vt, *dcost = cost;
    int64_t* dsv = sv;
    int32_t *dit = iters, *dst = status;
    void* p;
    if (!dev) {
        TLSQ_TRY(ws_get(h, WS_BATCH0, pn, &p));
        TLSQ_HIP(h, hipMemcpyAsync(p, D, pn, hipMemcpyHostToDevice, h->stream));
        dD = (const T*)p;
        TLSQ_TRY(ws_get(h, WS_BATCH1, pn, &p));
        dA = (T*)p;
        TLSQ_TRY(ws_get(h, WS_BATCH2, pn, &p));
        dE = (T*)p;
    }
    // the small per-problem outputs always go through one device block: S | Vt | cost | sv | iters | status
    auto al8 = [](size_t v) { return (v + 7) & ~(size_t)7; };
    const size_t oS = 0, oVt = al8(oS + (size_t)N * batch * ES), oC = al8(oVt + (size_t)N * N * batch * ES),
                 oSv = al8(oC + (size_t)batch * ES), oIt = oSv + (size_t)batch * 8, oSt = oIt + (size_t)batch * 4,
                 oEnd = oSt + (size_t)batch * 4;
    char* blk = nullptr;
    if (!dev) {
        TLSQ_TRY(ws_get(h, WS_BATCH3, oEnd, &p));
        blk = (char*)p;
        dS = (T*)(blk + oS);
        dVt = (T*)(blk + oVt);
        dcost = (T*)(blk + oC);
        dsv = (int64_t*)(blk + oSv);
        dit = (int32_t*)(blk + oIt);
        dst = (int32_t*)(blk + oSt);
    } else if (!status) {   // the return code needs the per-problem status even when the caller does not ask for it
        TLSQ_TRY(ws_get(h, WS_BATCH3, (size_t)batch * 4, &p));
        dst = (int32_t*)p;
    }
    TLSQ_TRY(launch_rpca_small<T>(h, dD, M, N, batch, ro.lambda, ro.tol, ro.rho, ro.iters, ro.maxrank, ro.nonnegA,
                               ro.nonnegE, ro.nukeA, dA, dE, dS, dVt, dsv, dit, dst, dcost, (T*)scratch));
    std::vector<int32_t> hst((size_t)batch);
    if (!dev) {
        TLSQ_HIP(h, hipMemcpyAsync(A, dA, pn, hipMemcpyDeviceToHost, h->stream));
        TLSQ_HIP(h, hipMemcpyAsync(E, dE, pn, hipMemcpyDeviceToHost, h->stream));
        std::vector<char> hb(oEnd);
        TLSQ_HIP(h, hipMemcpyAsync(hb.data(), blk, oEnd, hipMemcpyDeviceToHost, h->stream));
        TLSQ_HIP(h, hipStreamSynchronize(h->stream));
        if (S) memcpy(S, hb.data() + oS, (size_t)N * batch * ES);
        if (Vt) memcpy(Vt, hb.data() + oVt, (size_t)N * N * batch * ES);
        if (cost) memcpy(cost, hb.data() + oC, (size_t)batch * ES);
        if (sv) memcpy(sv, hb.data() + oSv, (size_t)batch * 8);
        if (iters) memcpy(iters, hb.data() + oIt, (size_t)batch * 4);
        if (status) memcpy(status, hb.data() + oSt, (size_t)batch * 4);
        memcpy(hst.data(), hb.data() + oSt, (size_t)batch * 4);
    } else {
        TLSQ_HIP(h, hipMemcpyAsync(hst.data(), dst, (size_t)batch * 4, hipMemcpyDeviceToHost, h->stream));
        TLSQ_HIP(h, hipStreamSynchronize(h->stream));
    }
    for (int32_t v : hst)
        if (v != 0) return TLSQ_MAXITER;   // at least one problem ran into the iteration limit (:232)
    return TLSQ_OK;
}

template <typename T>
static int rtls_batched_impl(tlsq_handle h, const T* A, const T* y, int64_t M, int64_t n, int64_t q,
                             int64_t batch, const tlsq_rpca_opts* opts, T* x, int32_t* iters, int32_t* status) {
    constexpr size_t ES = sizeof(T);
    TLSQ_TRY(check_handle(h));
    if (!A || !y || !x || M <= 0 || n <= 0 || q <= 0 || batch < 0)
        return set_err(h, TLSQ_ERR_ARG, "rtls_batched: bad argument");
    if (batch == 0) return TLSQ_OK;
    TLSQ_HIP(h, hipSetDevice(h->device));
    const int64_t nc = n + q;
    ResolvedOpts ro;
    TLSQ_TRY(batched_opts(h, opts, M, nc, "rtls_batched", &ro, std::sqrt((double)std::numeric_limits<T>::epsilon())));
    ro.nukeA = false;                                                                  // TotalLeastSquares.jl:154
    const bool dev = opts && opts->memory == TLSQ_MEM_DEVICE;
    const size_t pn = (size_t)M * nc * batch * ES;
    void *AA, *Ar, *Er, *blkv, *scratch = nullptr;
    TLSQ_TRY(ws_get(h, WS_BATCH0, pn, &AA));
    TLSQ_TRY(ws_get(h, WS_BATCH1, pn, &Ar));
    TLSQ_TRY(ws_get(h, WS_BATCH2, pn, &Er));
    bool in_lds;
    (void)rpca_small_lds_bytes(M, nc, &in_lds, ES);
    if (!in_lds) TLSQ_TRY(ws_get(h, WS_BATCH4, 5 * pn, &scratch));
    const size_t oVt = 0, oIt = (((size_t)nc * nc * batch * ES) + 7) & ~(size_t)7, oSt = oIt + (size_t)batch * 4,
                 oEnd = oSt + (size_t)batch * 4;
    TLSQ_TRY(ws_get(h, WS_BATCH3, oEnd, &blkv));
    char* blk = (char*)blkv;
    // AA_b = [A_b y_b]  (:153): two strided copies, one row of the 2-D copy per problem
    const hipMemcpyKind kin = dev ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice;
    TLSQ_HIP(h, hipMemcpy2DAsync(AA, (size_t)M * nc * ES, A, (size_t)M * n * ES, (size_t)M * n * ES, (size_t)batch, kin,
                                 h->stream));
    TLSQ_HIP(h, hipMemcpy2DAsync((char*)AA + (size_t)M * n * ES, (size_t)M * nc * ES, y, (size_t)M * q * ES,
                                 (size_t)M * q * ES, (size_t)batch, kin, h->stream));
    TLSQ_TRY(launch_rpca_small<T>(h, (const T*)AA, M, nc, batch, ro.lambda, ro.tol, ro.rho, ro.iters, ro.maxrank,
                                  ro.nonnegA, ro.nonnegE, ro.nukeA, (T*)Ar, (T*)Er, nullptr,
                                  (T*)(blk + oVt), nullptr, (int32_t*)(blk + oIt), (int32_t*)(blk + oSt), nullptr,
                                  (T*)scratch));
    std::vector<char> hb(oEnd);
    TLSQ_HIP(h, hipMemcpyAsync(hb.data(), blk, oEnd, hipMemcpyDeviceToHost, h->stream));
    TLSQ_HIP(h, hipStreamSynchronize(h->stream));
    const T* hVt = reinterpret_cast<const T*>(hb.data() + oVt);
    const int32_t* hst = reinterpret_cast<const int32_t*>(hb.data() + oSt);
    std::vector<double> hx((size_t)n * q * batch), vt64((size_t)nc * nc);
    int rc = TLSQ_OK;
    for (int64_t b = 0; b < batch; ++b) {                                              // tls!(s, n)  :155
        if (hst[b] == 2) {   // Infs / NaNs in this problem (batched.hip): x = NaN, the others are solved
            for (int64_t e = 0; e < n * q; ++e) hx[(size_t)(b * n * q + e)] = std::numeric_limits<double>::quiet_NaN();
            rc = TLSQ_MAXITER;
            continue;
        }
        for (int64_t e = 0; e < nc * nc; ++e) vt64[(size_t)e] = (double)hVt[(size_t)b * nc * nc + e];
        int st = tls_partition_solve(vt64.data(), nc, nc, n, hx.data() + (size_t)b * n * q, n);
        if (st < 0) return set_err(h, st, "rtls_batched: partition solve failed for problem %lld", (long long)b);
        if (hst[b] != 0) rc = TLSQ_MAXITER;
    }
    std::vector<T> hxT(hx.size());
    for (size_t e = 0; e < hx.size(); ++e) hxT[e] = (T)hx[e];
    if (dev) {
        TLSQ_HIP(h, hipMemcpyAsync(x, hxT.data(), hxT.size() * ES, hipMemcpyHostToDevice, h->stream));
        if (iters) TLSQ_HIP(h, hipMemcpyAsync(iters, blk + oIt, (size_t)batch * 4, hipMemcpyDeviceToDevice, h->stream));
        if (status) TLSQ_HIP(h, hipMemcpyAsync(status, blk + oSt, (size_t)batch * 4, hipMemcpyDeviceToDevice, h->stream));
        TLSQ_HIP(h, hipStreamSynchronize(h->stream));
    } else {
        memcpy(x, hxT.data(), hxT.size() * ES);
        if (iters) memcpy(iters, hb.data() + oIt, (size_t)batch * 4);
        if (status) memcpy(status, hb.data() + oSt, (size_t)batch * 4);
    }
    return rc;
}


extern "C" {
int tlsq_rpca_batched_f64(tlsq_handle h, const double* D, int64_t M, int64_t N, int64_t batch,
                          const tlsq_rpca_opts* opts, double* A, double* E, double* S, double* Vt, int64_t* sv,
                          int32_t* iters, int32_t* status, double* cost) {
    return rpca_batched_impl<double>(h, D, M, N, batch, opts, A, E, S, Vt, sv, iters, status, cost);
}
int tlsq_rpca_batched_f32(tlsq_handle h, const float* D, int64_t M, int64_t N, int64_t batch,
                          const tlsq_rpca_opts* opts, float* A, float* E, float* S, float* Vt, int64_t* sv,
                          int32_t* iters, int32_t* status, float* cost) {
    return rpca_batched_impl<float>(h, D, M, N, batch, opts, A, E, S, Vt, sv, iters, status, cost);
}
int tlsq_rtls_batched_f64(tlsq_handle h, const double* A, const double* y, int64_t M, int64_t n, int64_t q,
                          int64_t batch, const tlsq_rpca_opts* opts, double* x, int32_t* iters, int32_t* status) {
    return rtls_batched_impl<double>(h, A, y, M, n, q, batch, opts, x, iters, status);
}
int tlsq_rtls_batched_f32(tlsq_handle h, const float* A, const float* y, int64_t M, int64_t n, int64_t q,
                          int64_t batch, const tlsq_rpca_opts* opts, float* x, int32_t* iters, int32_t* status) {
    return rtls_batched_impl<float>(h, A, y, M, n, q, batch, opts, x, iters, status);
}

// ---- kernel-level entry points (device pointers) ---------------------------------------------------
int tlsq_k_shrink_f64(tlsq_handle h, const double* D, const double* A, const double* Y, double* E,
                      double* Z, int64_t n, double inv_mu, double thr, int nonnegE) {
    TLSQ_TRY(check_handle(h));
    return launch_shrink<double>(h, D, A, Y, E, Z, n, inv_mu, thr, nonnegE);
}
int tlsq_k_update_f64(tlsq_handle h, const double* D, double* A, const double* E, double* Y, double* R,
                      int64_t n, double mu, int nonnegA) {
    TLSQ_TRY(check_handle(h));
    return launch_update<double>(h, D, A, E, Y, R, n, mu, nonnegA);
}
int tlsq_k_shrink_f32(tlsq_handle h, const float* D, const float* A, const float* Y, float* E, float* Z,
                      int64_t n, float inv_mu, float thr, int nonnegE) {
    TLSQ_TRY(check_handle(h));
    return launch_shrink<float>(h, D, A, Y, E, Z, n, inv_mu, thr, nonnegE);
}
int tlsq_k_update_f32(tlsq_handle h, const float* D, float* A, const float* E, float* Y, float* R,
                      int64_t n, float mu, int nonnegA) {
    TLSQ_TRY(check_handle(h));
    return launch_update<float>(h, D, A, E, Y, R, n, mu, nonnegA);
}
int tlsq_k_update_shrink_f64(tlsq_handle h, const double* D, double* A, const double* E, double* Y, double* R,
                             double* En, double* Zn, int64_t n, double mu, int nonnegA, double inv_mu_next,
                             double thr_next, int nonnegE) {
    TLSQ_TRY(check_handle(h));
    return launch_update_shrink<double>(h, D, A, E, Y, R, En, Zn, n, mu, nonnegA, inv_mu_next, thr_next, nonnegE, nullptr, nullptr);
}
int tlsq_k_update_shrink_f32(tlsq_handle h, const float* D, float* A, const float* E, float* Y, float* R,
                             float* En, float* Zn, int64_t n, float mu, int nonnegA, float inv_mu_next,
                             float thr_next, int nonnegE) {
    TLSQ_TRY(check_handle(h));
    return launch_update_shrink<float>(h, D, A, E, Y, R, En, Zn, n, mu, nonnegA, inv_mu_next, thr_next, nonnegE, nullptr, nullptr);
}
int tlsq_k_rebuild_update_shrink_f64(tlsq_handle h, const double* D, const double* Tm, const double* Vs, const double* E,
                                     double* Y, double* R, double* En, double* Zn, int64_t M, int64_t N, int64_t r,
                                     double mu, int nonnegA, double inv_mu_next, double thr_next, int nonnegE) {
    TLSQ_TRY(check_handle(h));
    if (M % 2 != 0 || r > 32 || r < 0) return set_err(h, TLSQ_ERR_ARG, "k_rebuild_update_shrink: needs even M and r <= 32");
    return launch_rebuild_update_shrink<double>(h, D, Tm, Vs, E, Y, R, En, Zn, M, N, r, mu, nonnegA, inv_mu_next,
                                                thr_next, nonnegE, nullptr, nullptr);
}
int tlsq_k_zsweep_f64(tlsq_handle h, const double* D, const double* Tm, const double* Vs, double* A, const double* Yin,
                      double* Yout, double* Z, double* R, int64_t M, int64_t N, int64_t r, double mu, double inv_mu,
                      int nonnegA, double inv_mu_next, double thr_next, int nonnegE, double* sumsq) {
    TLSQ_TRY(check_handle(h));
    if (!D || !Yin || !Yout || !Z || M <= 0 || N <= 0 || r < 0 || (!A && r > 32) || Yin == Yout)
        return set_err(h, TLSQ_ERR_ARG, "k_zsweep: bad argument (factors serve r <= 32; Y is double-buffered)");
    return launch_zsweep<double>(h, D, Tm, Vs, A, Yin, Yout, Z, R, M, N, r, mu, inv_mu, nonnegA, inv_mu_next, thr_next,
                                 nonnegE, sumsq, nullptr);
}
int tlsq_k_zsweep_wide_f32(tlsq_handle h, const float* D, const double* Vg, const double* Vs, int64_t r, const float* Yin,
                           float* Yout, float* Z, float* Zout, float* R, double* Tm, int64_t M, int64_t N, float mu,
                           float inv_mu, int nonnegA, float inv_mu_next, float thr_next, int nonnegE, double* sumsq) {
    TLSQ_TRY(check_handle(h));
    if (!D || !Vg || !Vs || !Yin || !Yout || !Z || !Zout || M <= 0 || N <= 0 || Yin == Yout)
        return set_err(h, TLSQ_ERR_ARG, "k_zsweep_wide: bad argument");
    if (!zsweep_wide_ok(M, N, r) || !wide_factors_ok(Z, M, M, N, r))
        return set_err(h, TLSQ_ERR_UNSUPPORTED, "k_zsweep_wide: fp32 panels with M %% 128 == 0, N %% 128 == 0, M N >= 2^26, ranks 33..80");
    TLSQ_HIP(h, hipSetDevice(h->device));
    const float *t32 = nullptr, *vs32 = nullptr;
    int lw = 0;
    TLSQ_TRY(wide_factors_f32(h, Z, M, M, N, Vg, Vs, r, Tm, &t32, &vs32, &lw));
    return launch_zsweep_wide(h, D, t32, M, vs32, r, Yin, Yout, Z, Zout, R, M, N, mu, inv_mu, nonnegA, inv_mu_next, thr_next,
                              nonnegE, sumsq, nullptr, sumsq ? 0 : -1);
}
int tlsq_k_zsweep_gram_f64(tlsq_handle h, const double* D, const double* Tm, const double* Vs, const double* Yin,
                           double* Yout, const double* Zin, double* Zout, double* R, int64_t M, int64_t N, int64_t r,
                           double mu, double inv_mu, int nonnegA, double inv_mu_next, double thr_next, int nonnegE,
                           double* sumsq, const double* hankel_y, int64_t hankel_K, double* G, int64_t ldG) {
    TLSQ_TRY(check_handle(h));
    if ((!D && !hankel_y) || !Yin || !Yout || !Zin || !Zout || !G || M <= 0 || N <= 0 || r < 0 || Yin == Yout || ldG < N ||
        (r > 0 && (!Tm || !Vs)))
        return set_err(h, TLSQ_ERR_ARG, "k_zsweep_gram: bad argument");
    if (!fused_zgram_ok(M, N, r, D, Yin, Yout, Zin, Zout, R, hankel_y != nullptr, thr_next))
        return set_err(h, TLSQ_ERR_UNSUPPORTED, "k_zsweep_gram: fp64 panels of 256 or 512 columns, even M above the row floor, rank <= 16, 16-byte alignment");
    TLSQ_HIP(h, hipSetDevice(h->device));
    GramPlan pl;
    TLSQ_TRY(fused_zgram_plan(h, M, N, &pl));
    TLSQ_TRY(launch_fused_zgram(h, pl, D, Tm, Vs, Yin, Yout, Zin, Zout, R, M, N, r, mu, inv_mu, nonnegA, inv_mu_next, thr_next,
                                nonnegE, sumsq, nullptr, hankel_y, hankel_K, sumsq ? 0 : -1));
    if (ldG != N) return set_err(h, TLSQ_ERR_ARG, "k_zsweep_gram: ldG = N");
    return fused_zgram_finish(h, pl, Zout, M, N, G);
}
int tlsq_k_final_e_f64(tlsq_handle h, const double* D, const double* Tm, const double* Vs, const double* Aprev,
                       const double* Y, double* E, int64_t M, int64_t N, int64_t r, double inv_mu, double thr, int nonnegA,
                       int nonnegE) {
    TLSQ_TRY(check_handle(h));
    if (!D || !Y || !E || M <= 0 || N <= 0 || r < 0 || (!Aprev && r > 32))
        return set_err(h, TLSQ_ERR_ARG, "k_final_e: bad argument");
    return launch_final_e<double>(h, D, Tm, Vs, Aprev, Y, E, M, N, r, inv_mu, thr, nonnegA, nonnegE);
}
int tlsq_k_matfun_sign_f64(tlsq_handle h, const double* C, int64_t N, double* X, int32_t* iters) {
    TLSQ_TRY(check_handle(h));
    if (!C || !X || N <= 0 || N > 1024) return set_err(h, TLSQ_ERR_ARG, "matfun_sign: bad argument (N <= 1024)");
    TLSQ_HIP(h, hipSetDevice(h->device));
    void *w1, *w2;
    TLSQ_TRY(ws_get(h, WS_CP1, (size_t)N * N * 8, &w1));
    TLSQ_TRY(ws_get(h, WS_CP2, (size_t)N * N * 8, &w2));
    int it = 0;
    bool ok = false;
    TLSQ_TRY(matfun_sign(h, C, N, X, (double*)w1, (double*)w2, 100, &it, &ok));
    TLSQ_HIP(h, hipStreamSynchronize(h->stream));   // (the last copy of the iterate into X is still queued)
    if (iters) *iters = it;
    return ok ? TLSQ_OK : set_err(h, TLSQ_ERR_NOCONV, "matfun_sign: no convergence in 100 steps");
}
int tlsq_k_matfun_invsqrt_f64(tlsq_handle h, const double* B, int64_t N, double hi, double* W, int32_t* iters) {
    TLSQ_TRY(check_handle(h));
    if (!B || !W || N <= 0 || N > 1024) return set_err(h, TLSQ_ERR_ARG, "matfun_invsqrt: bad argument (N <= 1024)");
    TLSQ_HIP(h, hipSetDevice(h->device));
    void *y, *t, *w;
    TLSQ_TRY(ws_get(h, WS_CP1, (size_t)N * N * 8, &y));
    TLSQ_TRY(ws_get(h, WS_CP2, (size_t)N * N * 8, &t));
    TLSQ_TRY(ws_get(h, WS_GD, (size_t)N * N * 8, &w));
    int it = 0;
    bool ok = false;
    TLSQ_TRY(matfun_invsqrt(h, B, N, hi, W, (double*)y, (double*)t, (double*)w, 100, &it, &ok));
    TLSQ_HIP(h, hipStreamSynchronize(h->stream));   // (the final scaling of W is still queued)
    if (iters) *iters = it;
    return ok ? TLSQ_OK : set_err(h, TLSQ_ERR_NOCONV, "matfun_invsqrt: no convergence in 100 steps");
}
int tlsq_k_rr_small_f64(tlsq_handle h, const double* B, const double* Hg, int64_t p, int64_t nt, double tau2, double* C,
                        double* lam, double* status) {
    TLSQ_TRY(check_handle(h));
    if (!B || !Hg || !C || !lam || !status || p < 1 || p > 32 || nt < 0) return set_err(h, TLSQ_ERR_ARG, "k_rr_small: bad argument (p <= 32)");
    return launch_rr_small_only(h, B, Hg, C, lam, status, p, std::min(nt, p), tau2);
}
int tlsq_k_op_gram_f32(tlsq_handle h, const float* Z, int64_t M, int64_t N, int64_t ldZ, const double* X, int64_t p, double* Y) {
    TLSQ_TRY(check_handle(h));
    if (!Z || !X || !Y || M <= 0 || N <= 0 || p <= 0 || ldZ < M) return set_err(h, TLSQ_ERR_ARG, "k_op_gram_f32: bad arguments");
    for (int64_t c0 = 0; c0 < p; c0 += 96)
        TLSQ_TRY(op_gram_f32(h, Z, ldZ, M, N, X + (size_t)c0 * N, N, Y + (size_t)c0 * N, N, std::min<int64_t>(96, p - c0)));
    return TLSQ_OK;
}
int tlsq_k_gram_f32(tlsq_handle h, const float* Z, int64_t M, int64_t N, int64_t ldZ, double* G, int64_t ldG, int mfma32) {
    TLSQ_TRY(check_handle(h));
    if (!Z || !G || M < 0 || N <= 0 || ldZ < M || ldG < N) return set_err(h, TLSQ_ERR_ARG, "k_gram_f32: bad arguments");
    return gram_any(h, Z, 1, M, N, ldZ, G, ldG, mfma32);
}
int tlsq_k_gram_f64(tlsq_handle h, const double* Z, int64_t M, int64_t N, int64_t ldZ, double* G,
                    int64_t ldG) {
    TLSQ_TRY(check_handle(h));
    if (!Z || !G || N <= 0 || ldZ < M || ldG < N) return set_err(h, TLSQ_ERR_ARG, "gram: bad argument");
    return gram_f64(h, Z, M, N, ldZ, G, ldG);
}
int tlsq_k_gemm_nn_f64(tlsq_handle h, const double* Z, int64_t M, int64_t K, int64_t ldZ, const double* W,
                       int64_t Q, int64_t ldW, double* C, int64_t ldC) {
    TLSQ_TRY(check_handle(h));
    if (!Z || !W || !C || ldZ < M || ldW < K || ldC < M) return set_err(h, TLSQ_ERR_ARG, "gemm_nn: bad argument");
    if (Q <= 96) return tsmm_mixed(h, Z, 0, ldZ, W, ldW, C, ldC, M, K, Q);   // the rebuild's factor GEMM (tall-skinny kernel)
    return gemm_f64(h, true, false, W, ldW, Z, ldZ, C, ldC, Q, M, K, false);
}
int tlsq_k_gemm_nt_f64(tlsq_handle h, const double* T, int64_t M, int64_t K, int64_t ldT, const double* V,
                       int64_t Q, int64_t ldV, double* C, int64_t ldC) {
    TLSQ_TRY(check_handle(h));
    if (!T || !V || !C || ldT < M || ldV < Q || ldC < M) return set_err(h, TLSQ_ERR_ARG, "gemm_nt: bad argument");
    return gemm_f64(h, false, false, V, ldV, T, ldT, C, ldC, Q, M, K, false);
}
int tlsq_k_symeig_f64(tlsq_handle h, const double* G, int64_t N, int64_t ldG, double* lam, double* V,
                      int64_t ldV, int64_t* sweeps) {
    TLSQ_TRY(check_handle(h));
    if (!G || !lam || N <= 0 || ldG < N || (V && ldV < N)) return set_err(h, TLSQ_ERR_ARG, "symeig: bad argument");
    void *B, *Vw, *lamw;
    TLSQ_TRY(ws_get(h, WS_B, (size_t)N * N * 8, &B));
    TLSQ_TRY(ws_get(h, WS_V, (size_t)N * N * 8, &Vw));
    TLSQ_TRY(ws_get(h, WS_LAM, (size_t)N * 8, &lamw));
    int64_t sw = 0;
    TLSQ_TRY(symeig_f64(h, G, N, ldG, (double*)B, (double*)Vw, V != nullptr, (double*)lamw, &sw));
    if (sweeps) *sweeps = sw;
    // sort descending on the host, permute V columns on the device
    std::vector<double> hl((size_t)N);
    TLSQ_HIP(h, hipMemcpyAsync(hl.data(), lamw, (size_t)N * 8, hipMemcpyDeviceToHost, h->stream));
    TLSQ_HIP(h, hipStreamSynchronize(h->stream));
    std::vector<int32_t> order((size_t)N);
    std::iota(order.begin(), order.end(), 0);
    std::stable_sort(order.begin(), order.end(), [&](int32_t a, int32_t b) { return hl[a] > hl[b]; });
    std::vector<double> sorted((size_t)N);
    for (int64_t i = 0; i < N; ++i) sorted[i] = hl[order[i]];
    TLSQ_HIP(h, hipMemcpyAsync(lam, sorted.data(), (size_t)N * 8, hipMemcpyHostToDevice, h->stream));
    if (V) {
        void *aux, *Vs;
        TLSQ_TRY(ws_get(h, WS_AUX0, (size_t)N * 16, &aux));
        TLSQ_TRY(ws_get(h, WS_VS, (size_t)N * N * 8, &Vs));
        TLSQ_HIP(h, hipMemcpyAsync(aux, order.data(), (size_t)N * 4, hipMemcpyHostToDevice, h->stream));
        TLSQ_TRY(launch_gather_scale(h, (const double*)Vw, N, (const int32_t*)aux, nullptr, N, nullptr,
                                     (double*)Vs));
        TLSQ_TRY(copy2d(h, V, ldV, Vs, N, N, N, 8, hipMemcpyDeviceToDevice));
    }
    TLSQ_HIP(h, hipStreamSynchronize(h->stream));
    return TLSQ_OK;
}
int tlsq_k_symeig_chol_f64(tlsq_handle h, const double* G, int64_t N, int64_t ldG, double* lam, double* V,
                           int64_t ldV, int64_t* sweeps) {
    TLSQ_TRY(check_handle(h));
    if (!G || !lam || !V || N <= 0 || ldG < N || ldV < N) return set_err(h, TLSQ_ERR_ARG, "symeig_chol: bad argument");
    void *B, *Vw, *lamw;
    TLSQ_TRY(ws_get(h, WS_B, (size_t)N * N * 8, &B));
    TLSQ_TRY(ws_get(h, WS_V, (size_t)N * N * 8, &Vw));
    TLSQ_TRY(ws_get(h, WS_LAM, (size_t)N * 8, &lamw));
    int64_t sw = 0;
    double delta = 0.0;
    // (as eig_full does it: the spectrum cut into slices first where the shape allows - sliced.hip, factor form, no hints)
    bool sliced = false, normwise = false;
    // (SLICE_NORMWISE=force, tests: the NORMWISE sliced form - what the returned `s` of rpca takes, certified to 8 N eps ||G||_F
    //  here since no tighter bound of lambda_max is at hand - so that it can be held to synthetic spectra by itself; lam comes
    //  back as the eigenvalues themselves there, not as singular values of a factor)
    if (symeig_sliced_ok(N) && ldG == N && dev_is(DEV_SLICE_NORMWISE, 'f')) {
        double st3[3];
        TLSQ_TRY(matfun_stats(h, G, N, st3));
        const double fro = std::sqrt(std::max(st3[0] + 2.0 * st3[1] - (double)N, 0.0));   // ||G||_F from ||G - I||_F^2 and the trace
        TLSQ_TRY(symeig_sliced_normwise_f64(h, G, N, (double*)Vw, (double*)lamw, &sw, fro, 0, 0.0, 0.0, &normwise));
    }
    if (!normwise && symeig_sliced_ok(N))
        TLSQ_TRY(symeig_sliced_f64(h, G, N, ldG, (double*)B, (double*)Vw, (double*)lamw, &delta, &sw, 0.0, 0, 0.0, 0.0, &sliced));
    if (!normwise && !sliced) TLSQ_TRY(symeig_chol_f64(h, G, N, ldG, (double*)B, (double*)Vw, (double*)lamw, &delta, &sw));
    if (sweeps) *sweeps = normwise ? -sw : sw;   // (negative: the normwise form served the call)
    std::vector<double> hl((size_t)N);
    TLSQ_HIP(h, hipMemcpyAsync(hl.data(), lamw, (size_t)N * 8, hipMemcpyDeviceToHost, h->stream));
    TLSQ_HIP(h, hipStreamSynchronize(h->stream));
    if (!normwise)
        for (auto& v : hl) v = std::max(v * v - delta, 0.0);
    std::vector<int32_t> order((size_t)N);
    std::iota(order.begin(), order.end(), 0);
    std::stable_sort(order.begin(), order.end(), [&](int32_t a, int32_t b) { return hl[a] > hl[b]; });
    std::vector<double> sorted((size_t)N);
    for (int64_t i = 0; i < N; ++i) sorted[i] = hl[order[i]];
    TLSQ_HIP(h, hipMemcpyAsync(lam, sorted.data(), (size_t)N * 8, hipMemcpyHostToDevice, h->stream));
    void *aux, *Vs;
    TLSQ_TRY(ws_get(h, WS_AUX0, (size_t)N * 16, &aux));
    TLSQ_TRY(ws_get(h, WS_VS, (size_t)N * N * 8, &Vs));
    TLSQ_HIP(h, hipMemcpyAsync(aux, order.data(), (size_t)N * 4, hipMemcpyHostToDevice, h->stream));
    TLSQ_TRY(launch_gather_scale(h, (const double*)Vw, N, (const int32_t*)aux, nullptr, N, nullptr, (double*)Vs));
    TLSQ_TRY(copy2d(h, V, ldV, Vs, N, N, N, 8, hipMemcpyDeviceToDevice));
    TLSQ_HIP(h, hipStreamSynchronize(h->stream));
    return TLSQ_OK;
}
int tlsq_k_tsqr_f64(tlsq_handle h, const double* Z, int64_t M, int64_t N, int64_t ldZ, double* R, int64_t ldR) {
    TLSQ_TRY(check_handle(h));
    if (!Z || !R || N <= 0 || M < N || ldZ < M || ldR < N) return set_err(h, TLSQ_ERR_ARG, "tsqr: bad argument (needs M >= N)");
    TLSQ_HIP(h, hipSetDevice(h->device));
    TLSQ_TRY(tsqr_r(h, Z, M, N, ldZ, R, ldR));
    TLSQ_HIP(h, hipStreamSynchronize(h->stream));
    return TLSQ_OK;
}
int tlsq_k_svd_r_f64(tlsq_handle h, const double* Z, int64_t M, int64_t N, int64_t ldZ, double* S, double* V,
                     int64_t ldV, int64_t* sweeps) {
    TLSQ_TRY(check_handle(h));
    if (!Z || !S || N <= 0 || M < N || ldZ < M || (V && ldV < N) || N > kFullEigMaxN)
        return set_err(h, TLSQ_ERR_ARG, "svd_r: bad argument (needs M >= N, N <= %lld)", (long long)kFullEigMaxN);
    TLSQ_HIP(h, hipSetDevice(h->device));
    SmallSvd s;
    double* Vw = nullptr;
    int64_t sw = 0;
    TLSQ_TRY(svd_via_r<double>(h, Z, M, N, ldZ, &Vw, s, &sw));
    if (sweeps) *sweeps = sw;
    std::vector<double> sorted((size_t)N);
    for (int64_t i = 0; i < N; ++i) sorted[i] = s.sigma[s.order[i]];
    TLSQ_HIP(h, hipMemcpyAsync(S, sorted.data(), (size_t)N * 8, hipMemcpyHostToDevice, h->stream));
    if (V) {
        void *aux, *Vs;
        TLSQ_TRY(ws_get(h, WS_AUX0, (size_t)N * 16, &aux));
        TLSQ_TRY(ws_get(h, WS_VS, (size_t)N * N * 8, &Vs));
        TLSQ_HIP(h, hipMemcpyAsync(aux, s.order.data(), (size_t)N * 4, hipMemcpyHostToDevice, h->stream));
        TLSQ_TRY(launch_gather_scale(h, (const double*)Vw, N, (const int32_t*)aux, nullptr, N, nullptr, (double*)Vs));
        TLSQ_TRY(copy2d(h, V, ldV, Vs, N, N, N, 8, hipMemcpyDeviceToDevice));
    }
    TLSQ_HIP(h, hipStreamSynchronize(h->stream));
    return TLSQ_OK;
}
int tlsq_k_opnorm_f64(tlsq_handle h, const double* Z, int64_t M, int64_t N, int64_t ldZ,
                      double* sigma_max) {
    TLSQ_TRY(check_handle(h));
    if (!Z || !sigma_max || N <= 0 || ldZ < M) return set_err(h, TLSQ_ERR_ARG, "opnorm: bad argument");
    return opnorm_gram<double>(h, Z, M, N, ldZ, sigma_max, nullptr);
}
int tlsq_k_maxabs_f64(tlsq_handle h, const double* x, int64_t n, double* out) {
    TLSQ_TRY(check_handle(h));
    if (!x || !out) return set_err(h, TLSQ_ERR_ARG, "maxabs: bad argument");
    return launch_maxabs<double>(h, x, n, out);
}

}  // extern "C"
