"""Whole solves without the host-visible mailbox (NO_MAILBOX=1): every small result then comes back through a copy into the
handle's pinned buffer and a stream synchronisation - the read-back path the library also falls back to when the mapped
allocation fails or a mailbox poll times out.  Against the CPU oracle at the bars of tests/test_gpu_parity.py, and against the
same call with the mailbox: the same device doubles travel either way, so A, E, the iteration count and the rank trajectory
are the same bits.

The set-up of rpca queues its max |D| pass on the second stream and reads the result after the Lanczos run of opnorm(D)
(src/robustPCA.jl:177-179).  Without the mailbox that Lanczos run copies 64 + 16 (N + 2) bytes to the front of the pinned
buffer, from N = 123 on past byte 2048; the max |D| word must not lie in that range, or norm(D, Inf) / lambda - which decides
dual_norm when one entry dominates - is a Lanczos coefficient instead.  N = 122 / 123 sit on both sides of that size."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

NS = [64, 122, 123, 256, 512, 1024]
_ORACLE = {}


@pytest.fixture(scope="module")
def eng():
    import torch  # noqa: F401
    import tlsq_amd
    e = tlsq_amd.Engine(0)
    yield e
    e.close()


def relerr(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return np.linalg.norm(a - b) / np.linalg.norm(b)


def _panel(N, dtype, dominant):
    """M = 3N + 7 rows: low rank plus sparse as in test_gpu_parity._compare_with_oracle; `dominant` adds one entry of 1e3,
    so that norm(D, Inf) / lambda = 1e3 sqrt(M) is far above opnorm(D) and sets dual_norm (:179)."""
    from oracle import rpca_oracle as O
    M = 3 * N + 7
    D = O.synth_lowrank_sparse(M, N, 4 + N // 64, seed=N)[0]
    if dominant:
        D[M // 3, N // 2] = 1e3
    return np.asarray(D, dtype=dtype)


def _oracle(N, dtype, dominant):
    from oracle import rpca_oracle as O
    key = (N, np.dtype(dtype).name, dominant)
    if key not in _ORACLE:
        _ORACLE[key] = O.rpca(_panel(N, dtype, dominant))
    return _ORACLE[key]


def _cases():
    for dt in (np.float64, np.float32):
        for N in NS:
            for dominant in (False, True):
                if N == 1024 and (dt == np.float32 or dominant):
                    continue          # (the CPU oracle's time: the largest panel once, fp64, first fixture)
                for ch in (True, False):
                    yield pytest.param(N, dt, dominant, ch, id=f"{np.dtype(dt).name}-N{N}-{'dominant' if dominant else 'plain'}-"
                                                               f"{'cost' if ch else 'nocost'}")


@pytest.mark.parametrize("N,dtype,dominant,cost_history", list(_cases()))
def test_rpca_without_the_mailbox_vs_oracle_and_mailbox(eng, N, dtype, dominant, cost_history):
    """rpca under NO_MAILBOX=1 against the oracle (fp64: iterations, converged, rank trajectory, cost history, A and E to 1e-8;
    fp32: the fp32 bar of test_rpca_f32_vs_oracle - iterations within one, A and E to 1e-3) and against the same call with the
    mailbox: A, E, iters_done and svp_hist bit-identical.  The returned `s` is compared to 1e-10 (fp64), not bit for bit: with
    the mailbox the E-free loop speculates and keeps Z_k itself, without it the loop runs in line and rebuilds Z_k as
    A_k + Y_{k+1} / mu_k (the same split test_gpu_parity.py's speculative-loop test makes).  cost_history=False settles the
    cost test by power steps with the mailbox and by Lanczos without it: the trajectory must not depend on which.
    N = 1024 (rank 20) is the one panel whose subspace block is wider than 32 columns: there the cold step of the subspace solver
    orthonormalises with CholeskyQR2 when its status can come back through the mailbox and with CGS2 otherwise (svdstep.hip,
    `cold_chol`) - another rounding of the same iterates, so A and E agree to 1e-13 instead of bit for bit, with the same
    iterations and rank trajectory."""
    import warnings
    import tlsq_amd
    D = _panel(N, dtype, dominant)
    Ao, Eo, so, svo, io = _oracle(N, dtype, dominant)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        with tlsq_amd.dev_switches(NO_MAILBOX=1):
            A, E, s, sv, rep = eng.rpca(D, return_report=True, cost_history=cost_history)
        A1, E1, s1, sv1, rep1 = eng.rpca(D, return_report=True, cost_history=cost_history)
    assert A.dtype == dtype and E.dtype == dtype
    if N < 1024:
        assert np.array_equal(A, A1) and np.array_equal(E, E1), (relerr(A, A1), relerr(E, E1))
    else:
        assert relerr(A, A1) <= 1e-13 and relerr(E, E1) <= 1e-13, (relerr(A, A1), relerr(E, E1))
    assert (sv, rep.iters_done, rep.svp_hist, rep.converged) == (sv1, rep1.iters_done, rep1.svp_hist, rep1.converged)
    assert sv == svo and rep.converged == io.converged
    if dtype == np.float64:
        assert rep.iters_done == io.iters_done and rep.svp_hist == io.svp_hist, (rep.svp_hist, io.svp_hist)
        if cost_history:
            assert np.allclose(rep.cost_hist, io.cost_hist, rtol=1e-6, atol=1e-12)
        assert relerr(A, Ao) <= 1e-8 and relerr(E, Eo) <= 1e-8, (relerr(A, Ao), relerr(E, Eo))
        np.testing.assert_allclose(s.S, s1.S, rtol=1e-10, atol=1e-13 * s1.S[0])
    else:
        assert abs(rep.iters_done - io.iters_done) <= 1, (rep.iters_done, io.iters_done)
        assert relerr(A, Ao) < 1e-3 and relerr(E, Eo) < 1e-3, (relerr(A, Ao), relerr(E, Eo))
        np.testing.assert_allclose(s.S, s1.S, rtol=0, atol=1e-5 * s1.S[0])
    if dominant:
        assert E[(3 * N + 7) // 3, N // 2] != 0          # the dominant entry is an outlier, as in the oracle
        assert Eo[(3 * N + 7) // 3, N // 2] != 0


@pytest.mark.parametrize("N", [123, 512])
def test_poisoned_workspace_without_the_mailbox(eng, N):
    """WS_POISON=1 (every workspace slot refilled with NaN bytes at the start of the call) together with NO_MAILBOX=1 on the
    dominant-entry panel: the call succeeds - no NaN read back as max |D| - with the bits of the plain call."""
    import tlsq_amd
    D = _panel(N, np.float64, True)
    A1, E1, s1, sv1, rep1 = eng.rpca(D, return_report=True)
    try:
        tlsq_amd.dev_set("WS_POISON", 1)
        with tlsq_amd.dev_switches(NO_MAILBOX=1):
            A, E, s, sv, rep = eng.rpca(D, return_report=True)
    finally:
        tlsq_amd.dev_set("WS_POISON", None)
    assert np.array_equal(A, A1) and np.array_equal(E, E1)
    assert (sv, rep.iters_done, rep.svp_hist) == (sv1, rep1.iters_done, rep1.svp_hist)


# ---- the other callers of the pinned read-backs, once each -----------------------------------------------------------------
def test_rtls_without_the_mailbox(eng):
    """rtls (src/TotalLeastSquares.jl:152-156) at test_tls_and_rtls's oracle bar."""
    import tlsq_amd
    from oracle import rpca_oracle as O
    rng = np.random.default_rng(11)
    for _ in range(4):
        x = rng.standard_normal(3)
        A = rng.standard_normal((50, 3))
        An = A + 50 * rng.standard_normal(A.shape) * (rng.random(A.shape) < 0.1)
        yn = A @ x + 50 * rng.standard_normal(50) * (rng.random(50) < 0.1)
        with tlsq_amd.dev_switches(NO_MAILBOX=1):
            xr = eng.rtls(An, yn)
        assert np.allclose(xr, O.rtls(An, yn), rtol=1e-6, atol=1e-8)
        assert np.allclose(xr, eng.rtls(An, yn), rtol=1e-10, atol=1e-12)   # (tls!(s, n) on the last SVD: `s` above)


def test_robust_lowrankfilter_lazy_hankel_without_the_mailbox(eng):
    """lowrankfilter(y, 256) on a short series: the robust branch on the implicit (lazy) Hankel panel, against the oracle's
    filter to 1e-8 and the mailbox run's iterations and rank trajectory."""
    import tlsq_amd
    from oracle import rpca_oracle as O
    y, noise = O.synth_series(6000, seed=8)
    x = y + noise
    with tlsq_amd.dev_switches(NO_MAILBOX=1):
        yf, rep = eng.lowrankfilter(x, 256, return_report=True)
    yf1, rep1 = eng.lowrankfilter(x, 256, return_report=True)
    assert (rep.iters_done, rep.svp_hist, rep.converged) == (rep1.iters_done, rep1.svp_hist, rep1.converged)
    assert relerr(yf, yf1) <= 1e-12
    assert relerr(yf, O.lowrankfilter(x, 256)) < 1e-8


def test_rpca_hankel_flag_without_the_mailbox(eng):
    """rpca(H; hankel=true) at test_rpca_hankel_flag_vs_oracle's bar."""
    import tlsq_amd
    from oracle import rpca_oracle as O
    Ny, L = 3000, 64
    rng = np.random.default_rng(Ny + L)
    t = np.arange(Ny)
    y = np.sin(0.1 * t) + 0.3 * np.sin(0.37 * t) + 0.05 * rng.standard_normal(Ny)
    y[rng.random(Ny) < 0.02] += 5.0
    H = O.hankel(y, L)
    with tlsq_amd.dev_switches(NO_MAILBOX=1):
        A, E, s, sv, rep = eng.rpca(H, nukeA=False, hankel=True, iters=200, return_report=True)
    Ao, Eo, so, svo, io = O.rpca(H, nukeA=False, hankel=True, iters=200)
    assert rep.iters_done == io.iters_done and rep.svp_hist == io.svp_hist and sv == svo
    assert rep.converged == io.converged
    assert relerr(A, Ao) < 1e-8 and relerr(E, Eo) < 1e-8
    assert tlsq_amd.ishankel(A) == O.ishankel(Ao) and tlsq_amd.ishankel(E) == O.ishankel(Eo)


def test_loopback_group_without_the_mailbox():
    """A two-rank loop-back group (test_gpu_multi.py: the same device named twice, a host-staged communicator) against the
    plain handle and the oracle at test_loopback_rpca_rank_gt_1_vs_plain_and_oracle's bars."""
    import tlsq_amd
    from oracle import rpca_oracle as O
    D = O.synth_lowrank_sparse(1500, 96, 6, seed=1500)[0]
    D[500, 48] = 1e3
    plain = tlsq_amd.Engine(0)
    multi = tlsq_amd.Engine(devices=[0, 0])
    try:
        assert multi.ngpus == 2
        with tlsq_amd.dev_switches(NO_MAILBOX=1):
            A1, E1, s1, sv1, rep1 = plain.rpca(D, return_report=True)
            A2, E2, s2, sv2, rep2 = multi.rpca(D, return_report=True)
    finally:
        multi.close()
        plain.close()
    assert rep2.iters_done == rep1.iters_done and rep2.svp_hist == rep1.svp_hist and sv2 == sv1
    assert relerr(A2, A1) < 1e-9 and relerr(E2, E1) < 1e-9
    assert np.allclose(rep2.cost_hist, rep1.cost_hist, rtol=1e-6, atol=1e-12)
    Ao, Eo, so, svo, io = O.rpca(D)
    for A, E, s, rep in ((A1, E1, s1, rep1), (A2, E2, s2, rep2)):
        assert rep.iters_done == io.iters_done and rep.svp_hist == io.svp_hist
        assert relerr(A, Ao) < 1e-8 and relerr(E, Eo) < 1e-8
        assert np.allclose(s.S, so[1], rtol=1e-10, atol=64 * 2.2e-16 * np.sqrt(96) * so[1][0])
