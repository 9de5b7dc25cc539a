"""flts on the GPU through the C ABI, against the reference's testset (test/runtests.jl:572-595) and the numpy oracle on the
same p-subset draws (tests/flts_oracle.py)."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import flts_oracle as O  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    # torch first: it ships its own HIP runtime, and whichever one is loaded first serves the whole process
    import torch
    assert torch.cuda.is_available()
    torch.zeros(1, device="cuda")
    import tlsq_amd
    e = tlsq_amd.Engine(0)
    yield e
    e.close()


def _design(rng, n, p, frac, mode):
    """y = A θ + noise with an intercept column (p >= 2); a fraction of rows are outliers: vertical (y shifted) or leverage
    (the regressors moved far out as well)"""
    A = rng.standard_normal((n, p)) if p == 1 else np.column_stack([rng.standard_normal((n, p - 1)), np.ones(n)])
    th = rng.uniform(-2, 2, p)
    y = A @ th + 0.1 * rng.standard_normal(n)
    k = int(frac * n)
    if k:
        rows = rng.choice(n, k, replace=False)
        y[rows] += 10 + 5 * rng.standard_normal(k)
        if mode == "leverage":
            A[rows, 0] += 20
    return (A[:, 0].copy() if p == 1 else A), y


def _parity(eng, A, y, N, seed=0, theta_tol=1e-10, f32=False):
    tr = {}
    H, th, Q = O.flts(A, y, N=N, return_set=True, seed=seed, trace=tr)
    (Hg, thg, Qg), rep = eng.flts(A, y, N=N, return_set=True, seed=seed, return_report=True)
    assert rep["h_mismatch"] == 0
    assert list(rep["subset_rows"]) == tr["subset_rows"]
    return (H, th, Q, tr), (Hg, thg, Qg, rep)


def _rel(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.max(np.abs(a - b)) / max(np.max(np.abs(b)), 1e-300))


def _same_top10(tr, rep):
    q = np.sort(np.asarray(tr["q_stage2"]))
    gaps = np.diff(q[:11]) / np.maximum(np.abs(q[1:11]), 1e-300)
    if np.all(gaps > 1e-12):
        assert list(rep["candidates"]) == tr["candidates"]


def test_reference_testset_f64(eng):
    rng = np.random.default_rng(11)
    xb, y, a, b = O.paper_example(rng)
    rt = np.sqrt(np.finfo(np.float64).eps)
    res = eng.flts(xb, y, verbose=True)
    assert np.isclose(res[0], a, rtol=rt, atol=0) and np.isclose(res[1], b, rtol=rt, atol=0)
    res1 = eng.flts(xb, y, N=10, outliers=0.20, verbose=True)
    assert np.isclose(res1[0], a, rtol=rt, atol=0) and np.isclose(res1[1], b, rtol=rt, atol=0)
    H, res2, Q = eng.flts(xb, y, N=10, h=800, return_set=True, verbose=True)
    assert np.isclose(res2[0], a, rtol=rt, atol=0) and np.isclose(res2[1], b, rtol=rt, atol=0)
    assert len(H) == 800 and np.all(H < 800)
    assert np.isclose(Q + 1, 1, rtol=rt, atol=0)


def test_reference_testset_f32(eng):
    rng = np.random.default_rng(12)
    xb, y, a, b = O.paper_example(rng, f32=True)
    rt = np.sqrt(np.finfo(np.float32).eps)
    res = eng.flts(xb, y)
    assert res.dtype == np.float32
    assert np.isclose(res[0], a, rtol=rt, atol=0) and np.isclose(res[1], b, rtol=rt, atol=0)
    H, res2, Q = eng.flts(xb, y, N=10, h=800, return_set=True)
    assert np.isclose(res2[0], a, rtol=rt, atol=0) and np.isclose(res2[1], b, rtol=rt, atol=0)
    assert np.all(H < 800)
    assert np.isclose(Q + 1, 1, rtol=rt, atol=0)


CASES = []
for n, ps, N in [(50, (1, 2, 5), 30), (1000, (1, 2, 5, 16, 33, 64), 30), (10007, (1, 5, 16, 64), 12), (200003, (2, 8, 33), 10)]:
    for i, p in enumerate(ps):
        frac, mode = [(0.0, "vertical"), (0.2, "vertical"), (0.45, "leverage"), (0.2, "leverage")][(i + n) % 4]
        CASES.append((n, p, N, frac, mode))


@pytest.mark.parametrize("n,p,N,frac,mode", CASES)
def test_parity_with_oracle(eng, n, p, N, frac, mode):
    rng = np.random.default_rng(n * 100 + p)
    A, y = _design(rng, n, p, frac, mode)
    (H, th, Q, tr), (Hg, thg, Qg, rep) = _parity(eng, A, y, N, seed=n + p)
    assert _rel(thg, th) < 1e-10, (thg, th)
    assert abs(Qg - Q) <= 1e-10 * abs(Q) + 1e-300
    assert np.array_equal(Hg, H)
    _same_top10(tr, rep)


def test_dummies_extend_the_draws(eng):
    rng = np.random.default_rng(5)
    n = 2000
    d1 = (rng.random(n) < 0.03).astype(float)
    d2 = (rng.random(n) < 0.05).astype(float)
    A = np.column_stack([np.ones(n), rng.standard_normal(n), d1, d2])
    y = A @ np.array([1.0, 2.0, -3.0, 4.0]) + 0.1 * rng.standard_normal(n)
    (H, th, Q, tr), (Hg, thg, Qg, rep) = _parity(eng, A, y, 40, seed=3)
    assert rep["rank_extended_draws"] > 0
    assert _rel(thg, th) < 1e-10 and np.array_equal(Hg, H)


def test_rank_deficient_design_gives_minimum_norm(eng):
    rng = np.random.default_rng(6)
    n = 120
    x = rng.standard_normal(n)
    A = np.column_stack([x, x, np.zeros(n), np.ones(n)])
    y = 3 * x + 1 + 0.05 * rng.standard_normal(n)
    H, th, Q = O.flts(A, y, N=10, return_set=True, seed=1)
    Hg, thg, Qg = eng.flts(A, y, N=10, return_set=True, seed=1)
    assert np.array_equal(np.sort(Hg), np.sort(H))
    mn = np.linalg.lstsq(A[Hg], y[Hg], rcond=None)[0]
    assert _rel(thg, mn) < 1e-8 and abs(thg[0] - thg[1]) < 1e-8 and thg[2] == 0.0


def test_fp32_parity(eng):
    rng = np.random.default_rng(8)
    A, y = _design(rng, 5000, 5, 0.2, "vertical")
    A32, y32 = A.astype(np.float32), y.astype(np.float32)
    H, th, Q = O.flts(A32, y32, N=20, return_set=True, seed=2)
    Hg, thg, Qg = eng.flts(A32, y32, N=20, return_set=True, seed=2)
    assert _rel(thg, th) < 1e-4
    assert abs(Qg - Q) <= 1e-3 * abs(Q)
    assert len(np.intersect1d(Hg, H)) >= 0.99 * len(H)


def test_scale_1e6(eng):
    rng = np.random.default_rng(9)
    A, y = _design(rng, 1_000_000, 8, 0.2, "leverage")
    (H, th, Q, tr), (Hg, thg, Qg, rep) = _parity(eng, A, y, 20, seed=4)
    assert _rel(thg, th) < 1e-10 and abs(Qg - Q) <= 1e-10 * Q
    assert np.array_equal(Hg, H)
    _same_top10(tr, rep)


def test_reproducible_and_device_pointers(eng):
    import torch
    rng = np.random.default_rng(10)
    A, y = _design(rng, 20000, 6, 0.2, "vertical")
    r1 = eng.flts(A, y, N=50, return_set=True)
    # easy data (the inliers fit exactly): any clean subset finds the same θ, whatever the draws
    Ae, ye = _design(rng, 20000, 6, 0.0, "vertical")
    ye = Ae @ np.arange(1.0, 7.0)
    ye[:4000] += 50.0
    e1 = eng.flts(Ae, ye, N=50)
    e2 = eng.flts(Ae, ye, N=50, seed=99)
    assert _rel(e2, e1) < 1e-10 and _rel(e1, np.arange(1.0, 7.0)) < 1e-10
    r2 = eng.flts(A, y, N=50, return_set=True)
    assert r1[1].tobytes() == r2[1].tobytes() and np.array_equal(r1[0], r2[0]) and r1[2] == r2[2]
    # device pointers
    from tlsq_amd import _lib as L
    dA = torch.from_numpy(np.asfortranarray(A).T.copy()).to("cuda:0")   # (p, n) row-major = column-major A
    dy = torch.from_numpy(y).to("cuda:0")
    dth = torch.zeros(6, dtype=torch.float64, device="cuda:0")
    dH = torch.zeros(len(r1[0]), dtype=torch.int64, device="cuda:0")
    dQ = torch.zeros(1, dtype=torch.float64, device="cuda:0")
    torch.cuda.synchronize()
    o = L.FltsOpts()
    eng.lib.tlsq_flts_opts_default(C.byref(o))
    o.nsub, o.memory = 50, L.MEM_DEVICE
    info = L.FltsInfo()
    st = eng.lib.tlsq_flts_f64(eng.h, C.c_void_p(dA.data_ptr()), 20000, 6, 20000, C.c_void_p(dy.data_ptr()), 20000, C.byref(o),
                               C.c_void_p(dth.data_ptr()), C.c_void_p(dH.data_ptr()), C.c_void_p(dQ.data_ptr()), C.byref(info))
    assert st == 0, eng.lib.tlsq_last_error(eng.h)
    assert dth.cpu().numpy().tobytes() == r1[1].tobytes()
    assert np.array_equal(dH.cpu().numpy(), r1[0]) and float(dQ.cpu()[0]) == r1[2]


def test_errors_leave_the_handle_usable(eng):
    from tlsq_amd import TlsqError
    from tlsq_amd import _lib as L
    rng = np.random.default_rng(13)
    A, y = _design(rng, 500, 3, 0.1, "vertical")
    cases = [(dict(A=A[:-1], y=y), L.TLSQ_ERR_ARG, "DimensionMismatch"), (dict(A=A, y=y, N=9), L.TLSQ_ERR_ARG, "N needs to be >= 10"),
             (dict(A=A, y=y, maxiter=0), L.TLSQ_ERR_ARG, "maxiter"),
             (dict(A=np.where(np.arange(500)[:, None] == 7, np.nan, A), y=y), L.TLSQ_ERR_NONFINITE, "Infs or NaNs"),
             (dict(A=rng.standard_normal((500, 65)), y=y), L.TLSQ_ERR_UNSUPPORTED, "at most 64")]
    for kw, code, msg in cases:
        with pytest.raises(TlsqError) as ei:
            eng.flts(**kw)
        assert ei.value.code == code and msg in str(ei.value), str(ei.value)
        th = eng.flts(A, y, N=10)
        assert np.all(np.isfinite(th))
