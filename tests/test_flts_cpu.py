"""flts without a GPU: the host functions of the C ABI (h rule, subset draw, defaults), the struct mirrors, and the numpy
oracle against the reference's own flts testset (test/runtests.jl:572-595) and the optimize_H semantics (src/flts.jl:92-105)."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import flts_oracle as O  # noqa: E402
from tlsq_amd import _lib as L  # noqa: E402
from test_julia_shim_cpu import _header_struct, _julia_struct, julia_kind  # noqa: E402


def _resolve(n, p, h, outliers):
    hh = C.c_int64()
    rule = L.load().tlsq_flts_resolve_h(n, p, h, outliers, C.byref(hh))
    return rule, hh.value


@pytest.mark.parametrize("n,p,h,outliers", [(1000, 2, 0, -1), (1000, 2, 800, -1), (1000, 2, 10, 0.2), (1000, 2, 10, 0.6),
                                            (1000, 1, 0, -1), (999, 1, 0, -1), (1001, 2, 0, -1), (1000, 2, 1001, 0.25),
                                            (1000, 2, 0, 0.5), (1000, 2, 0, 0.0), (7, 3, 0, -1)])
def test_resolve_h_is_the_references_rule(n, p, h, outliers):
    rule, hh = _resolve(n, p, h, outliers)
    assert hh == O.resolve_h(n, p, h, outliers)
    assert rule == (0 if round(0.5 * (n + p + 1)) <= h <= n else (1 if 0 <= outliers <= 0.5 else 2))


def test_resolve_h_pinned_values():
    assert _resolve(1000, 2, 0, -1) == (2, 502)      # round(501.5) = 502: ties to even
    assert _resolve(1000, 2, 800, -1) == (0, 800)
    assert _resolve(1000, 2, 10, 0.2) == (1, 800)
    assert _resolve(1000, 2, 10, 0.6) == (2, 502)
    assert _resolve(1000, 1, 0, -1) == (2, 501)      # p = 1: round(501.0)
    assert _resolve(1000, 3, 0, -1) == (2, 502)      # round(502.0)
    assert L.load().tlsq_flts_resolve_h(0, 1, 0, -1.0, C.byref(C.c_int64())) == L.TLSQ_ERR_ARG


def test_subset_draws_distinct_in_range_deterministic():
    for n, k in [(10, 3), (1000, 8), (1000, 999), (50, 49), (7, 7), (1 << 20, 64)]:
        J = O.draw(0, 3, 0, n, k)
        assert len(J) == k and len(set(J.tolist())) == k
        assert J.min() >= 0 and J.max() < n
        assert np.array_equal(J, O.draw(0, 3, 0, n, k))
    a = O.draw(0, 0, 0, 10000, 20)
    assert not np.array_equal(a, O.draw(1, 0, 0, 10000, 20))
    assert not np.array_equal(a, O.draw(0, 1, 0, 10000, 20))
    assert not np.array_equal(a, O.draw(0, 0, 1, 10000, 20))
    lib = L.load()
    J = np.zeros(4, dtype=np.int64)
    assert lib.tlsq_flts_subset(0, 0, 0, 3, 4, J.ctypes.data_as(C.POINTER(C.c_int64))) == L.TLSQ_ERR_ARG   # k > n


def test_subset_draws_are_uniform():
    n, k, draws = 20, 3, 20000
    counts = np.zeros(n)
    for s in range(draws):
        counts[O.draw(7, s, 0, n, k)] += 1
    expect = draws * k / n
    chi2 = float(((counts - expect) ** 2 / expect).sum())
    assert chi2 < 60, chi2           # 19 degrees of freedom: p ~ 1e-5 at 50
    pairs = np.zeros((n, n))
    for s in range(draws):
        J = O.draw(9, s, 2, n, 2)
        pairs[J[0], J[1]] += 1
        pairs[J[1], J[0]] += 1
    off = pairs[~np.eye(n, dtype=bool)]
    assert off.min() > 0.5 * off.mean() and off.max() < 1.5 * off.mean()


def test_opts_default():
    o = L.FltsOpts()
    L.load().tlsq_flts_opts_default(C.byref(o))
    assert (o.h, o.outliers, o.nsub, o.maxiter, o.dQmin, o.seed, o.memory) == (0, -1.0, 500, 100, 1e-4, 0, L.MEM_HOST)
    assert C.sizeof(L.FltsOpts) == 48 and C.sizeof(L.FltsInfo) == 112


@pytest.mark.parametrize("jl_name,c_name,py_name", [("FltsOpts", "tlsq_flts_opts", "FltsOpts"),
                                                    ("FltsInfo", "tlsq_flts_info", "FltsInfo")])
def test_flts_struct_mirrors(jl_name, c_name, py_name):
    jf = _julia_struct(jl_name)
    hf = _header_struct(c_name)
    assert [n for n, _ in jf] == [n for n, _ in hf]
    for (jn, jt), (hn, hk) in zip(jf, hf):
        jk = "ptr" if jt.startswith("Ptr{") else julia_kind(jt)
        assert jk == hk, f"{jl_name}.{jn}: {jt} in the shim, {hk} in the header"
    pf = getattr(L, py_name)._fields_
    assert [n for n, _ in pf] == [n for n, _ in hf]
    for (pn, pt), (hn, hk) in zip(pf, hf):
        pk = "ptr" if isinstance(pt, type) and issubclass(pt, C._Pointer) else {
            C.c_int32: "i32", C.c_int64: "i64", C.c_uint64: "u64", C.c_double: "f64"}[pt]
        assert pk == hk, f"{py_name}.{pn}"


def test_oracle_passes_the_references_testset():
    rng = np.random.default_rng(1)
    xb, y, a, b = O.paper_example(rng)
    rt = np.sqrt(np.finfo(float).eps)
    res = O.flts(xb, y)
    assert np.isclose(res[0], a, rtol=rt, atol=0) and np.isclose(res[1], b, rtol=rt, atol=0)
    res1 = O.flts(xb, y, N=10, outliers=0.20)
    assert np.isclose(res1[0], a, rtol=rt, atol=0) and np.isclose(res1[1], b, rtol=rt, atol=0)
    H, res2, Q = O.flts(xb, y, N=10, h=800, return_set=True)
    assert np.isclose(res2[0], a, rtol=rt, atol=0) and np.isclose(res2[1], b, rtol=rt, atol=0)
    assert np.all(H < 800) and len(H) == 800
    assert np.isclose(Q + 1, 1, rtol=rt, atol=0)


def test_oracle_errors():
    rng = np.random.default_rng(0)
    xb, y, _, _ = O.paper_example(rng)
    with pytest.raises(ValueError, match="DimensionMismatch"):
        O.flts(xb[:-1], y)
    with pytest.raises(ValueError, match="DomainError"):
        O.flts(xb, y, N=9)
    with pytest.raises(NameError):
        O.flts(xb, y, N=10, maxiter=0)


def test_optimize_H_is_one_distinct_cstep():
    """optimize_H restarts every iteration from the initial θ: maxiter 1 and 100 agree, and the result equals an explicit
    chain - C(θ_J), C(θ₁) for every subset, C(θ₂) for the ten best."""
    rng = np.random.default_rng(3)
    n = 300
    A = np.column_stack([rng.standard_normal(n), rng.standard_normal(n), np.ones(n)])
    y = A @ np.array([1.0, -2.0, 0.5]) + 0.1 * rng.standard_normal(n)
    y[:60] += 20 * rng.standard_normal(60)
    t1, t100 = {}, {}
    r1 = O.flts(A, y, N=30, maxiter=1, return_set=True, seed=5, trace=t1)
    r100 = O.flts(A, y, N=30, maxiter=100, dQmin=-1.0, return_set=True, seed=5, trace=t100)
    assert np.array_equal(r1[0], r100[0]) and np.array_equal(r1[1], r100[1]) and r1[2] == r100[2]
    assert t1["candidates"] == t100["candidates"]
    # the explicit chain
    h = O.resolve_h(n, 3, 0, -1)
    chains = []
    for s in range(30):
        J = O.draw(5, s, 0, n, 3)
        i = 1
        while (3 + i + 1) < n and O.julia_rank(A[J]) < 3:
            J = O.draw(5, s, i, n, 3 + i)
            i += 1
        c1 = O.C_step(A, y, O.backslash(A[J], y[J]), h)
        chains.append(O.C_step(A, y, c1[1], h))
    order = sorted(range(30), key=lambda s: chains[s][2])
    assert order[:10] == t1["candidates"]
    third = [O.C_step(A, y, chains[s][1], h) for s in order[:10]]
    w = sorted(range(10), key=lambda k: third[k][2])[0]
    assert np.array_equal(third[w][0], r1[0]) and np.array_equal(third[w][1], r1[1]) and third[w][2] == r1[2]
