"""numpy restatement of the reference's flts (src/flts.jl), statement by statement: the checker of the GPU path.

The only departure is the random p-subsets: `sample(inds, k, replace = false)` draws from Julia's global RNG, which no other
program reproduces, so the oracle draws through the library's host function tlsq_flts_subset (no GPU needed) - the very
draws the device makes.  Everything else follows the Julia text:
    rank(M)      count(svdvals > min(size)·eps(T)·σ₁)
    M \\ b        square: LU with partial pivoting (np.linalg.solve); tall: minimum-norm least squares
    sortperm     np.argsort(kind="stable")
"""
import ctypes as C

import numpy as np


def _lib():
    from tlsq_amd import _lib as L
    return L.load()


def draw(seed, s, attempt, n, k):
    J = np.zeros(k, dtype=np.int64)
    st = _lib().tlsq_flts_subset(int(seed), int(s), int(attempt), int(n), int(k), J.ctypes.data_as(C.POINTER(C.c_int64)))
    assert st == 0, st
    return J


def resolve_h(n, p, h, outliers):
    """:53-61 (Julia's round: ties to even, as Python's round)"""
    if round(0.5 * (n + p + 1)) <= h <= n:
        return h
    if 0.0 <= outliers <= 0.5:
        return int(round((1 - outliers) * n))
    return int(round(0.5 * (n + p + 1)))


def julia_rank(M):
    s = np.linalg.svd(M, compute_uv=False)
    if s.size == 0:
        return 0
    tol = min(M.shape) * np.finfo(M.dtype).eps * s[0]
    return int(np.count_nonzero(s > tol))


def backslash(M, b):
    if M.shape[0] == M.shape[1]:
        return np.linalg.solve(M, b)
    return np.linalg.lstsq(M, b, rcond=min(M.shape) * np.finfo(M.dtype).eps)[0]


def get_Q(A, y, H, theta):
    residuals = A @ theta - y
    return residuals[H] @ residuals[H]


def C_step(A, y, theta_old, h):
    residuals = A @ theta_old - y
    H_new = np.argsort(np.abs(residuals), kind="stable")[:h]
    theta_new = backslash(A[H_new, :], y[H_new])
    return H_new, theta_new, get_Q(A, y, H_new, theta_new)


def optimize_H(A, y, h, initial, maxiter, dQmin):
    Q_old = initial[2]
    opt = None
    for _ in range(maxiter):
        opt = C_step(A, y, initial[1], h)
        if Q_old - opt[2] < dQmin:
            break
        Q_old = opt[2]
    if opt is None:
        raise NameError("UndefVarError: opt not defined")
    return opt


def get_initial_H(A, y, p, n, h, seed, s, trace):
    J = draw(seed, s, 0, n, p)
    i = 1
    while (p + i + 1) < n and julia_rank(A[J, :]) < p:
        J = draw(seed, s, i, n, p + i)
        i += 1
    trace.setdefault("subset_rows", []).append(len(J))
    theta_J = backslash(A[J, :], y[J])
    return C_step(A, y, theta_J, h)


def flts(A, y, *, h=0, outliers=-1, N=500, maxiter=100, dQmin=1e-4, return_set=False, seed=0, trace=None):
    """trace (a dict, optional) receives subset_rows, q_stage2, candidates (subset indices) and q_final"""
    trace = {} if trace is None else trace
    A = np.asarray(A)
    y = np.asarray(y)
    n = len(y)
    if A.shape[0] != n:
        raise ValueError("DimensionMismatch: Both inputs A and y should have the same number of rows")
    if N < 10:
        raise ValueError("DomainError: N needs to be >= 10")
    if A.ndim == 1:
        A = A.reshape(-1, 1)
    p = A.shape[1]
    h = resolve_h(n, p, h, outliers)
    initials = [get_initial_H(A, y, p, n, h, seed, s, trace) for s in range(N)]
    opts = [optimize_H(A, y, h, x, 2, 0) for x in initials]
    trace["q_stage2"] = [o[2] for o in opts]
    order = sorted(range(N), key=lambda s: opts[s][2])          # sort! is stable
    candidates = [opts[s] for s in order[:10]]
    trace["candidates"] = order[:10]
    results = [optimize_H(A, y, h, x, maxiter, dQmin) for x in candidates]
    trace["q_final"] = [r[2] for r in results]
    w = sorted(range(10), key=lambda k: results[k][2])[0]
    trace["winner"] = order[w]
    winner = results[w]
    return winner if return_set else winner[1]


def paper_example(rng, f32=False):
    """test/runtests.jl:574-581: x = 10randn(1000), y = x + 2, rows 801:1000 replaced by outliers"""
    x = 10 * rng.standard_normal(1000)
    a, b = 1.0, 2.0
    y = a * x + b
    y[800:] = 5 * rng.standard_normal(200)
    x[800:] = 5 * rng.standard_normal(200) + 50
    xb = np.column_stack([x, np.ones(1000)])
    if f32:
        return xb.astype(np.float32), y.astype(np.float32), a, b
    return xb, y, a, b
