"""flts on the GPU: F1 (n = 1e6, p = 8, 20 % outliers, half of them high-leverage, N = 500, fp64; device and host pointers)
and F2 (the reference's 1000 x 2 example, N = 500), with the numpy oracle beside them (F2, and n = 1e5 with N = 500) and
the algorithmic work of one all-subset C-step computed from the shapes.  Prints one JSON line.

    python tools/bench_flts.py [--reps 5] [--no-oracle] [--out flts_bench.json]
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def f1_data(n, seed=0):
    rng = np.random.default_rng(seed)
    A = np.column_stack([rng.standard_normal((n, 7)), np.ones(n)])
    th = rng.uniform(-2, 2, 8)
    y = A @ th + 0.1 * rng.standard_normal(n)
    k = n // 5
    rows = rng.choice(n, k, replace=False)
    y[rows] += 10 + 5 * rng.standard_normal(k)
    A[rows[: k // 2], :7] += 20 * rng.standard_normal((k // 2, 7))
    return np.asfortranarray(A), y


def work(n, p, h, N, passes):
    """FLOPs and bytes of one all-subset C-step: `passes` residual passes (selection, gather, moments, Q) of 2p flops per
    row and subset, the masked moments (p(p+1)/2 + p products and adds per member), A read once per pass (fp64)"""
    flops = N * (passes * 2.0 * p * n + 2.0 * (p * (p + 1) / 2 + p) * h)
    bytes_ = passes * 8.0 * n * (p + 1)
    return flops, bytes_


def timed(fn, reps):
    import torch
    ts = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ts)), ts


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--no-oracle", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    import tlsq_amd
    from tlsq_amd import _lib as L
    import flts_oracle as O
    eng = tlsq_amd.Engine(0)
    out = {"config": {}}
    # ---- F1
    n, p, N = a.n, 8, 500
    A, y = f1_data(n)
    eng.flts(A, y, N=N)      # warm-up (code objects, workspace)
    host_ms, host_all = timed(lambda: eng.flts(A, y, N=N), a.reps)
    dA = torch.from_numpy(A.T.copy()).to("cuda:0")
    dy = torch.from_numpy(y).to("cuda:0")
    dth = torch.zeros(p, dtype=torch.float64, device="cuda:0")
    o = L.FltsOpts()
    eng.lib.tlsq_flts_opts_default(C.byref(o))
    o.nsub, o.memory = N, L.MEM_DEVICE
    info = L.FltsInfo()

    def dev_call():
        st = eng.lib.tlsq_flts_f64(eng.h, C.c_void_p(dA.data_ptr()), n, p, n, C.c_void_p(dy.data_ptr()), n, C.byref(o),
                                   C.c_void_p(dth.data_ptr()), None, None, C.byref(info))
        assert st == 0, eng.lib.tlsq_last_error(eng.h)

    dev_call()
    dev_ms, dev_all = timed(dev_call, a.reps)
    h = int(info.h)
    passes_per_cstep = info.select_passes / 3.0 + 3    # histogram passes + gather + moments + Q
    fl, by = work(n, p, h, N, passes_per_cstep)
    out["F1"] = {"n": n, "p": p, "N": N, "h": h, "device_ms": dev_ms, "host_ms": host_ms, "device_all": dev_all, "host_all": host_all,
                 "select_passes": int(info.select_passes), "cstep_gflop": fl / 1e9, "cstep_gbytes": by / 1e9,
                 "target_device_ms": 10.0, "theta": dth.cpu().numpy().tolist()}
    # ---- F2
    rng = np.random.default_rng(1)
    xb, y2, _, _ = O.paper_example(rng)
    eng.flts(xb, y2, N=500)
    f2_ms, f2_all = timed(lambda: eng.flts(xb, y2, N=500), max(a.reps, 10))
    out["F2"] = {"n": 1000, "p": 2, "N": 500, "ms": f2_ms, "all": f2_all, "target_ms": 1.0}
    if not a.no_oracle:
        t0 = time.perf_counter()
        O.flts(xb, y2, N=500)
        out["F2"]["oracle_ms"] = (time.perf_counter() - t0) * 1e3
        A5, y5 = f1_data(100_000, seed=2)
        t0 = time.perf_counter()
        O.flts(A5, y5, N=500)
        oracle5 = (time.perf_counter() - t0) * 1e3
        eng.flts(A5, y5, N=500)
        g5, _ = timed(lambda: eng.flts(A5, y5, N=500), a.reps)
        out["F1_1e5"] = {"n": 100_000, "p": 8, "N": 500, "oracle_ms": oracle5, "host_ms": g5}
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    eng.close()


if __name__ == "__main__":
    main()
