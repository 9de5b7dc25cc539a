"""Writes tests/golden/oracle_vectors.json — frozen outputs of the CPU oracle (oracle/rpca_oracle.py, once it had
passed the reference's own known-answer vectors) at BASELINE config C1 (500x50) and a shrunken C2 (2000x128),
SURVEY.md §8c item (6): per-iteration cost and svp, the singular values of the last Z, Frobenius norms and a
strided sample of A and E.  The inputs come from the seeded generator (a checksum of D guards against generator
drift).  These are DATA produced by this repo's oracle, not by the reference (Julia cannot run here).

The generator's low-rank product G1 G2 goes through BLAS, whose rounding depends on the CPU kernel and the thread count,
so D's bits differ between machines.  tests/golden/oracle_inputs.npz therefore freezes the exact D as well: per case, the
difference in ulps (int32, column-major) between D and `fixed_order_d`, a BLAS-free product that every machine rounds
alike.  The test rebuilds D from it bit for bit and checks it against the checksum.

    python tests/golden/make_oracle_vectors.py
"""
import hashlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from oracle import rpca_oracle as O  # noqa: E402

CASES = {"c1_500x50_r5": (500, 50, 5, 0), "c2s_2000x128_r8": (2000, 128, 8, 1)}
STRIDE = 97


def fixed_order_d(M, N, r, seed, S):
    """G1 G2 + S with the factors of O.synth_lowrank_sparse (its first two draws) and the rank-one terms added in order
    by elementwise numpy arithmetic (no BLAS, no FMA): the same bits on every machine.  Column-major."""
    rng = np.random.default_rng(seed)
    G1 = rng.standard_normal((M, r))
    G2 = rng.standard_normal((r, N))
    P = G1[:, :1] * G2[:1, :]
    for k in range(1, r):
        P = P + G1[:, k:k + 1] * G2[k:k + 1, :]
    return np.asfortranarray(P + S)


def main():
    out = {}
    ulps = {}
    for name, (M, N, r, seed) in CASES.items():
        D, _, S = O.synth_lowrank_sparse(M, N, r, seed=seed)
        d = np.asfortranarray(D).view(np.int64) - fixed_order_d(M, N, r, seed, S).view(np.int64)
        assert np.abs(d).max() < 2 ** 31
        ulps[name] = d.ravel(order="F").astype(np.int32)
        A, E, s, sv, info = O.rpca(D)
        out[name] = {
            "M": M, "N": N, "rank": r, "seed": seed,
            "D_sha256_of_float64_column_major": hashlib.sha256(np.asfortranarray(D).tobytes(order="F")).hexdigest(),
            "iters_done": info.iters_done, "sv": int(sv), "svp_hist": [int(v) for v in info.svp_hist],
            "cost_hist": [float(v) for v in info.cost_hist],
            "S": [float(v) for v in s[1]],
            "normA": float(np.linalg.norm(A)), "normE": float(np.linalg.norm(E)),
            "sample_stride": STRIDE,
            "A_sample": [float(v) for v in A.ravel(order="F")[::STRIDE]],
            "E_sample": [float(v) for v in E.ravel(order="F")[::STRIDE]],
        }
    here = os.path.dirname(os.path.abspath(__file__))
    with open(os.path.join(here, "oracle_vectors.json"), "w") as f:
        json.dump(out, f)
    np.savez_compressed(os.path.join(here, "oracle_inputs.npz"), **ulps)
    print({k: (v["iters_done"], v["sv"]) for k, v in out.items()})


if __name__ == "__main__":
    main()
