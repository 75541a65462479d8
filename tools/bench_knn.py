#!/usr/bin/env python3
"""Exact nearest-neighbour mode micro-bench (pgx_knn_batch_dev / pgx_match_nn_batch_dev) on the bench job's shape: F frames of
N descriptors resident in HBM, all F * (F - 1) / 2 image pairs.  Times, interleaved on the same box and stream (median over
--reps rounds of --steps calls each): k = 1; k = 2 with the column nearest; match_nn (k = 2, column nearest, selection); and
the greedy matcher (pgx_match_batch_dev) on the same sets.  Then one profiled pass per mode for the kernels' own times
(HIP event groups "knn", "knn_col", "knn_select", and the greedy's "ham_argmin" = k_ham_fp4).
kind = random (uniform descriptors) | true (frame f = a permuted copy of frame 0 with 15 % of the bits flipped)."""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.abspath(os.path.join(os.path.dirname(__file__), "..")))
import photogrammetry_amd as pg
from photogrammetry_amd import synth

FP4_PEAK_OPS = 10.0e15   # dense FP4 MFMA peak, as bench.py's k_ham_fp4 roofline


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--n", type=int, default=4096)
    ap.add_argument("--kind", default="random")
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--max-dist", type=int, default=64)
    ap.add_argument("--ratio", type=float, default=0.8)
    args = ap.parse_args()
    F, N = args.frames, args.n
    dev = torch.device("cuda", 0)
    eng = pg.Engine(0)
    stream = torch.cuda.Stream()   # a real stream: torch's default is the null stream, which the context's own does not order with
    eng.set_stream(stream.cuda_stream)
    if args.kind == "true":
        rng = np.random.default_rng(64)
        base = synth.random_descriptors(N, 8, 1)
        bits = np.unpackbits(base.view(np.uint8), axis=1)
        desc = np.stack([base] + [np.packbits(bits ^ (rng.random(bits.shape) < 0.15).astype(np.uint8), axis=1).view(np.uint32)
                                  [rng.permutation(N)] for _ in range(F - 1)])
    else:
        desc = np.random.default_rng(64).integers(0, 2**32, size=(F, N, 8), dtype=np.uint32)
    d_desc = torch.from_numpy(desc.view(np.int32)).to(dev)
    d_counts = torch.full((F,), N, dtype=torch.int32, device=dev)
    pl = [(i, j) for i in range(F) for j in range(i + 1, F)]
    M = len(pl)
    d_pl = torch.tensor(pl, dtype=torch.int32, device=dev)
    i32 = dict(dtype=torch.int32, device=dev)
    idx1, dist1 = torch.empty((M, N, 1), **i32), torch.empty((M, N, 1), **i32)
    idx2, dist2, col = torch.empty((M, N, 2), **i32), torch.empty((M, N, 2), **i32), torch.empty((M, N), **i32)
    out_nn, out_g = torch.empty((M, N, 3), **i32), torch.empty((M, N, 3), **i32)

    modes = {
        "knn_k1": lambda: eng.knn_batch_dev(d_desc, d_counts, N, 8, d_pl, M, 1, idx1, dist1),
        "knn_k2_col": lambda: eng.knn_batch_dev(d_desc, d_counts, N, 8, d_pl, M, 2, idx2, dist2, col),
        "match_nn": lambda: eng.match_nn_batch_dev(d_desc, d_counts, N, 8, d_pl, M, out_nn, args.max_dist, args.ratio, True),
        "greedy": lambda: eng.match_batch_dev(d_desc, d_counts, N, 8, d_pl, M, out_g),
    }
    torch.cuda.synchronize()
    for f in modes.values():   # warm-up: workspaces, code objects
        f()
    torch.cuda.synchronize()
    eng.check_status()

    times = {k: [] for k in modes}
    for _ in range(args.reps):   # interleaved: every round times every mode once
        for name, f in modes.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            for _ in range(args.steps):
                f()
            e1.record(stream)
            e1.synchronize()
            times[name].append(e0.elapsed_time(e1) / args.steps)
    eng.check_status()
    ms = {k: statistics.median(v) for k, v in times.items()}

    kern = {}
    for name, f in modes.items():   # one profiled pass per mode: the kernels' own times
        eng.profile_reset()
        eng.profile_enable(True)
        for _ in range(args.steps):
            f()
        torch.cuda.synchronize()
        eng.profile_enable(False)
        kern[name] = {}
        for g in ("knn", "knn_col", "knn_select", "match_init", "ham_argmin", "match_select", "tail_rows", "match_finish"):
            n, t = eng.profile_get(g)
            if n:
                kern[name][g] = round(t / args.steps, 4)
    eng.check_status()

    evals = M * N * N
    ops = evals * 512.0   # 2 * P ops per descriptor pair (the +-1 contraction), as bench.py counts k_ham_fp4
    k2 = kern["knn_k2_col"].get("knn")
    ham = kern["greedy"].get("ham_argmin")
    out = {"frames": F, "n": N, "pairs": M, "kind": args.kind, "steps": args.steps, "reps": args.reps,
           "ms_per_call": {k: round(v, 4) for k, v in ms.items()},
           "ms_per_call_all_reps": {k: [round(x, 4) for x in v] for k, v in times.items()},
           "kernels_ms": kern,
           "descriptor_pairs_per_s": {k: evals / (v * 1e-3) for k, v in ms.items()},
           "knn_k2_kernel_frac_of_fp4_peak": ops / (k2 * 1e-3) / FP4_PEAK_OPS if k2 else None,
           "knn_k2_call_frac_of_fp4_peak": ops / (ms["knn_k2_col"] * 1e-3) / FP4_PEAK_OPS,
           "ham_fp4_kernel_ms": ham,
           "knn_k2_kernel_over_ham_fp4": k2 / ham if k2 and ham else None,
           "match_nn_over_greedy": ms["match_nn"] / ms["greedy"],
           "match_nn_params": {"max_dist": args.max_dist, "ratio": args.ratio, "cross_check": 1},
           "accepted_per_pair_match_nn": float((out_nn[..., 1] >= 0).sum().item()) / M}
    print(json.dumps(out))
    eng.close()


if __name__ == "__main__":
    main()
