#!/usr/bin/env python3
"""Vocabulary and pair-selection micro-bench (pgx_vocab_quantize_dev / pgx_vocab_train_dev / pgx_select_pairs_dev) on the bench
job's shape: F frames of N random descriptors resident in HBM, for every --vocab size V.  Times, interleaved on the same box
and stream (median over --reps rounds of --steps calls each): the quantiser alone, one training iteration (the call with
iters = 1 minus the call with iters = 0 is reported beside both), and the whole selection.  Then one profiled pass per mode
for the kernels' own times (HIP event groups "vocab_quantize", "vocab_train_init", "vocab_train_update", "select_hist",
"select_scores", "select_pick").  The quantiser's descriptor pairs per second (F * N * V per call) stand beside the k = 1 figure
of tools/bench_knn.py, which is the same arithmetic on the same operands."""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.abspath(os.path.join(os.path.dirname(__file__), "..")))
import photogrammetry_amd as pg

GROUPS = ("vocab_quantize", "vocab_train_init", "vocab_train_update", "select_hist", "select_scores", "select_pick")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--n", type=int, default=4096)
    ap.add_argument("--vocab", type=int, nargs="+", default=[4096, 65536])
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--top-k", type=int, default=10)
    args = ap.parse_args()
    F, N = args.frames, args.n
    dev = torch.device("cuda", 0)
    eng = pg.Engine(0)
    stream = torch.cuda.Stream()   # a real stream: torch's default is the null stream, which the context's own does not order with
    eng.set_stream(stream.cuda_stream)
    desc = np.random.default_rng(64).integers(0, 2**32, size=(F, N, 8), dtype=np.uint32)
    d_desc = torch.from_numpy(desc.view(np.int32)).to(dev)
    d_counts = torch.full((F,), N, dtype=torch.int32, device=dev)
    i32 = dict(dtype=torch.int32, device=dev)
    max_pairs = F * (F - 1) // 2
    word, wdist = torch.empty((F, N), **i32), torch.empty((F, N), **i32)
    d_pl, d_ps, d_sum, d_rep = torch.empty((max_pairs, 2), **i32), torch.empty((max_pairs,), **i32), torch.empty((8,), **i32), \
        torch.empty((4,), **i32)

    for V in args.vocab:
        d_vocab, d_scratch = torch.empty((V, 8), **i32), torch.empty((V, 8), **i32)
        torch.cuda.synchronize()
        eng.vocab_train_dev(d_desc, d_counts, F, N, V, d_vocab, d_rep, iters=0, seed=1)   # the vocabulary the other modes read
        modes = {
            "quantize": lambda: eng.vocab_quantize_dev(d_desc, d_counts, F, N, d_vocab, V, word, wdist),
            "train_iters0": lambda: eng.vocab_train_dev(d_desc, d_counts, F, N, V, d_scratch, d_rep, iters=0, seed=1),
            "train_iters1": lambda: eng.vocab_train_dev(d_desc, d_counts, F, N, V, d_scratch, d_rep, iters=1, seed=1),
            "select": lambda: eng.select_pairs_dev(d_desc, d_counts, F, N, d_vocab, V, max_pairs, d_pl, d_ps, d_sum, weighting=1,
                                                   top_k=args.top_k, window=0, min_score=1),
        }
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
            for g in GROUPS:
                n, t = eng.profile_get(g)
                if n:
                    kern[name][g] = round(t / args.steps, 4)
        eng.check_status()
        evals = F * N * V
        qk = kern["quantize"].get("vocab_quantize")
        out = {"frames": F, "n": N, "V": V, "steps": args.steps, "reps": args.reps, "top_k": args.top_k,
               "ms_per_call": {k: round(v, 4) for k, v in ms.items()},
               "ms_per_call_all_reps": {k: [round(x, 4) for x in v] for k, v in times.items()},
               "train_one_iteration_ms": round(ms["train_iters1"] - ms["train_iters0"], 4),
               "kernels_ms": kern,
               "quantize_descriptor_pairs_per_s_call": evals / (ms["quantize"] * 1e-3),
               "quantize_descriptor_pairs_per_s_kernel": evals / (qk * 1e-3) if qk else None,
               "pairs_selected": int(d_sum[0].item()), "of_pairs": max_pairs}
        print(json.dumps(out))
    eng.close()


if __name__ == "__main__":
    main()
