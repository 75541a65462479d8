#!/usr/bin/env python3
"""The scale pyramid (pgx_set_pyramid, csrc/k_pyramid.hip) measured at the bench job's shape: --frames frames of 1920 x 1080
resident in HBM, up to bench.NKP survivors per level.  One JSON line:

pyramid     for each mode in --modes (n_levels:step_q16), interleaved with the mode off in one process, median over --reps
            rounds of --steps detect-chain calls each:
              pyr_down     HIP event group "pyramid" (k_pyr_down, one launch per level), in total and per level -- level l's
                           time is the group's total with l + 1 levels minus its total with l levels -- with the bytes read
                           plus written (4 B per source and per destination pixel) over that time as a share of 8 TB/s;
              append       HIP event group "pyramid_append" (k_pyr_append, one launch per call);
              chain        the whole detect-chain call with the mode on and with it off (torch events around the calls);
              survivors    entries and raw hits per level over the frames (d_level_stats).
bench_off   bench.py's step time with the mode off -- the default path, which launches the kernels it always did -- and, with
            --parent-tree DIR (a built checkout of the commit to compare against), that checkout's bench.py alternating with
            this one in the same call (tools/bench_brief_steered.py's bench_off)."""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, ROOT)
import bench
import photogrammetry_amd as pg
from bench_brief_steered import bench_off, log

HBM_PEAK = 8.0e12


def measure(args, dev):
    F, w, h, nkp = args.frames, bench.W, bench.H, bench.NKP
    modes = [tuple(int(v) for v in m.split(":")) for m in args.modes.split(",")]
    eng = pg.Engine(0)
    stream = torch.cuda.Stream()   # a real stream: torch's default is the null stream, which the context's own does not order with
    eng.set_stream(stream.cuda_stream)
    eng.set_brief_pairs(pg.make_brief_pairs(0, 50, bench.P))
    eng.set_detect_params(bench.THRESH, bench.RADIUS)
    eng.set_capacity(1 << 18, nkp)                           # per level, as for the single scale
    d_base = torch.from_numpy(bench.base_frame(w, h, 0)).to(dev)
    d_frames = bench.roll_frames(torch, d_base, [(37 * k, 11 * k) for k in range(F)])
    i32 = dict(dtype=torch.int32, device=dev)
    max_levels = max(n for n, _ in modes)
    cap = max_levels * nkp                                   # the merged list holds every level's survivors
    d_kp, d_desc = torch.zeros((F, cap, 4), **i32), torch.zeros((F, cap, bench.WORDS), **i32)
    d_counts, d_nraw = torch.zeros(F, **i32), torch.zeros(F, **i32)
    d_origin, d_stats = torch.zeros((F, cap, 3), **i32), torch.zeros(F * 8 * 2, **i32)   # stats: [F][n_levels][2] of the mode
    torch.cuda.synchronize()

    def call(n_levels):
        if n_levels > 1:
            eng.detect_batch_pyramid_dev(d_frames, F, w, h, d_kp, d_desc, d_counts, d_nraw, cap, d_origin, d_stats)
        else:
            eng.detect_batch_dev(d_frames, F, w, h, d_kp, d_desc, d_counts, d_nraw, cap)

    def group_ms(name, n_levels):
        """ms per detect-chain call of one HIP event group"""
        eng.profile_filter(name)
        eng.profile_reset()
        eng.profile_enable(True)
        for _ in range(args.steps):
            call(n_levels)
        n, t = eng.profile_get(name)
        eng.profile_enable(False)
        return t / args.steps

    def chain_ms(n_levels):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        for _ in range(args.steps):
            call(n_levels)
        e1.record(stream)
        e1.synchronize()
        return e0.elapsed_time(e1) / args.steps

    res, stats = {}, {}
    for n, step in [(1, 92682)] + modes:                     # warm-up of every mode: workspaces, code objects; the counts
        eng.set_pyramid(n, step)
        call(n)
        eng.check_status()
        if n > 1:
            stats[(n, step)] = d_stats.cpu().numpy()[:F * n * 2].reshape(F, n, 2).copy()
    down = {m: {k: [] for k in range(2, m[0] + 1)} for m in modes}
    append = {m: [] for m in modes}
    chain = {m: [] for m in modes}
    chain_off = []
    for _ in range(args.reps):
        eng.set_pyramid(1, 92682)
        chain_off.append(chain_ms(1))
        for m in modes:
            n, step = m
            for k in range(2, n + 1):
                eng.set_pyramid(k, step)
                down[m][k].append(group_ms("pyramid", k))
            append[m].append(group_ms("pyramid_append", n))
            eng.profile_filter(None)
            chain[m].append(chain_ms(n))
    eng.check_status()
    eng.set_pyramid(1, 92682)
    eng.close()
    med = statistics.median
    for m in modes:
        n, step = m
        dims, _ = pg.pyramid_dims(w, h, n, step)
        tot = {k: med(v) for k, v in down[m].items()}
        tot[1] = 0.0
        levels, all_bytes = [], 0
        for l in range(1, n):
            ms = tot[l + 1] - tot[l]
            nbytes = 4 * F * (int(dims[l - 1, 0]) * int(dims[l - 1, 1]) + int(dims[l, 0]) * int(dims[l, 1]))
            all_bytes += nbytes
            levels.append({"level": l, "size": dims[l].tolist(), "ms": round(ms, 4), "bytes": nbytes,
                           "share_of_8TBps": round(nbytes / (ms * 1e-3) / HBM_PEAK, 3) if ms > 0 else None})
        st = stats[m]
        res["%d:%d" % m] = {
            "pyr_down_ms_total": round(tot[n], 4), "pyr_down_bytes": all_bytes,
            "pyr_down_share_of_8TBps": round(all_bytes / (tot[n] * 1e-3) / HBM_PEAK, 3),
            "pyr_down_levels": levels, "append_ms": round(med(append[m]), 4),
            "chain_ms": {"on": round(med(chain[m]), 4), "off": round(med(chain_off), 4),
                         "on_over_off": round(med(chain[m]) / med(chain_off), 3)},
            "survivors_per_level": {"min": st[:, :, 0].min(0).tolist(), "median": np.median(st[:, :, 0], 0).astype(int).tolist(),
                                    "max": st[:, :, 0].max(0).tolist()},
            "raw_hits_per_level_median": np.median(st[:, :, 1], 0).astype(int).tolist(),
            "merged_per_frame": [int(st[:, :, 0].sum(1).min()), int(st[:, :, 0].sum(1).max())]}
    return {"frames": F, "image": [w, h], "steps": args.steps, "reps": args.reps, "survivor_limit_per_level": nkp, "modes": res}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=bench.SEQ_FRAMES)
    ap.add_argument("--modes", default="4:92682,8:78643")
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--bench-steps", type=int, default=20)
    ap.add_argument("--bench-warmup", type=int, default=5)
    ap.add_argument("--bench-reps", type=int, default=2)
    ap.add_argument("--parent-tree", default=None, help="a built checkout of the commit to compare bench.py's step time against")
    ap.add_argument("--no-bench", action="store_true")
    args = ap.parse_args()
    out = {"pyramid": measure(args, torch.device("cuda", 0))}
    log("pyramid:", json.dumps(out["pyramid"]))
    if not args.no_bench:
        out["bench_off"] = bench_off(args)   # child processes: after this one's contexts are closed
    print(json.dumps(out))


if __name__ == "__main__":
    main()
