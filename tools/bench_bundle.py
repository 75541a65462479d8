"""Micro-benchmark of pgx_bundle_adjust_dev, timed with HIP events:
  (a) tools/bench_triangulate.py's shape (a): 64 frames (2 fixed, 62 free), 8000 tracks of 2..64 nodes
  (b) the same scene with 130 frames (2 fixed, 128 free: the largest reduced system), no target
Cameras and points are perturbed by synth.perturb; the call may run up to --iters LM iterations and stops by the contract's
tests (the iterations after the stop cost only their early-exit launches).  The per-iteration time is (the call's median -
the median of the same call with max_iters = 0) / the iterations it attempted.  Writes profiles/bundle_<shape>.json (or
--out DIR).  For the kernel split run it under `rocprofv3 --kernel-trace --stats -- python tools/bench_bundle.py`."""
import argparse
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, ROOT)
import geom_bench as gb  # noqa: E402
import photogrammetry_amd as pg  # noqa: E402
from geom_bench import F64, I32  # noqa: E402
from photogrammetry_amd import synth  # noqa: E402


def make_shape(rng, nf, n_points=8000):
    s, off, nodes, pts = gb.cut_scene(rng, nf, n_points)
    fixed = np.zeros(nf, np.int32)
    fixed[[0, nf - 1]] = 1
    Rt, X = synth.perturb(s["Rt"], s["points"][pts], seed=3, fixed=fixed)
    return gb.device_inputs(s["kps"], off, nodes, K=s["K"], Rt=Rt, fixed=fixed, X=X)


def bench(eng, d, steps, warmup, iters):
    nt, nf = d["n_tracks"], d["nf"]
    Rt_out, P_out, X_out = torch.empty((nf, 12), **F64), torch.empty((nf, 12), **F64), torch.empty((nt, 3), **F64)
    err, trace, report = torch.empty(nf * d["stride"], **F64), torch.empty((iters + 1, 2), **F64), torch.empty(8, **I32)
    torch.cuda.synchronize()

    def call():
        eng.bundle_adjust_dev(d["kp"], nf, d["stride"], nf, d["K"], d["Rt"], d["fixed"], d["off"], d["nodes"], d["tsum"], nt, d["X"],
                              Rt_out, P_out, X_out, trace, report, iters, float("inf"), 1e-3, d_node_err=err)
    return gb.time_on_stream(eng, call, steps, warmup), report.cpu().tolist(), trace.cpu().numpy()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--shapes", default="a,b")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles"))
    args = ap.parse_args()
    eng = pg.Engine(0)
    for name in args.shapes.split(","):
        rng = np.random.default_rng(0)
        t0 = time.time()
        d = make_shape(rng, 64 if name == "a" else 130)
        gen_s = time.time() - t0
        ms, report, trace = bench(eng, d, args.steps, args.warmup, args.iters)
        # the same call with max_iters = 0: setup, first linearisation and outputs, so that the per-iteration cost is the rest
        ms0, _, _ = bench(eng, d, args.steps, args.warmup, 0)
        its = max(report[0], 1)
        lens = d["lengths"]
        rec = dict(shape=name, frames=d["nf"], free_frames=report[3], unknowns_reduced=6 * report[3], tracks=d["n_tracks"],
                   nodes=d["n_nodes"], length_min=int(lens.min()), length_max=int(lens.max()), length_mean=float(lens.mean()),
                   max_iters=args.iters, steps=args.steps, report=report, cost_start=float(trace[0, 0]),
                   cost_end=float(trace[report[0], 0]), ms_median=float(np.median(ms)), ms_min=float(ms.min()),
                   ms_max=float(ms.max()), ms_setup_median=float(np.median(ms0)),
                   ms_per_iteration=float((np.median(ms) - np.median(ms0)) / its), input_generation_s=round(gen_s, 1),
                   target_ms_per_iteration=1.0 if name == "a" else None)
        gb.write_record(rec, args.out, "bundle")
    eng.close()


if __name__ == "__main__":
    main()
