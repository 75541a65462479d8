"""Micro-benchmark of pgx_register_frames_dev, timed with HIP events on a stream of its own:
  (a) the bench graph's size: 64 frames (2 known, 62 targets), 8000 tracks of 2..64 nodes (about 4 k correspondences per
      target), n_samples = 1024
  (b) one target with about 50 k correspondences, n_samples = 4096
Points are the scene's true points; keypoints are make_scene's rounded projections.  Writes profiles/register_<shape>.json
(or --out DIR).  For the kernel split run it under `rocprofv3 --kernel-trace --stats -- python tools/bench_register.py`."""
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


def shape_a(rng):
    nf = 64
    s, off, nodes, pts = gb.cut_scene(rng, nf)
    reg = np.ones(nf, np.int32)
    reg[[0, nf - 1]] = 0
    return s, off, nodes, s["points"][pts], reg, 1024


def shape_b(rng):
    s = synth.make_scene(50000, 3, seed=2, arc_deg=20.0)
    off, nodes, pid = synth.scene_tracks(s, min_len=1)
    reg = np.array([0, 0, 1], np.int32)
    return s, off, nodes, s["points"][pid], reg, 4096


def bench(eng, d, steps, warmup, n_samples):
    nt, nf = d["n_tracks"], d["nf"]
    Rt_out, P_out = torch.empty((nf, 12), **F64), torch.empty((nf, 12), **F64)
    stats, ferr, report = torch.empty((nf, 4), **I32), torch.empty((nf, 2), **F64), torch.empty(8, **I32)
    torch.cuda.synchronize()

    def call():
        eng.register_frames_dev(d["kp"], nf, d["stride"], nf, d["K"], d["Rt"], d["reg"], d["off"], d["nodes"], d["tsum"], nt, d["X"],
                                Rt_out, P_out, stats, ferr, report, n_samples, 2.0, 12, 10, 1)
    ms = gb.time_on_stream(eng, call, steps, warmup)
    return ms, report.cpu().tolist(), stats.cpu().numpy(), Rt_out.cpu().numpy(), ferr.cpu().numpy()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=11)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--shapes", default="a,b")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles"))
    args = ap.parse_args()
    eng = pg.Engine(0)
    for name in args.shapes.split(","):
        rng = np.random.default_rng(0)
        t0 = time.time()
        s, off, nodes, X, reg, ns = (shape_a if name == "a" else shape_b)(rng)
        d = gb.device_inputs(s["kps"], off, nodes, K=s["K"], Rt=s["Rt"], reg=reg, X=X)
        gen_s = time.time() - t0
        ms, report, stats, Rt, ferr = bench(eng, d, args.steps, args.warmup, ns)
        tg = reg != 0
        cerr = max(float(np.abs(-Rt[f, :9].reshape(3, 3).T @ Rt[f, 9:] - s["centres"][f]).max()) for f in np.flatnonzero(tg))
        corr = stats[tg, 0]
        rec = dict(shape=name, frames=d["nf"], targets=int(tg.sum()), tracks=d["n_tracks"], nodes=d["n_nodes"],
                   correspondences_mean=float(corr.mean()), correspondences_max=int(corr.max()), n_samples=ns,
                   predicate_evaluations=int(4 * ns * corr.sum()), steps=args.steps, report=report,
                   max_centre_error=cerr, rms_px_max=float(np.nanmax(ferr[tg, 0])), ms_median=float(np.median(ms)),
                   ms_min=float(ms.min()), ms_max=float(ms.max()), input_generation_s=round(gen_s, 1),
                   target_ms=2.0 if name == "a" else None)
        gb.write_record(rec, args.out, "register")
    eng.close()


if __name__ == "__main__":
    main()
