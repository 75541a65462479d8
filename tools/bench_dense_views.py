"""Micro-benchmark of pgx_dense_views_dev on tools/bench_triangulate.py's two shapes, timed with HIP
events on geom_bench's loop:
  (a) the bench graph's size: 64 frames, about 8 k tracks of 2..64 nodes
  (b) 1 M tracks of 2..4 nodes over 64 frames
The points and flags are pgx_triangulate_tracks_dev's of the same graph, every frame is a reference (64 x 64 cells: the pair
counts stay in LDS), S = 8.  The split into the stage's three parts comes from its profiling groups (pgx_profile_get),
measured in a second pass.  Writes profiles/dense_views_<shape>.json (or --out DIR)."""
import argparse
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, ROOT)
import bench_triangulate as bt  # noqa: E402
import geom_bench as gb  # noqa: E402
import photogrammetry_amd as pg  # noqa: E402
from geom_bench import F64, I32  # noqa: E402

PARTS = ("dense_views_nodes", "dense_views_pairs", "dense_views_select")


def bench(eng, d, steps, warmup, S, kw):
    nt, nf, N = d["n_tracks"], d["nf"], d["nf"] * d["stride"]
    xyz, q, tfl, tsum = torch.empty((nt, 3), **F64), torch.empty((nt, 3), **F64), torch.empty(nt, **I32), torch.empty(8, **I32)
    views, rng, st, rep = torch.empty((nf, 1 + S), **I32), torch.empty((nf, 2), **F64), torch.empty((nf, 4), **I32), torch.empty(8, **I32)
    pc = torch.empty((nf, nf, 2), **I32)
    torch.cuda.synchronize()
    eng.triangulate_tracks_dev(d["kp"], nf, d["stride"], nf, d["P"], d["off"], d["nodes"], d["tsum"], nt, xyz, q, tfl, tsum, 1.0, 2.0, 10)
    eng.check_status()

    def call():
        eng.dense_views_dev(d["off"], d["nodes"], d["tsum"], nt, N, xyz, nf, d["P"], nf, S, views, rng, st, rep, d_track_flags=tfl,
                            d_pair_counts=pc, **kw)
    ms = gb.time_on_stream(eng, call, steps, warmup)
    eng.profile_reset()
    eng.profile_enable(True)
    for _ in range(steps):
        call()
    eng.check_status()
    parts = {p: eng.profile_get(p)[1] / steps for p in PARTS}
    eng.profile_enable(False)
    return ms, parts, rep.cpu().tolist(), st.cpu().numpy(), rng.cpu().numpy()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--shapes", default="a,b")
    ap.add_argument("--sources", type=int, default=8)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles"))
    args = ap.parse_args()
    rng = np.random.default_rng(0)
    eng = pg.Engine(0)
    kw = dict(min_angle_deg=2.0, max_angle_deg=45.0, min_shared=8, min_points=8, q_near_pm=10, q_far_pm=990, grow=1.25)
    for name in args.shapes.split(","):
        t0 = time.time()
        kp, P, (off, nodes) = (bt.shape_a if name == "a" else bt.shape_b)(rng)
        d = gb.device_inputs(kp, off, nodes, P=P)
        gen_s = time.time() - t0
        ms, parts, report, stats, ranges = bench(eng, d, args.steps, args.warmup, args.sources, kw)
        lens = d["lengths"]
        rec = dict(shape=name, frames=d["nf"], stride=d["stride"], tracks=d["n_tracks"], nodes=d["n_nodes"],
                   length_min=int(lens.min()), length_max=int(lens.max()), length_mean=float(lens.mean()),
                   tracks_over_32=int((lens > 32).sum()), tracks_9_32=int(((lens > 8) & (lens <= 32)).sum()), steps=args.steps,
                   sources=args.sources, ms_median=float(np.median(ms)), ms_min=float(ms.min()), ms_max=float(ms.max()),
                   parts_ms={k: round(v, 4) for k, v in parts.items()}, report=report,
                   pairs_per_s=report[3] / (parts["dense_views_pairs"] * 1e-3) if parts["dense_views_pairs"] > 0 else None,
                   refs_flagged=int((stats[:, 3] != 0).sum()), range_first=ranges[0].tolist(),
                   input_generation_s=round(gen_s, 1), **kw)
        gb.write_record(rec, args.out, "dense_views")
    eng.close()


if __name__ == "__main__":
    main()
