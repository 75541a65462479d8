"""Micro-benchmark of pgx_track_consensus_dev on tools/bench_triangulate.py's two shapes, timed with
HIP events:
  (a) the bench graph's size: 64 frames, about 8 k tracks of 2..64 nodes
  (b) 1 M tracks of 2..4 nodes over 64 frames
A tenth of the tracks of three or more nodes carry one wrong observation (the keypoints of two tracks swapped in a frame
they share, or for shape (b) a keypoint moved by 200 px), so the compaction has work to do.  The yardstick is
pgx_triangulate_tracks_dev on the same graph and machine, timed by the same loop.  The split by part comes from the stage's
profiling groups (pgx_profile_get), measured in a second pass.  Writes profiles/consensus_<shape>.json (or --out DIR)."""
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

PARTS = ("consensus", "consensus_frames", "consensus_score", "consensus_scan", "consensus_write")


def plant(rng, name, kp, off, nodes):
    """one wrong observation in a tenth of the tracks of >= 3 nodes -> nodes"""
    nodes = np.array(nodes, dtype=np.int64).reshape(-1, 2)
    lens = np.diff(off)
    cand = np.flatnonzero(lens >= 3)
    hit = cand[rng.random(len(cand)) < 0.1]
    o = off[hit] + rng.integers(0, lens[hit])
    if name == "b":
        for f, k in nodes[o]:
            kp[f][k, 0] += 200
        return nodes
    # swap the keypoint with that of another hit observation in the same frame
    for f in np.unique(nodes[o, 0]):
        sel = o[nodes[o, 0] == f]
        sel = sel[: len(sel) // 2 * 2].reshape(-1, 2)
        nodes[sel[:, 0], 1], nodes[sel[:, 1], 1] = nodes[sel[:, 1], 1].copy(), nodes[sel[:, 0], 1].copy()
    return nodes


def bench(eng, d, steps, warmup, kw):
    nt, N = d["n_tracks"], d["nf"] * d["stride"]
    off2, nodes2, sum2, rep = torch.empty(nt + 1, **I32), torch.empty((N, 2), **I32), torch.empty(8, **I32), torch.empty(8, **I32)
    tmap, stats = torch.empty(nt, **I32), torch.empty((nt, 4), **I32)
    xyz, fl = torch.empty((nt, 3), **F64), torch.empty(nt, **I32)
    q, tfl, tsum = torch.empty((nt, 3), **F64), torch.empty(nt, **I32), torch.empty(8, **I32)
    torch.cuda.synchronize()

    def call():
        eng.track_consensus_dev(d["kp"], d["nf"], d["stride"], d["nf"], d["P"], d["off"], d["nodes"], d["tsum"], nt, off2, nodes2, sum2,
                                tmap, xyz, fl, stats, rep, **kw)

    def tri():
        eng.triangulate_tracks_dev(d["kp"], d["nf"], d["stride"], d["nf"], d["P"], d["off"], d["nodes"], d["tsum"], nt, xyz, q, tfl,
                                   tsum, 1.0, 2.0, 10)
    ms = gb.time_on_stream(eng, call, steps, warmup)
    ms_tri = gb.time_on_stream(eng, tri, steps, warmup)
    eng.profile_reset()
    eng.profile_enable(True)
    for _ in range(steps):
        call()
    eng.check_status()
    parts = {p: eng.profile_get(p)[1] / steps for p in PARTS}
    eng.profile_enable(False)
    return ms, ms_tri, parts, rep.cpu().tolist()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--shapes", default="a,b")
    ap.add_argument("--max-hyp", type=int, default=256)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles"))
    args = ap.parse_args()
    rng = np.random.default_rng(0)
    eng = pg.Engine(0)
    kw = dict(inlier_px=4.0, min_parallax_deg=1.0, min_inliers=2, min_len=2, max_hyp=args.max_hyp, seed=0)
    for name in args.shapes.split(","):
        t0 = time.time()
        kp, P, (off, nodes) = (bt.shape_a if name == "a" else bt.shape_b)(rng)
        if name == "a":
            kp = [np.stack([k["x"], k["y"]], 1).astype(np.int64) for k in kp]
        nodes = plant(rng, name, kp, np.asarray(off), nodes)
        d = gb.device_inputs(kp, off, nodes, P=P)
        gen_s = time.time() - t0
        ms, ms_tri, parts, report = bench(eng, d, args.steps, args.warmup, kw)
        lens = d["lengths"]
        rec = dict(shape=name, frames=d["nf"], stride=d["stride"], tracks=d["n_tracks"], nodes=d["n_nodes"],
                   length_min=int(lens.min()), length_max=int(lens.max()), length_mean=float(lens.mean()),
                   tracks_over_32=int((lens > 32).sum()), tracks_9_32=int(((lens > 8) & (lens <= 32)).sum()), steps=args.steps,
                   ms_median=float(np.median(ms)), ms_min=float(ms.min()), ms_max=float(ms.max()),
                   triangulate_ms_median=float(np.median(ms_tri)), parts_ms={k: round(v, 4) for k, v in parts.items()},
                   report=report, input_generation_s=round(gen_s, 1), **kw)
        gb.write_record(rec, args.out, "consensus")
    eng.close()


if __name__ == "__main__":
    main()
