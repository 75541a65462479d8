"""Micro-benchmark of pgx_triangulate_tracks_dev on two shapes, timed with HIP events:
  (a) the bench graph's size: 64 frames, about 8 k tracks of 2..64 nodes, about 240 k nodes
  (b) 1 M tracks of 2..4 nodes over 64 frames
Tracks are true tracks of synthetic scenes (synth.make_scene's cameras; rounded projections), so most points are valid and
every refinement step runs.  Writes profiles/triangulate_<shape>.json (or --out DIR).  For the kernel split run it under
`rocprofv3 --kernel-trace --stats -- python tools/bench_triangulate.py`."""
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


def shape_a(rng, nf=64, n_points=8000):
    s, off, nodes, _ = gb.cut_scene(rng, nf, n_points)
    return s["kps"], s["P"], (off, nodes)


def shape_b(rng, nf=64, n_tracks=1 << 20):
    s = synth.make_scene(1, nf, seed=2, arc_deg=120.0)
    P = s["P"].reshape(nf, 3, 4)
    L = rng.integers(2, 5, size=n_tracks)
    start = rng.integers(0, nf - L + 1)
    X = rng.uniform(-1.5, 1.5, size=(n_tracks, 3))
    t_of = np.repeat(np.arange(n_tracks), L)
    off = np.concatenate([[0], np.cumsum(L)])
    frames = start[t_of] + (np.arange(len(t_of)) - off[t_of])
    h = np.einsum("nij,nj->ni", P[frames, :, :3], X[t_of]) + P[frames, :, 3]
    uv = np.round(h[:, :2] / h[:, 2:3]).astype(np.int64)
    order = np.argsort(frames, kind="stable")
    counts = np.bincount(frames, minlength=nf)
    first = np.concatenate([[0], np.cumsum(counts)])[:-1]
    kidx = np.empty(len(frames), np.int64)
    kidx[order] = np.arange(len(frames)) - first[frames[order]]
    kp = [np.zeros((counts[f], 2), np.int64) for f in range(nf)]
    for f in range(nf):
        sel = order[first[f]:first[f] + counts[f]]
        kp[f][kidx[sel]] = uv[sel]
    nodes = np.stack([frames, kidx], 1)
    return kp, s["P"], (off, nodes)


def bench(eng, d, steps, warmup, iters, min_par, max_e):
    nt = d["n_tracks"]
    xyz, q = torch.empty((nt, 3), **F64), torch.empty((nt, 3), **F64)
    fl, summ = torch.empty(nt, **I32), torch.empty(8, **I32)
    err = torch.empty(d["n_nodes"], **F64)
    torch.cuda.synchronize()

    def call():
        eng.triangulate_tracks_dev(d["kp"], d["nf"], d["stride"], d["nf"], d["P"], d["off"], d["nodes"], d["tsum"], nt, xyz, q, fl,
                                   summ, min_par, max_e, iters, d_node_err=err)
    return gb.time_on_stream(eng, call, steps, warmup), summ.cpu().tolist()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--shapes", default="a,b")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles"))
    args = ap.parse_args()
    rng = np.random.default_rng(0)
    eng = pg.Engine(0)
    for name in args.shapes.split(","):
        t0 = time.time()
        kp, P, (off, nodes) = (shape_a if name == "a" else shape_b)(rng)
        d = gb.device_inputs(kp, off, nodes, P=P)
        gen_s = time.time() - t0
        ms, summary = bench(eng, d, args.steps, args.warmup, args.iters, 1.0, 2.0)
        lens = d["lengths"]
        rec = dict(shape=name, frames=d["nf"], stride=d["stride"], tracks=d["n_tracks"], nodes=d["n_nodes"],
                   length_min=int(lens.min()), length_max=int(lens.max()), length_mean=float(lens.mean()),
                   tracks_over_32=int((lens > 32).sum()), tracks_9_32=int(((lens > 8) & (lens <= 32)).sum()),
                   refine_iters=args.iters, min_parallax_deg=1.0, max_reproj_px=2.0, steps=args.steps,
                   ms_median=float(np.median(ms)), ms_min=float(ms.min()), ms_max=float(ms.max()), summary=summary,
                   input_generation_s=round(gen_s, 1), target_ms=0.05 if name == "a" else 1.0)
        gb.write_record(rec, args.out, "triangulate")
    eng.close()


if __name__ == "__main__":
    main()
