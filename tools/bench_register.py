"""Micro-benchmark of pgx_register_frames_dev, timed with HIP events on a stream of its own:
  (a) the bench graph's size: 64 frames (2 known, 62 targets), 8000 tracks of 2..64 nodes (about 4 k correspondences per
      target), n_samples = 1024
  (b) one target with about 50 k correspondences, n_samples = 4096
Points are the scene's true points; keypoints are make_scene's rounded projections.  Writes profiles/register_<shape>.json
(or --out DIR).  For the kernel split run it under `rocprofv3 --kernel-trace --stats -- python tools/bench_register.py`."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, ROOT)
import photogrammetry_amd as pg  # noqa: E402
from photogrammetry_amd import synth  # noqa: E402

DEV = "cuda:0"


def shape_a(rng):
    nf = 64
    s = synth.make_scene(8000, nf, seed=1, arc_deg=120.0)
    seen = {}
    for f, pid in enumerate(s["point_id"]):
        for k, p in enumerate(pid):
            seen.setdefault(int(p), []).append((f, k))
    tracks, pts = [], []
    for p in sorted(seen):
        v = seen[p]
        L = min(len(v), int(rng.integers(2, 65)))
        if L < 2:
            continue
        a = int(rng.integers(0, len(v) - L + 1))
        tracks.append(v[a:a + L])
        pts.append(p)
    reg = np.ones(nf, np.int32)
    reg[[0, nf - 1]] = 0
    return s, tracks, s["points"][pts], reg, 1024


def shape_b(rng):
    s = synth.make_scene(50000, 3, seed=2, arc_deg=20.0)
    off, nodes, pid = synth.scene_tracks(s, min_len=1)
    tracks = [[tuple(n) for n in nodes[off[t]:off[t + 1]]] for t in range(len(off) - 1)]
    reg = np.array([0, 0, 1], np.int32)
    return s, tracks, s["points"][pid], reg, 4096


def device_inputs(s, tracks, X, reg):
    off = np.concatenate([[0], np.cumsum([len(t) for t in tracks])])
    nodes = np.array([n for t in tracks for n in t])
    nf = len(s["kps"])
    stride = max(len(k) for k in s["kps"])
    buf = np.zeros((nf, stride), dtype=pg.KEYPOINT_DTYPE)
    for f, k in enumerate(s["kps"]):
        buf[f, :len(k)] = k
    i32, f64 = dict(dtype=torch.int32, device=DEV), dict(dtype=torch.float64, device=DEV)
    return dict(kp=torch.from_numpy(buf.view(np.int32).reshape(nf, stride, 4)).to(DEV), K=torch.from_numpy(s["K"]).to(DEV),
                Rt=torch.from_numpy(s["Rt"]).to(DEV), reg=torch.from_numpy(reg).to(DEV), X=torch.from_numpy(np.asarray(X)).to(DEV),
                off=torch.from_numpy(off.astype(np.int32)).to(DEV), nodes=torch.from_numpy(nodes.astype(np.int32)).to(DEV),
                tsum=torch.tensor([len(off) - 1, len(nodes), 0, 0, 0, 0, 0, 0], **i32), nf=nf, stride=stride, n_tracks=len(off) - 1,
                n_nodes=len(nodes), lengths=np.diff(off), f64=f64, i32=i32, true_Rt=s["Rt"], centres=s["centres"])


def bench(eng, d, steps, warmup, n_samples):
    nt, nf, f64, i32 = d["n_tracks"], d["nf"], d["f64"], d["i32"]
    Rt_out, P_out = torch.empty((nf, 12), **f64), torch.empty((nf, 12), **f64)
    stats, ferr, report = torch.empty((nf, 4), **i32), torch.empty((nf, 2), **f64), torch.empty(8, **i32)
    torch.cuda.synchronize()

    def call():
        eng.register_frames_dev(d["kp"], nf, d["stride"], nf, d["K"], d["Rt"], d["reg"], d["off"], d["nodes"], d["tsum"], nt, d["X"],
                                Rt_out, P_out, stats, ferr, report, n_samples, 2.0, 12, 10, 1)
    for _ in range(warmup):
        call()
    eng.check_status()
    stream = torch.cuda.Stream()
    eng.set_stream(stream.cuda_stream)
    times = []
    for _ in range(steps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(stream)
        call()
        b.record(stream)
        b.synchronize()
        times.append(a.elapsed_time(b))
    eng.set_stream(0)
    eng.check_status()
    return np.array(times), report.cpu().tolist(), stats.cpu().numpy(), Rt_out.cpu().numpy(), ferr.cpu().numpy()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=11)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--shapes", default="a,b")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles"))
    args = ap.parse_args()
    os.makedirs(args.out, exist_ok=True)
    eng = pg.Engine(0)
    for name in args.shapes.split(","):
        rng = np.random.default_rng(0)
        t0 = time.time()
        s, tracks, X, reg, ns = (shape_a if name == "a" else shape_b)(rng)
        d = device_inputs(s, tracks, X, reg)
        gen_s = time.time() - t0
        ms, report, stats, Rt, ferr = bench(eng, d, args.steps, args.warmup, ns)
        tg = reg != 0
        cerr = max(float(np.abs(-Rt[f, :9].reshape(3, 3).T @ Rt[f, 9:] - d["centres"][f]).max()) for f in np.flatnonzero(tg))
        corr = stats[tg, 0]
        rec = dict(shape=name, frames=d["nf"], targets=int(tg.sum()), tracks=d["n_tracks"], nodes=d["n_nodes"],
                   correspondences_mean=float(corr.mean()), correspondences_max=int(corr.max()), n_samples=ns,
                   predicate_evaluations=int(4 * ns * corr.sum()), steps=args.steps, report=report,
                   max_centre_error=cerr, rms_px_max=float(np.nanmax(ferr[tg, 0])), ms_median=float(np.median(ms)),
                   ms_min=float(ms.min()), ms_max=float(ms.max()), input_generation_s=round(gen_s, 1),
                   target_ms=2.0 if name == "a" else None)
        print(json.dumps(rec))
        with open(os.path.join(args.out, "register_%s.json" % name), "w") as fh:
            json.dump(rec, fh, indent=1)
    eng.close()


if __name__ == "__main__":
    main()
