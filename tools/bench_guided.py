#!/usr/bin/env python3
"""Epipolar-guided matching micro-bench (pgx_match_guided_batch_dev against pgx_match_nn_batch_dev) on the bench job's shape:
F frames of 1920 x 1080 with N keypoints each, all F * (F - 1) / 2 image pairs.  The keypoints are projections of one 3D cloud
seen from a camera that moves and turns a little per frame, so every pair has a true F; the descriptors are per-point copies
with --flip of the bits flipped.  Times, interleaved on one stream (median over --reps rounds of --steps calls each):
match_nn and guided at every --bands value, all at the same gate, ratio and cross-check.  Then the accepted and correct
matches of each (correct = both keypoints are views of the same 3D point), and one profiled pass per mode for the kernels'
own times (HIP event groups guided_bucket, guided_walk, guided_col, knn, knn_col, knn_select)."""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.abspath(os.path.join(os.path.dirname(__file__), "..")))
import photogrammetry_amd as pg
from photogrammetry_amd.synth import fundamental_from_pose, rot_y

W, H = 1920, 1080
K = np.array([[1000.0, 0, W / 2], [0, 1000.0, H / 2], [0, 0, 1]])


def scene(F, N, words, flip, seed):
    """-> desc [F][N][words], kp [F][N] (KEYPOINT_DTYPE), point id [F][N], poses [(R, t)] (x ~ K (R X + t))."""
    rng = np.random.default_rng(seed)
    P = 5 * N
    X = np.stack([rng.uniform(-8, 8 + 0.08 * F, P), rng.uniform(-5, 5, P), rng.uniform(8, 20, P)], 1)
    base = rng.integers(0, 2**32, size=(P, words), dtype=np.uint32)
    poses = [(rot_y(-0.002 * f), np.array([-0.08 * f, -0.005 * f, 0.01 * f])) for f in range(F)]
    desc = np.zeros((F, N, words), dtype=np.uint32)
    kp = np.zeros((F, N), dtype=pg.KEYPOINT_DTYPE)
    ids = np.zeros((F, N), dtype=np.int64)
    for f, (R, t) in enumerate(poses):
        x = (K @ (R @ X.T + t[:, None])).T
        p = np.rint(x[:, :2] / x[:, 2:3]).astype(np.int64)
        vis = np.nonzero((x[:, 2] > 0) & (p[:, 0] >= 0) & (p[:, 0] < W) & (p[:, 1] >= 0) & (p[:, 1] < H))[0]
        if len(vis) < N:
            raise SystemExit("frame %d sees %d points, fewer than %d" % (f, len(vis), N))
        keep = rng.permutation(vis)[:N]
        bits = np.unpackbits(base[keep].view(np.uint8), axis=1)
        bits ^= (rng.random(bits.shape) < flip).astype(np.uint8)
        desc[f] = np.packbits(bits, axis=1).view(np.uint32)
        kp["x"][f], kp["y"][f] = p[keep, 0], p[keep, 1]
        ids[f] = keep
    return desc, kp, ids, poses


def true_F(poses, a, b):
    """h_a^T F h_b = 0 (include/pgx.h), unit Frobenius norm."""
    (Ra, ta), (Rb, tb) = poses[a], poses[b]
    R = Rb @ Ra.T
    return fundamental_from_pose(K, R, tb - R @ ta).reshape(9)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--n", type=int, default=4096)
    ap.add_argument("--words", type=int, default=8)
    ap.add_argument("--flip", type=float, default=0.1)
    ap.add_argument("--bands", default="1,2,4,8,32")
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--max-dist", type=int, default=64)
    ap.add_argument("--ratio", type=float, default=0.8)
    ap.add_argument("--no-profile", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    F, N, words = args.frames, args.n, args.words
    bands = [float(b) for b in args.bands.split(",")]
    desc, kp, ids, poses = scene(F, N, words, args.flip, 7)
    pl = [(i, j) for i in range(F) for j in range(i + 1, F)]
    M = len(pl)
    Fs = np.stack([true_F(poses, a, b) for a, b in pl])

    dev = torch.device("cuda", 0)
    eng = pg.Engine(0)
    stream = torch.cuda.Stream()
    eng.set_stream(stream.cuda_stream)
    d_desc = torch.from_numpy(desc.view(np.int32)).to(dev)
    d_kp = torch.from_numpy(kp.view(np.int32).reshape(F, N, 4)).to(dev)
    d_counts = torch.full((F,), N, dtype=torch.int32, device=dev)
    d_pl = torch.tensor(pl, dtype=torch.int32, device=dev)
    d_F = torch.from_numpy(Fs).to(dev)
    outs = {}

    def nn_mode(out):
        return lambda: eng.match_nn_batch_dev(d_desc, d_counts, N, words, d_pl, M, out, args.max_dist, args.ratio, True)

    def guided_mode(out, band):
        return lambda: eng.match_guided_batch_dev(d_desc, d_kp, d_counts, N, words, d_pl, M, d_F, band, out, args.max_dist,
                                                  args.ratio, True)
    modes = {}
    outs["match_nn"] = torch.empty((M, N, 3), dtype=torch.int32, device=dev)
    modes["match_nn"] = nn_mode(outs["match_nn"])
    for b in bands:
        name = "guided_%g" % b
        outs[name] = torch.empty((M, N, 3), dtype=torch.int32, device=dev)
        modes[name] = guided_mode(outs[name], b)
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

    quality = {}
    pa, pb = np.array([p[0] for p in pl]), np.array([p[1] for p in pl])
    for name, o in outs.items():   # accepted and correct matches over all pairs
        o = o.cpu().numpy()
        acc = o[..., 1] >= 0
        j = np.where(acc, o[..., 1], 0)
        ida = ids[pa]                                    # [M][N] point of row i
        idb = np.take_along_axis(ids[pb], j, axis=1)     # [M][N] point of the matched column
        correct = acc & (ida == idb)
        quality[name] = {"accepted": int(acc.sum()), "correct": int(correct.sum()), "wrong": int(acc.sum() - correct.sum())}

    kern = {}
    if not args.no_profile:
        for name, f in modes.items():   # one profiled pass per mode: the kernels' own times
            eng.profile_reset()
            eng.profile_enable(True)
            for _ in range(args.steps):
                f()
            torch.cuda.synchronize()
            eng.profile_enable(False)
            kern[name] = {}
            for g in ("knn", "knn_col", "knn_select", "guided_bucket", "guided_walk", "guided_col"):
                n, t = eng.profile_get(g)
                if n:
                    kern[name][g] = round(t / args.steps, 4)
        eng.check_status()

    res = {"frames": F, "n": N, "pairs": M, "words": words, "image": [W, H], "flip": args.flip, "steps": args.steps,
           "reps": args.reps, "params": {"max_dist": args.max_dist, "ratio": args.ratio, "cross_check": 1},
           "ms_per_call": {k: round(v, 4) for k, v in ms.items()},
           "ms_per_call_all_reps": {k: [round(x, 4) for x in v] for k, v in times.items()},
           "guided_over_match_nn": {k: round(v / ms["match_nn"], 4) for k, v in ms.items() if k != "match_nn"},
           "matches": quality, "kernels_ms": kern}
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(line + "\n")
    eng.close()


if __name__ == "__main__":
    main()
