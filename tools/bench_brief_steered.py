#!/usr/bin/env python3
"""Steered BRIEF (pgx_set_brief_steering, csrc/k_steer.hip) measured at the bench job's shape: --frames frames of 1920 x 1080
resident in HBM, up to 4096 survivors each, R = 15, B = 32.  One JSON line with three parts:

kernel      the descriptor launch alone (HIP event group "brief": k_steer_kept<true> with the mode on, k_brief_kept<true> with
            it off), interleaved in one process: every round times both modes, --steps detect-chain calls each, median over
            --reps rounds; and the whole detect-chain call the same way.
bench_off   bench.py's step time with the mode off -- the default path, which launches the kernels it always did -- and, with
            --parent-tree DIR (a built checkout of the commit to compare against), that checkout's bench.py alternating with
            this one in the same call.
quality     one synth.make_frame image turned by --angle degrees with scipy about its centre; pgx_match_nn_batch_dev lists
            (distance gate, ratio test, cross check) from the plain and from the steered descriptors of the two images; the
            figure is the share of accepted matches whose partner lies within 2 px of the keypoint's true position."""
import argparse
import json
import os
import statistics
import subprocess
import sys

import numpy as np
import torch

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, ROOT)
import bench
import photogrammetry_amd as pg
from photogrammetry_amd import synth

R, B = 15, 32


def log(*a):
    print(*a, file=sys.stderr, flush=True)


def kernel_times(args, dev):
    F, w, h, cap = args.frames, bench.W, bench.H, bench.NKP
    eng = pg.Engine(0)
    stream = torch.cuda.Stream()   # a real stream: torch's default is the null stream, which the context's own does not order with
    eng.set_stream(stream.cuda_stream)
    pairs = pg.make_brief_pairs(0, 50, bench.P)
    rot, dirs = pg.make_steering(pairs, B)
    eng.set_brief_pairs(pairs)
    eng.set_detect_params(bench.THRESH, bench.RADIUS)
    eng.set_capacity(1 << 18, cap)
    d_base = torch.from_numpy(bench.base_frame(w, h, 0)).to(dev)
    d_frames = bench.roll_frames(torch, d_base, [(37 * k, 11 * k) for k in range(F)])
    i32 = dict(dtype=torch.int32, device=dev)
    d_kp, d_desc = torch.zeros((F, cap, 4), **i32), torch.zeros((F, cap, bench.WORDS), **i32)
    d_counts, d_nraw = torch.zeros(F, **i32), torch.zeros(F, **i32)
    torch.cuda.synchronize()

    def call():
        eng.detect_batch_dev(d_frames, F, w, h, d_kp, d_desc, d_counts, d_nraw, cap)

    def mode(on):
        eng.set_brief_steering(rot if on else None, dirs, R)

    descs = {}
    for on in (False, True):   # warm-up of both modes: workspaces, code objects; and the descriptors for the record
        mode(on)
        call()
        eng.check_status()
        descs[on] = d_desc.cpu().numpy().view(np.uint32).copy()
    counts = d_counts.cpu().numpy()
    eng.profile_filter("brief")
    kern, chain = {False: [], True: []}, {False: [], True: []}
    for _ in range(args.reps):
        for on in (False, True):
            mode(on)
            eng.profile_reset()
            eng.profile_enable(True)
            for _ in range(args.steps):
                call()
            n, t = eng.profile_get("brief")
            eng.profile_enable(False)
            kern[on].append(t / n)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            for _ in range(args.steps):
                call()
            e1.record(stream)
            e1.synchronize()
            chain[on].append(e0.elapsed_time(e1) / args.steps)
    eng.check_status()
    mode(False)
    eng.close()
    changed = sum(int((descs[True][f, :counts[f]] != descs[False][f, :counts[f]]).any(axis=1).sum()) for f in range(F))
    med = statistics.median
    return {"frames": F, "survivors_per_frame": [int(counts.min()), int(counts.max())], "radius": R, "directions": B,
            "steps": args.steps, "reps": args.reps,
            "brief_kernel_ms": {"plain": round(med(kern[False]), 4), "steered": round(med(kern[True]), 4)},
            "brief_kernel_ms_all_reps": {"plain": [round(x, 4) for x in kern[False]], "steered": [round(x, 4) for x in kern[True]]},
            "steered_over_plain": round(med(kern[True]) / med(kern[False]), 3),
            "detect_chain_ms": {"plain": round(med(chain[False]), 4), "steered": round(med(chain[True]), 4)},
            "descriptors_changed_by_steering": changed, "descriptors": int(counts.sum())}


def bench_step(tree, args):
    out = subprocess.run([sys.executable, os.path.join(tree, "bench.py"), "--gpus", "1", "--steps", str(args.bench_steps),
                          "--warmup", str(args.bench_warmup)],
                         cwd=tree, capture_output=True, text=True, check=True).stdout
    line = [ln for ln in out.splitlines() if ln.startswith("{")][-1]
    return float(json.loads(line)["ms_per_step"])


def bench_off(args):
    trees = {"this": ROOT}
    if args.parent_tree:
        trees["parent"] = os.path.abspath(args.parent_tree)
    ms = {k: [] for k in trees}
    for _ in range(args.bench_reps):   # alternating: every round runs each tree once
        for k, tree in trees.items():
            ms[k].append(bench_step(tree, args))
            log("bench.py of %s: %.4f ms per step" % (k, ms[k][-1]))
    out = {"bench_steps": args.bench_steps, "ms_per_step_all_runs": {k: [round(x, 4) for x in v] for k, v in ms.items()},
           "ms_per_step": {k: round(statistics.median(v), 4) for k, v in ms.items()}}
    if "parent" in ms:
        out["this_over_parent"] = round(out["ms_per_step"]["this"] / out["ms_per_step"]["parent"], 4)
    return out


def turned(frame, angle_deg, background=0.5):
    """The RGBA64 frame turned by angle_deg about its centre (bilinear, ground grey outside), and the map of a pixel (x, y) of
    the original to its position in the turned image."""
    from scipy import ndimage
    h, w = frame.shape[:2]
    th = np.deg2rad(angle_deg)
    c, s = np.cos(th), np.sin(th)
    fwd = np.array([[c, -s], [s, c]])                       # on (x, y): p' = centre + fwd (p - centre)
    inv_yx = np.linalg.inv(fwd)[::-1, ::-1]                 # affine_transform maps OUTPUT (row, col) to INPUT (row, col)
    centre_yx = np.array([(h - 1) / 2.0, (w - 1) / 2.0])
    grey = ndimage.affine_transform(frame[..., 0].astype(np.float64), inv_yx, offset=centre_yx - inv_yx @ centre_yx, order=1,
                                    mode="constant", cval=round(background * 65535.0))
    out = np.empty_like(frame)
    out[..., :3] = np.rint(grey).astype(np.uint16)[..., None]
    out[..., 3] = 65535
    centre_xy = centre_yx[::-1]
    return np.ascontiguousarray(out), lambda xy: centre_xy + (np.asarray(xy, np.float64) - centre_xy) @ fwd.T


def quality(args, dev):
    w, h, cap = 1280, 720, 8192
    f0 = synth.make_frame(w, h, seed=3)
    f1, to_turned = turned(f0, args.angle)
    eng = pg.Engine(0)
    pairs = pg.make_brief_pairs(0, 50, bench.P)
    rot, dirs = pg.make_steering(pairs, B)
    eng.set_brief_pairs(pairs)
    eng.set_detect_params(bench.THRESH, 8)
    eng.set_capacity(1 << 18, cap)
    i32 = dict(dtype=torch.int32, device=dev)
    d_frames = torch.from_numpy(np.stack([f0, f1])).to(dev)
    d_kp, d_desc = torch.zeros((2, cap, 4), **i32), torch.zeros((2, cap, bench.WORDS), **i32)
    d_counts, d_nraw = torch.zeros(2, **i32), torch.zeros(2, **i32)
    d_pl = torch.tensor([[0, 1]], **i32)
    d_out = torch.zeros((1, cap, 3), **i32)
    res = {"image": [w, h], "angle_deg": args.angle, "max_dist": args.max_dist, "ratio": args.ratio, "cross_check": 1, "within_px": 2.0}
    for name, on in (("plain", False), ("steered", True)):
        eng.set_brief_steering(rot if on else None, dirs, R)
        torch.cuda.synchronize()
        eng.detect_batch_dev(d_frames, 2, w, h, d_kp, d_desc, d_counts, d_nraw, cap)
        eng.match_nn_batch_dev(d_desc, d_counts, cap, bench.WORDS, d_pl, 1, d_out, args.max_dist, args.ratio, True)
        eng.check_status()
        kp, counts, out = d_kp.cpu().numpy(), d_counts.cpu().numpy(), d_out.cpu().numpy()[0]
        lst = out[:counts[0]]
        acc = lst[lst[:, 1] >= 0]
        want = to_turned(kp[0, acc[:, 0], :2])
        err = np.linalg.norm(kp[1, acc[:, 1], :2] - want, axis=1)
        inside = ((want >= 0) & (want <= [w - 1, h - 1])).all(axis=1)
        res[name] = {"keypoints": [int(counts[0]), int(counts[1])], "accepted": int(len(acc)), "correct": int((err <= 2.0).sum()),
                     "share_correct": round(float((err <= 2.0).mean()), 4) if len(acc) else None,
                     "accepted_with_true_position_inside": int(inside.sum())}
    eng.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=bench.SEQ_FRAMES)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--bench-steps", type=int, default=20)
    ap.add_argument("--bench-warmup", type=int, default=5)
    ap.add_argument("--bench-reps", type=int, default=2)
    ap.add_argument("--parent-tree", default=None, help="a built checkout of the commit to compare bench.py's step time against")
    ap.add_argument("--no-bench", action="store_true")
    ap.add_argument("--angle", type=float, default=30.0)
    ap.add_argument("--max-dist", type=int, default=64)
    ap.add_argument("--ratio", type=float, default=0.8)
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    out = {"kernel": kernel_times(args, dev)}
    log("kernel:", json.dumps(out["kernel"]))
    out["quality"] = quality(args, dev)
    log("quality:", json.dumps(out["quality"]))
    if not args.no_bench:
        out["bench_off"] = bench_off(args)   # child processes: after this one's contexts are closed
    print(json.dumps(out))


if __name__ == "__main__":
    main()
