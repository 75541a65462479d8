"""Micro-benchmark of the dense stage at the bench job's frame size: 1920 x 1080, 8 references with 4
sources each out of 12 frames on a line, D = 128 planes, agg_radius 2.  Timed with HIP events on geom_bench's loop: the whole
pgx_depth_maps_dev call and the whole pgx_depth_fuse_dev call, then the split by part from the stage's profiling groups
(pgx_profile_get) in a second pass.  Projections are counted as the rule counts them (R W H D S) and as the sweep executes
them (tile plus halo); the share of them that gather a census word is measured on a sample of pixels with the device's own warp
and plane tables.  Writes profiles/depth_<shape>.json (or --out DIR)."""
import argparse
import os
import re
import sys

import numpy as np
import torch

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, ROOT)
import geom_bench as gb  # noqa: E402
import photogrammetry_amd as pg  # noqa: E402
from geom_bench import DEV, F64, I32  # noqa: E402
from photogrammetry_amd import _lib  # noqa: E402

PARTS = ("depth_census", "depth_plan", "depth_sweep", "depth_fuse")


def cameras(n, W, H, f, step):
    K = np.array([[f, 0, W / 2], [0, f, H / 2], [0, 0, 1.0]])
    return np.stack([(K @ np.hstack([np.eye(3), -np.array([[step * (i - n / 2)], [0.02 * (i % 3)], [0.0]])])).reshape(12) for i in range(n)])


def valid_share(warp, planes, W, H, rng, n=20000):
    """the share of (pixel, plane, source) triples whose source pixel is valid, on n random pixels of every reference"""
    u, v = rng.integers(0, W, n).astype(np.float64), rng.integers(0, H, n).astype(np.float64)
    ok = tot = 0
    for r in range(warp.shape[0]):
        for s in range(warp.shape[1]):
            A, b = warp[r, s, :9].reshape(3, 3), warp[r, s, 9:]
            y = [(A[i, 0] * u + A[i, 1] * v) + A[i, 2] for i in range(3)]
            q = [planes[r][:, None] * y[i][None] + b[i] for i in range(3)]
            with np.errstate(all="ignore"):
                us, vs = q[0] / q[2] + 0.5, q[1] / q[2] + 0.5
                ok += int(((q[2] > 0) & (us >= 0) & (us < W) & (vs >= 0) & (vs < H)).sum())
            tot += q[2].size
    return ok / tot


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--frames", type=int, default=12)
    ap.add_argument("--refs", type=int, default=8)
    ap.add_argument("--planes", type=int, default=128)
    ap.add_argument("--radius", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles"))
    args = ap.parse_args()
    assert args.steps >= 7, "the median of at least 7 calls"
    W, H, F, R, D, a, S = args.width, args.height, args.frames, args.refs, args.planes, args.radius, 4
    rng = np.random.default_rng(0)
    eng = pg.Engine(0)
    torch.manual_seed(0)
    # smooth-ish texture: noise at a quarter of the resolution, enlarged, plus fine noise
    coarse = torch.rand((F, 1, H // 4 + 1, W // 4 + 1), device=DEV)
    gray = (torch.nn.functional.interpolate(coarse, size=(H, W), mode="bilinear")[:, 0] * 0.8 + 0.2 * torch.rand((F, H, W), device=DEV)).contiguous()
    P = torch.from_numpy(cameras(F, W, H, 1500.0, 0.25)).to(DEV)
    first = (F - R) // 2
    views = np.array([[first + r] + [first + r + o for o in (-2, -1, 1, 2)] for r in range(R)], dtype=np.int32)
    views[(views < 0) | (views >= F)] = -1
    d_views = torch.from_numpy(views).to(DEV)
    d_range = torch.tensor([[2.0, 6.0]] * R, **F64)
    kq8, fl, cost = torch.empty((R, H, W), **I32), torch.empty((R, H, W), **I32), torch.empty((R, H, W), **I32)
    dep, warp, planes = torch.empty((R, H, W), **F64), torch.empty((R, S, 12), **F64), torch.empty((R, D), **F64)
    summary, fsum = torch.empty(8, **I32), torch.empty(4, **I32)
    cap = R * W * H
    xyz, src, agree = torch.empty((cap, 3), **F64), torch.empty((cap, 2), **I32), torch.empty((R, H, W), **I32)
    torch.cuda.synchronize()

    def maps():
        eng.depth_maps_dev(gray, F, W, H, F, P, d_views, R, S, d_range, D, kq8, dep, fl, summary, agg_radius=a, min_views=2,
                           d_cost=cost, d_warp=warp, d_planes=planes)

    def fuse():
        eng.depth_fuse_dev(dep, d_views, R, S, W, H, F, P, cap, xyz, src, fsum, rel_tol=0.05, min_agree=2, d_agree=agree)
    ms_maps = gb.time_on_stream(eng, maps, args.steps, args.warmup)
    ms_fuse = gb.time_on_stream(eng, fuse, args.steps, args.warmup)
    eng.profile_reset()
    eng.profile_enable(True)
    for _ in range(args.steps):
        maps()
        fuse()
    eng.check_status()
    parts = {p: eng.profile_get(p)[1] / args.steps for p in PARTS}
    eng.profile_enable(False)
    src_text = open(os.path.join(_lib.CSRC, "k_depth.hip")).read()
    tw, th = (int(re.search(r"\b%s = (\d+)" % k, src_text).group(1)) for k in ("DEP_TW", "DEP_TH"))
    n_src = int((views[:, 1:] >= 0).sum())
    proj_rule = float(W) * H * D * n_src
    proj_run = proj_rule * ((tw + 2 * a) * (th + 2 * a)) / (tw * th)
    share = valid_share(warp.cpu().numpy(), planes.cpu().numpy(), W, H, rng)
    sweep_s = parts["depth_sweep"] * 1e-3
    rec = dict(shape="%dx%d_r%d_s%d_d%d_a%d" % (W, H, R, S, D, a), frames=F, refs=R, sources=S, planes=D, agg_radius=a, steps=args.steps,
               maps_ms_median=float(np.median(ms_maps)), maps_ms_min=float(ms_maps.min()), maps_ms_max=float(ms_maps.max()),
               fuse_ms_median=float(np.median(ms_fuse)), fuse_ms_min=float(ms_fuse.min()), fuse_ms_max=float(ms_fuse.max()),
               parts_ms={k: round(v, 4) for k, v in parts.items()}, projections_rule=proj_rule, projections_executed=proj_run,
               valid_share=round(share, 4), rule_projections_per_s=proj_rule / sweep_s, executed_projections_per_s=proj_run / sweep_s,
               executed_gathers_per_s=proj_run * share / sweep_s, maps_summary=summary.cpu().tolist(), fuse_summary=fsum.cpu().tolist())
    gb.write_record(rec, args.out, "depth")
    eng.close()


if __name__ == "__main__":
    main()
