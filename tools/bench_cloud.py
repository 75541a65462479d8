"""Micro-benchmark of the cloud merge at tools/bench_depth.py's shape: 8 references of 1920 x 1080 out of
12 frames on a line, the filter's list of their depth maps merged at a cell of the median depth divided by the focal length (the
footprint of a pixel).  The depth maps are a smooth synthetic surface seen by every camera, so that the filter keeps most pixels
and neighbouring maps give the same surface points: the sweep is not what is measured here.  Timed with HIP events on geom_bench's
loop: the whole pgx_cloud_merge_dev call and the whole pgx_rgba8_batch_dev call, then the merge by pass from the stage's profiling
groups (pgx_profile_get) in a second pass.  Writes profiles/cloud_<shape>.json (or --out DIR)."""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, ROOT)
import geom_bench as gb  # noqa: E402
import photogrammetry_amd as pg  # noqa: E402
from bench_depth import cameras  # noqa: E402
from geom_bench import DEV, F64, I32  # noqa: E402

PARTS = ("cloud_plan", "cloud_normals", "cloud_points", "cloud_rank", "cloud_accum", "cloud_final")
HBM_BYTES_PER_S = 8e12


def surface_depths(P, W, H, R, first):
    """the depth at every pixel of references first .. first + R - 1 of the surface z = 4 + 0.3 sin(1.5 x) cos(1.2 y), for cameras
    K [I | -C]: eight fixed-point steps along the ray from z = 4 (the surface is shallow: they converge far inside the filter's tolerance)"""
    v, u = torch.meshgrid(torch.arange(H, **F64), torch.arange(W, **F64), indexing="ij")
    out = torch.empty((R, H, W), **F64)
    for r in range(R):
        p = P[first + r].reshape(3, 4)
        fx, fy, cx, cy = p[0, 0], p[1, 1], p[0, 2], p[1, 2]
        C = torch.stack([-(p[0, 3] - cx * p[2, 3]) / fx, -(p[1, 3] - cy * p[2, 3]) / fy, -p[2, 3]])
        dx, dy = (u - cx) / fx, (v - cy) / fy
        z = torch.full_like(u, 4.0)
        for _ in range(8):
            z = 4.0 + 0.3 * torch.sin(1.5 * (C[0] + (z - C[2]) * dx)) * torch.cos(1.2 * (C[1] + (z - C[2]) * dy))
        out[r] = z - C[2]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--frames", type=int, default=12)
    ap.add_argument("--refs", type=int, default=8)
    ap.add_argument("--cell-scale", type=float, default=1.0, help="the cell in pixel footprints")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles"))
    args = ap.parse_args()
    assert args.steps >= 7, "the median of at least 7 calls"
    W, H, F, R, S, focal = args.width, args.height, args.frames, args.refs, 4, 1500.0
    eng = pg.Engine(0)
    torch.manual_seed(0)
    P = torch.from_numpy(cameras(F, W, H, focal, 0.25)).to(DEV)
    first = (F - R) // 2
    views = np.array([[first + r] + [first + r + o for o in (-2, -1, 1, 2)] for r in range(R)], dtype=np.int32)
    views[(views < 0) | (views >= F)] = -1
    d_views = torch.from_numpy(views).to(DEV)
    dep = surface_depths(P, W, H, R, first)
    rgba = torch.from_numpy(np.random.default_rng(0).integers(0, 65536, (F, H, W, 4), dtype=np.uint16)).to(DEV)
    col = torch.empty((F, H, W), **I32)
    cap = R * W * H
    xyz, src, fsum = torch.empty((cap, 3), **F64), torch.empty((cap, 2), **I32), torch.empty(4, **I32)
    oxyz, onrm = torch.empty((cap, 3), **F64), torch.empty((cap, 3), dtype=torch.float32, device=DEV)
    orgb, oinf, rep = torch.empty(cap, **I32), torch.empty((cap, 4), **I32), torch.empty(8, **I32)
    cell = float(dep.median()) / focal * args.cell_scale
    origin = (-(2**19) * cell,) * 3
    torch.cuda.synchronize()
    eng.depth_fuse_dev(dep, d_views, R, S, W, H, F, P, cap, xyz, src, fsum, rel_tol=0.05, min_agree=2)
    eng.check_status()

    def colour():
        eng.rgba8_batch_dev(rgba, F, W, H, col)

    def merge():
        eng.cloud_merge_dev(xyz, src, fsum, cap, dep, d_views, R, S, W, H, F, P, cell, origin, cap, oxyz, onrm, orgb, oinf, rep,
                            d_rgba8=col, F=F, normal_step=1, disc_tol=0.02, min_support=1)
    ms_col = gb.time_on_stream(eng, colour, args.steps, args.warmup)
    ms_merge = gb.time_on_stream(eng, merge, args.steps, args.warmup)
    eng.profile_reset()
    eng.profile_enable(True)
    for _ in range(args.steps):
        merge()
    eng.check_status()
    parts = {p: eng.profile_get(p)[1] / args.steps for p in PARTS}
    eng.profile_enable(False)
    report = rep.cpu().tolist()
    info = oinf[:report[6]].cpu().numpy()
    med, col_bytes = float(np.median(ms_merge)), F * W * H * (8 + 4)
    rec = dict(shape="%dx%d_r%d_c%g" % (W, H, R, args.cell_scale), frames=F, refs=R, cell=cell, steps=args.steps,
               merge_ms_median=med, merge_ms_min=float(ms_merge.min()), merge_ms_max=float(ms_merge.max()),
               parts_ms={k: round(v, 4) for k, v in parts.items()}, report=report, input_points=report[0], output_cells=report[6],
               cells_with_support_2=int((info[:, 0] >= 2).sum()), points_per_s=report[0] / (med * 1e-3),
               rgba8_ms_median=float(np.median(ms_col)), rgba8_ms_min=float(ms_col.min()), rgba8_ms_max=float(ms_col.max()),
               rgba8_bytes=col_bytes, rgba8_fraction_of_8TBps=col_bytes / (float(np.median(ms_col)) * 1e-3) / HBM_BYTES_PER_S,
               fuse_summary=fsum.cpu().tolist())
    gb.write_record(rec, args.out, "cloud")
    eng.close()


if __name__ == "__main__":
    main()
