"""Micro-benchmark of the mesh at tools/bench_cloud.py's shape: 8 references of 1920 x 1080 out of 12
frames on a line, the filter's list of their depth maps (a smooth synthetic surface seen by every camera) meshed at a cell of
--cell-scale pixel footprints, band 1, truncation 3 cells.  Timed with HIP events on geom_bench's loop: the whole pgx_mesh_dev
call, and the whole pgx_cloud_merge_dev call on the same list for scale; then the mesh by pass from the stage's profiling groups
(pgx_profile_get) in a second pass.  With --clean, pgx_mesh_clean_dev on the mesh's outputs and report:
the whole call without smoothing and with --clean-iters iterations, and its passes as medians over the calls (one profile read
per call).  With --clean --decimate, pgx_mesh_decimate_dev behind the clean stage, on its outputs and report: the
whole call and its passes for a uniform and an adaptive setting.  Writes profiles/mesh_<shape>.json, with --clean
profiles/mesh_clean_<shape>.json, with --decimate profiles/mesh_decimate_<shape>.json (or --out DIR)."""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, ROOT)
import geom_bench as gb  # noqa: E402
import photogrammetry_amd as pg  # noqa: E402
from bench_cloud import surface_depths  # noqa: E402
from bench_depth import cameras  # noqa: E402
from geom_bench import DEV, F64, I32  # noqa: E402

CLEAN_PARTS = ("mclean_init", "mclean_union", "mclean_count", "mclean_rank", "mclean_emit", "mclean_rows", "mclean_smooth", "mclean_normals")
DECIMATE_PARTS = ("mdec_init", "mdec_tris", "mdec_levels", "mdec_clusters", "mdec_dedup", "mdec_rank", "mdec_emit", "mdec_normals")
DECIMATE_SETTINGS = (("uniform", 1, 1, 1015), ("adaptive", 0, 3, 1015), ("adaptive6", 0, 6, 1015))
PARTS = ("mesh_plan", "mesh_seed", "mesh_dilate", "mesh_tsdf", "mesh_cubes", "mesh_rank", "mesh_vertices", "mesh_tris")


def bench_clean(eng, args, mesh_out, rep, nv, nt, cell, origin):
    """pgx_mesh_clean_dev on the mesh's outputs where they lie, the counts from the mesh's report on the device -> the record"""
    oxyz, onrm, orgb, oinf, otri = mesh_out
    cx, cn = torch.empty((max(nv, 1), 3), **F64), torch.empty((max(nv, 1), 3), dtype=torch.float32, device=DEV)
    cc, ci, ct, crep = torch.empty(max(nv, 1), **I32), torch.empty((max(nv, 1), 4), **I32), torch.empty((max(nt, 1), 3), **I32), torch.empty(8, **I32)
    out = {}
    for name, iters in (("iters0", 0), ("iters%d" % args.clean_iters, args.clean_iters)):
        def clean():
            eng.mesh_clean_dev(oxyz, onrm, orgb, oinf, otri, rep, nv, nt, cell, origin, nv, nt, cx, cn, cc, ci, ct, crep,
                               min_tris=args.min_tris, iters=iters, lam=0.5, mu=-0.53)
        ms = gb.time_on_stream(eng, clean, args.steps, args.warmup)
        eng.profile_enable(True)
        per = {p: [] for p in CLEAN_PARTS}
        for _ in range(args.steps):
            eng.profile_reset()
            clean()
            for p in CLEAN_PARTS:
                per[p].append(eng.profile_get(p)[1])
        eng.profile_enable(False)
        eng.check_status()
        parts = {p: round(float(np.median(v)), 4) for p, v in per.items()}
        half = 2 * iters
        # what a half-step must move: per kept vertex its row (4 B an entry, 3 entries a triangle in all), per entry a triangle
        # (12 B) and three positions (72 B) that mostly hit in cache, one position read and one written (48 B)
        r = crep.cpu().tolist()
        floor_bytes = r[6] * 3 * 4 + r[6] * 12 + r[5] * 24 * 2
        out[name] = dict(iters=iters, ms_median=float(np.median(ms)), ms_min=float(ms.min()), ms_max=float(ms.max()), parts_ms=parts,
                         report=r, half_step_ms=(parts["mclean_smooth"] / half if half else None),
                         half_step_floor_bytes=floor_bytes,
                         half_step_gbps=(floor_bytes / (parts["mclean_smooth"] / half * 1e-3) / 1e9 if half and parts["mclean_smooth"] > 0 else None),
                         union_ns_per_triangle=parts["mclean_union"] * 1e6 / max(r[1], 1))
    return out


def bench_decimate(eng, args, mesh_out, rep, nv, nt, cell, origin):
    """pgx_mesh_decimate_dev behind pgx_mesh_clean_dev (--clean-iters iterations) on the clean stage's outputs where they lie, the
    counts from its report on the device -> the record"""
    def bufs():
        return (torch.empty((max(nv, 1), 3), **F64), torch.empty((max(nv, 1), 3), dtype=torch.float32, device=DEV), torch.empty(max(nv, 1), **I32),
                torch.empty((max(nv, 1), 4), **I32), torch.empty((max(nt, 1), 3), **I32), torch.empty(8, **I32))
    c, d = bufs(), bufs()
    eng.mesh_clean_dev(*mesh_out, rep, nv, nt, cell, origin, nv, nt, *c, min_tris=args.min_tris, iters=args.clean_iters, lam=0.5, mu=-0.53)
    eng.check_status()
    crep = c[5].cpu().tolist()
    out = dict(clean_iters=args.clean_iters, clean_report=crep)
    for name, lmin, lmax, flat_q in DECIMATE_SETTINGS:
        def decimate():
            eng.mesh_decimate_dev(*c, nv, nt, cell, origin, nv, nt, *d, lmin=lmin, lmax=lmax, flat_q=flat_q)
        ms = gb.time_on_stream(eng, decimate, args.steps, args.warmup)
        eng.profile_enable(True)
        per = {p: [] for p in DECIMATE_PARTS}
        for _ in range(args.steps):
            eng.profile_reset()
            decimate()
            for p in DECIMATE_PARTS:
                per[p].append(eng.profile_get(p)[1])
        eng.profile_enable(False)
        eng.check_status()
        parts = {p: round(float(np.median(v)), 4) for p, v in per.items()}
        r = d[5].cpu().tolist()
        # what the incidence pass must move: per triangle its indices (12 B), the used mark and m (4 + 8 B written); per vertex its
        # position once (24 B; the other reads of it hit in cache) and the member byte
        floor_bytes = r[1] * 24 + r[0] * 25
        out[name] = dict(lmin=lmin, lmax=lmax, flat_q=flat_q, ms_median=float(np.median(ms)), ms_min=float(ms.min()), ms_max=float(ms.max()),
                         parts_ms=parts, report=r, tris_floor_bytes=floor_bytes,
                         tris_gbps=(floor_bytes / (parts["mdec_tris"] * 1e-3) / 1e9 if parts["mdec_tris"] > 0 else None),
                         tris_ns_per_triangle=parts["mdec_tris"] * 1e6 / max(r[1], 1))
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
    ap.add_argument("--band", type=int, default=1)
    ap.add_argument("--trunc-cells", type=int, default=3)
    ap.add_argument("--max-voxels", type=int, default=1 << 25)
    ap.add_argument("--clean", action="store_true", help="also time pgx_mesh_clean_dev behind the mesh")
    ap.add_argument("--clean-iters", type=int, default=5)
    ap.add_argument("--decimate", action="store_true", help="with --clean: also time pgx_mesh_decimate_dev behind the clean stage")
    ap.add_argument("--min-tris", type=int, default=100)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles"))
    args = ap.parse_args()
    assert args.steps >= 7, "the median of at least 7 calls"
    assert args.clean or not args.decimate, "--decimate follows the clean stage: give --clean too"
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
    col, agr = torch.empty((F, H, W), **I32), torch.empty((R, H, W), **I32)
    cap = R * W * H
    xyz, src, fsum = torch.empty((cap, 3), **F64), torch.empty((cap, 2), **I32), torch.empty(4, **I32)
    mvox, mv, mt = args.max_voxels, args.max_voxels // 2, args.max_voxels
    oxyz, onrm = torch.empty((cap, 3), **F64), torch.empty((cap, 3), dtype=torch.float32, device=DEV)
    orgb, oinf, crep = torch.empty(cap, **I32), torch.empty((cap, 4), **I32), torch.empty(8, **I32)
    otri, rep = torch.empty((mt, 3), **I32), torch.empty(8, **I32)
    cell = float(dep.median()) / focal * args.cell_scale
    origin = (-(2**19) * cell,) * 3
    torch.cuda.synchronize()
    eng.depth_fuse_dev(dep, d_views, R, S, W, H, F, P, cap, xyz, src, fsum, rel_tol=0.05, min_agree=2, d_agree=agr)
    eng.rgba8_batch_dev(rgba, F, W, H, col)
    eng.check_status()

    def mesh():   # the vertex outputs reuse the cloud's buffers: mv <= cap rows
        eng.mesh_dev(xyz, src, fsum, cap, dep, d_views, R, S, W, H, F, P, cell, origin, mvox, min(mv, cap), mt, oxyz, onrm, orgb, oinf, otri,
                     rep, d_agree=agr, min_agree=2, d_rgba8=col, F=F, band=args.band, trunc_cells=args.trunc_cells)

    def merge():
        eng.cloud_merge_dev(xyz, src, fsum, cap, dep, d_views, R, S, W, H, F, P, cell, origin, cap, oxyz, onrm, orgb, oinf, crep,
                            d_rgba8=col, F=F, normal_step=1, disc_tol=0.02, min_support=1)
    ms_merge = gb.time_on_stream(eng, merge, args.steps, args.warmup)
    ms_mesh = gb.time_on_stream(eng, mesh, args.steps, args.warmup)
    eng.profile_reset()
    eng.profile_enable(True)
    for _ in range(args.steps):
        mesh()
    eng.check_status()
    parts = {p: eng.profile_get(p)[1] / args.steps for p in PARTS}
    eng.profile_enable(False)
    report = rep.cpu().tolist()
    med = float(np.median(ms_mesh))
    rec = dict(shape="%dx%d_r%d_c%g_b%d" % (W, H, R, args.cell_scale, args.band), frames=F, refs=R, cell=cell, band=args.band,
               trunc_cells=args.trunc_cells, steps=args.steps, mesh_ms_median=med, mesh_ms_min=float(ms_mesh.min()),
               mesh_ms_max=float(ms_mesh.max()), parts_ms={k: round(v, 4) for k, v in parts.items()}, report=report,
               input_points=report[0], seed_cells=report[2], voxels=report[3], valid_voxels=report[4], vertices=report[5],
               triangles=report[6], max_voxels=mvox, voxels_per_s=report[3] / (med * 1e-3),
               cloud_merge_ms_median=float(np.median(ms_merge)), cloud_report=crep.cpu().tolist(), fuse_summary=fsum.cpu().tolist())
    if args.clean:
        rec["clean"] = bench_clean(eng, args, (oxyz, onrm, orgb, oinf, otri), rep, report[5], report[6], cell, origin)
    if args.decimate:
        rec["decimate"] = bench_decimate(eng, args, (oxyz, onrm, orgb, oinf, otri), rep, report[5], report[6], cell, origin)
    gb.write_record(rec, args.out, "mesh_decimate" if args.decimate else "mesh_clean" if args.clean else "mesh")
    eng.close()


if __name__ == "__main__":
    main()
