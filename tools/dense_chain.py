"""One command for the chain that DESIGN.md sections 27 and 28 close: pgx_triangulate_tracks_dev -> pgx_dense_views_dev ->
pgx_gray_batch_dev -> pgx_depth_maps_dev -> pgx_depth_fuse_dev -> pgx_rgba8_batch_dev -> pgx_cloud_merge_dev on one stream, with
no synchronisation between the triangulation and the merged cloud.  The scene is synth.make_scene's (frames on an arc, true tracks cut to runs); the frames are
seeded noise, so the maps carry no meaning: the tool shows that the chain runs and what it costs.  Timed with HIP events on
geom_bench's loop; prints one JSON line and writes profiles/dense_chain_<shape>.json (or --out DIR).  --mesh adds pgx_mesh_dev
behind the cloud and writes profiles/dense_chain_mesh_<shape>.json; --mesh --clean adds pgx_mesh_clean_dev
behind the mesh on the same stream (the mesh's outputs and its report on the device, no wait between them),
its time as clean_ms in the record dense_chain_mesh_clean_<shape>.json; --mesh --clean --decimate adds pgx_mesh_decimate_dev behind
the clean stage in the same way, its time as decimate_ms in dense_chain_mesh_clean_decimate_<shape>.json; the
default run is the chain above."""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, ROOT)
import geom_bench as gb  # noqa: E402
import photogrammetry_amd as pg  # noqa: E402
from geom_bench import DEV, F64, I32  # noqa: E402

PARTS = ("triangulate", "dense_views_nodes", "dense_views_pairs", "dense_views_select", "dewarp_gray", "depth_census", "depth_plan",
         "depth_sweep", "depth_fuse", "dewarp_rgba8", "cloud_plan", "cloud_normals", "cloud_points", "cloud_rank", "cloud_accum",
         "cloud_final")
CLEAN_PARTS = ("mclean_init", "mclean_union", "mclean_count", "mclean_rank", "mclean_emit", "mclean_rows", "mclean_smooth", "mclean_normals")
DECIMATE_PARTS = ("mdec_init", "mdec_tris", "mdec_levels", "mdec_clusters", "mdec_dedup", "mdec_rank", "mdec_emit", "mdec_normals")
MESH_PARTS = ("mesh_plan", "mesh_seed", "mesh_dilate", "mesh_tsdf", "mesh_cubes", "mesh_rank", "mesh_vertices", "mesh_tris")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--width", type=int, default=640)
    ap.add_argument("--height", type=int, default=480)
    ap.add_argument("--frames", type=int, default=16)
    ap.add_argument("--points", type=int, default=4000)
    ap.add_argument("--sources", type=int, default=4)
    ap.add_argument("--planes", type=int, default=64)
    ap.add_argument("--cell", type=float, default=0.02)
    ap.add_argument("--mesh", action="store_true", help="pgx_mesh_dev behind the cloud (band 2, truncation 3 cells); the record is dense_chain_mesh_*")
    ap.add_argument("--clean", action="store_true", help="with --mesh: pgx_mesh_clean_dev behind the mesh (min_tris 100, --clean-iters Taubin steps); the record is dense_chain_mesh_clean_*")
    ap.add_argument("--clean-iters", type=int, default=5)
    ap.add_argument("--decimate", action="store_true", help="with --mesh --clean: pgx_mesh_decimate_dev behind the clean stage (lmin 0, lmax 3, flat_q 1015); the record is dense_chain_mesh_clean_decimate_*")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles"))
    args = ap.parse_args()
    assert args.mesh or not args.clean, "--clean cleans the mesh: give --mesh too"
    assert args.clean or not args.decimate, "--decimate follows the clean stage: give --mesh --clean too"
    W, H, nf, S, D = args.width, args.height, args.frames, args.sources, args.planes
    rng = np.random.default_rng(0)
    eng = pg.Engine(0)
    s, off, nodes, _ = gb.cut_scene(rng, nf, args.points)
    d = gb.device_inputs(s["kps"], off, nodes, P=s["P"])
    nt, N = d["n_tracks"], nf * d["stride"]
    rgba = torch.from_numpy(rng.integers(0, 65536, (nf, H, W, 4), dtype=np.uint16)).to(DEV)
    xyz, q, tfl, tsum = torch.empty((nt, 3), **F64), torch.empty((nt, 3), **F64), torch.empty(nt, **I32), torch.empty(8, **I32)
    views, rng_d, st, rep = torch.empty((nf, 1 + S), **I32), torch.empty((nf, 2), **F64), torch.empty((nf, 4), **I32), torch.empty(8, **I32)
    gray = torch.empty((nf, H, W), dtype=torch.float32, device=DEV)
    kq8, fl, dep, msum = torch.empty((nf, H, W), **I32), torch.empty((nf, H, W), **I32), torch.empty((nf, H, W), **F64), torch.empty(8, **I32)
    cap = nf * H * W
    pts, src, fsum = torch.empty((cap, 3), **F64), torch.empty((cap, 2), **I32), torch.empty(4, **I32)
    col = torch.empty((nf, H, W), **I32)
    oxyz, onrm = torch.empty((cap, 3), **F64), torch.empty((cap, 3), dtype=torch.float32, device=DEV)
    orgb, oinf, crep = torch.empty(cap, **I32), torch.empty((cap, 4), **I32), torch.empty(8, **I32)
    origin = (-(2**19) * args.cell,) * 3      # the scene in the middle of the grid
    parts_of = PARTS
    if args.mesh:
        parts_of = PARTS + MESH_PARTS
        mvox, mv, mt = 1 << 24, 1 << 22, 1 << 23
        agr = torch.empty((nf, H, W), **I32)
        mxyz, mnrm = torch.empty((mv, 3), **F64), torch.empty((mv, 3), dtype=torch.float32, device=DEV)
        mrgb, minf, mtri, mrep = torch.empty(mv, **I32), torch.empty((mv, 4), **I32), torch.empty((mt, 3), **I32), torch.empty(8, **I32)
    if args.clean:
        parts_of = parts_of + CLEAN_PARTS
        cxyz, cnrm = torch.empty((mv, 3), **F64), torch.empty((mv, 3), dtype=torch.float32, device=DEV)
        crgb, cinf, ctri, clrep = torch.empty(mv, **I32), torch.empty((mv, 4), **I32), torch.empty((mt, 3), **I32), torch.empty(8, **I32)
    if args.decimate:
        parts_of = parts_of + DECIMATE_PARTS
        dxyz, dnrm = torch.empty((mv, 3), **F64), torch.empty((mv, 3), dtype=torch.float32, device=DEV)
        drgb, dinf, dtri, dcrep = torch.empty(mv, **I32), torch.empty((mv, 4), **I32), torch.empty((mt, 3), **I32), torch.empty(8, **I32)
    torch.cuda.synchronize()

    def chain():
        eng.triangulate_tracks_dev(d["kp"], nf, d["stride"], nf, d["P"], d["off"], d["nodes"], d["tsum"], nt, xyz, q, tfl, tsum, 1.0, 2.0, 10)
        eng.dense_views_dev(d["off"], d["nodes"], d["tsum"], nt, N, xyz, nf, d["P"], nf, S, views, rng_d, st, rep, d_track_flags=tfl)
        eng.gray_batch_dev(rgba, nf, W, H, gray)
        eng.depth_maps_dev(gray, nf, W, H, nf, d["P"], views, nf, S, rng_d, D, kq8, dep, fl, msum, agg_radius=2, min_views=2)
        eng.depth_fuse_dev(dep, views, nf, S, W, H, nf, d["P"], cap, pts, src, fsum, d_agree=agr if args.mesh else None)
        eng.rgba8_batch_dev(rgba, nf, W, H, col)
        eng.cloud_merge_dev(pts, src, fsum, cap, dep, views, nf, S, W, H, nf, d["P"], args.cell, origin, cap, oxyz, onrm, orgb, oinf, crep,
                            d_rgba8=col, F=nf)
        if args.mesh:
            eng.mesh_dev(pts, src, fsum, cap, dep, views, nf, S, W, H, nf, d["P"], args.cell, origin, mvox, mv, mt, mxyz, mnrm, mrgb, minf,
                         mtri, mrep, d_agree=agr, min_agree=2, d_rgba8=col, F=nf, band=2, trunc_cells=3)
        if args.clean:
            eng.mesh_clean_dev(mxyz, mnrm, mrgb, minf, mtri, mrep, mv, mt, args.cell, origin, mv, mt, cxyz, cnrm, crgb, cinf, ctri, clrep,
                               min_tris=100, iters=args.clean_iters, lam=0.5, mu=-0.53)
        if args.decimate:
            eng.mesh_decimate_dev(cxyz, cnrm, crgb, cinf, ctri, clrep, mv, mt, args.cell, origin, mv, mt, dxyz, dnrm, drgb, dinf, dtri, dcrep,
                                  lmin=0, lmax=3, flat_q=1015)
    ms = gb.time_on_stream(eng, chain, args.steps, args.warmup)
    eng.profile_reset()
    eng.profile_enable(True)
    for _ in range(args.steps):
        chain()
    eng.check_status()
    parts = {p: eng.profile_get(p)[1] / args.steps for p in parts_of}
    eng.profile_enable(False)
    rec = dict(shape="%dx%d_f%d_s%d_d%d" % (W, H, nf, S, D), frames=nf, tracks=nt, nodes=d["n_nodes"], steps=args.steps,
               chain_ms_median=float(np.median(ms)), chain_ms_min=float(ms.min()), chain_ms_max=float(ms.max()),
               parts_ms={k: round(v, 4) for k, v in parts.items()}, views_report=rep.cpu().tolist(), maps_summary=msum.cpu().tolist(),
               fuse_summary=fsum.cpu().tolist(), cloud_report=crep.cpu().tolist(), refs_flagged=int((st.cpu().numpy()[:, 3] != 0).sum()))
    if args.mesh:
        rec["mesh_report"] = mrep.cpu().tolist()
    if args.clean:
        rec["clean_report"] = clrep.cpu().tolist()
        rec["clean_ms"] = round(sum(parts[p] for p in CLEAN_PARTS), 4)
    if args.decimate:
        rec["decimate_report"] = dcrep.cpu().tolist()
        rec["decimate_ms"] = round(sum(parts[p] for p in DECIMATE_PARTS), 4)
    gb.write_record(rec, args.out, "dense_chain_mesh_clean_decimate" if args.decimate else "dense_chain_mesh_clean" if args.clean else ("dense_chain_mesh" if args.mesh else "dense_chain"))
    eng.close()


if __name__ == "__main__":
    main()
