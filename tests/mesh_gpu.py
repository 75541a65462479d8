"""What the GPU tests of the mesh and of the host forms share (test_gpu_mesh.py, test_gpu_host_forms.py): the run wrapper
of pgx_mesh_dev with sentinel-filled outputs, and the two-map rig with the point lists drawn from its surface.  The engine is
always the caller's.  A plain helper module: no test module imports another."""
import functools

import numpy as np
import torch

import depth_ref
import photogrammetry_amd as pg

DEV = "cuda:0"
CELL, ORIGIN = 0.25, (-8.0, -8.0, -8.0)           # the grid of the rig cases: a pixel's footprint at depth 3 is 0.17


def dev(a, dtype):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).to(DEV)


def run_mesh(engine, c, caps, cell=CELL, origin=ORIGIN, band=1, trunc_cells=3, min_weight=1, min_agree=0, count=None, check=True):
    """pgx_mesh_dev on case c (xyz, src, depth, views, P; agree, rgba8, frame_ids or absent) over sentinel-filled outputs of the
    capacities caps = (max_voxels, max_vertices, max_tris), one sync -> dict of host arrays (untrimmed) and err"""
    xyz = np.asarray(c["xyz"], dtype=np.float64).reshape(-1, 3)
    src = np.asarray(c["src"], dtype=np.int32).reshape(-1, 2)
    depth = np.asarray(c["depth"], dtype=np.float64)
    R, H, W = depth.shape
    views = np.asarray(c["views"], dtype=np.int32).reshape(R, -1)
    P = np.reshape(c["P"], (-1, 12))
    agree, rgba8, frame_ids = c.get("agree"), c.get("rgba8"), c.get("frame_ids")
    max_in = len(xyz)
    mvox, mv, mt = caps
    i32 = dict(dtype=torch.int32, device=DEV)
    oxyz = torch.full((max(mv, 1), 3), 5.0, dtype=torch.float64, device=DEV)
    onrm = torch.full((max(mv, 1), 3), 5.0, dtype=torch.float32, device=DEV)
    orgb, oinf = torch.full((max(mv, 1),), 77, **i32), torch.full((max(mv, 1), 4), 77, **i32)
    otri, rep = torch.full((max(mt, 1), 3), 77, **i32), torch.full((8,), 77, **i32)
    dx, ds = dev(xyz if max_in else np.zeros((1, 3)), np.float64), dev(src if max_in else np.zeros((1, 2)), np.int32)
    dd, dv, dP = dev(depth, np.float64), dev(views, np.int32), dev(P, np.float64)
    dc = None if count is None else dev([count, 9, 9, 9], np.int32)
    dag = None if agree is None else dev(agree, np.int32)
    dcol = None if rgba8 is None else dev(np.asarray(rgba8).astype(np.uint32).view(np.int32), np.int32)
    dids = None if frame_ids is None else dev(frame_ids, np.int32)
    torch.cuda.synchronize()
    engine.mesh_dev(dx, ds, dc, max_in, dd, dv, R, views.shape[1] - 1, W, H, len(P), dP, cell, origin, mvox, mv, mt, oxyz, onrm, orgb,
                    oinf, otri, rep, d_agree=dag, min_agree=min_agree, d_rgba8=dcol, F=0 if rgba8 is None else len(rgba8),
                    d_frame_ids=dids, band=band, trunc_cells=trunc_cells, min_weight=min_weight)
    err = None
    try:
        engine.check_status()
    except pg.CapacityError as e:
        if check:
            raise
        err = e
    return dict(xyz=oxyz.cpu().numpy(), normal=onrm.cpu().numpy(), rgba8=orgb.cpu().numpy().view(np.uint32), info=oinf.cpu().numpy(),
                tri=otri.cpu().numpy(), report=rep.cpu().numpy(), err=err)


@functools.lru_cache(maxsize=None)
def rig():
    """two maps of 16 x 12 with smooth depths and their cameras, colours by slot, the filter's list and agreement counts"""
    W, H = 16, 12
    P = np.stack([depth_ref.scene_camera(c, W, H, 18.0).reshape(12) for c in [(0.0, 0.0, 0.0), (0.3, 0.1, 0.0)]])
    v, u = np.mgrid[0:H, 0:W]
    depth = np.stack([3.0 + 0.02 * u + 0.01 * v, 3.1 + 0.015 * u + 0.012 * v]).astype(np.float64)
    views = np.array([[0, 1], [1, 0]], np.int32)
    rgba8 = np.random.default_rng(1).integers(0, 2**32, (2, H, W), dtype=np.uint32)
    f = depth_ref.fuse(depth, views, 2, P, 0.5, 0)
    return dict(depth=depth, views=views, P=P, rgba8=rgba8, W=W, H=H, xyz=f["xyz"], src=f["src"])


def synth(n, seed, jitter=CELL / 4):
    """n points drawn from rig()'s surface points, each moved by up to `jitter`: many points a cell, a few hundred cells"""
    rng = np.random.default_rng(seed)
    c = dict(rig())
    idx = rng.integers(0, len(c["xyz"]), n)
    c["xyz"] = c["xyz"][idx] + rng.uniform(-jitter, jitter, (n, 3))
    c["src"] = c["src"][idx]
    return c
