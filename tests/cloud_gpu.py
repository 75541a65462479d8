"""What the GPU tests of the cloud merge and of the host forms share (test_gpu_cloud.py, test_gpu_host_forms.py): the run
wrapper of pgx_cloud_merge_dev with sentinel-filled outputs, and the two-map rig with its random point lists.  The engine is
always the caller's.  A plain helper module: no test module imports another."""
import functools

import numpy as np
import torch

import cloud_ref as ref
import depth_ref
import photogrammetry_amd as pg

DEV = "cuda:0"
CELL, ORIGIN = ref.CELL, ref.ORIGIN


def dev(a, dtype):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).to(DEV)


def run_merge(engine, xyz, src, depth, views, P, cell=CELL, origin=ORIGIN, k=1, disc_tol=0.02, min_support=1, max_points=None,
              count=None, rgba8=None, frame_ids=None, optional=True, check=True):
    """pgx_cloud_merge_dev on sentinel-filled outputs, one sync -> dict of host arrays (untrimmed) and err"""
    xyz = np.asarray(xyz, dtype=np.float64).reshape(-1, 3)
    src = np.asarray(src, dtype=np.int32).reshape(-1, 2)
    depth = np.asarray(depth, dtype=np.float64)
    R, H, W = depth.shape
    views = np.asarray(views, dtype=np.int32).reshape(R, -1)
    P = np.reshape(P, (-1, 12))
    max_in = len(xyz)
    cap = max_in if max_points is None else max_points
    i32 = dict(dtype=torch.int32, device=DEV)
    m, ni = max(cap, 1), max(max_in, 1)
    oxyz = torch.full((m, 3), 5.0, dtype=torch.float64, device=DEV)
    onrm = torch.full((m, 3), 5.0, dtype=torch.float32, device=DEV)
    orgb, oinf = torch.full((m,), 77, **i32), torch.full((m, 4), 77, **i32)
    ptn, cof, rep = torch.full((ni, 3), 77, **i32), torch.full((ni,), 77, **i32), torch.full((8,), 77, **i32)
    dx, ds = dev(xyz if max_in else np.zeros((1, 3)), np.float64), dev(src if max_in else np.zeros((1, 2)), np.int32)
    dd, dv, dP = dev(depth, np.float64), dev(views, np.int32), dev(P, np.float64)
    dc = None if count is None else dev([count, 9, 9, 9], np.int32)
    dcol = None if rgba8 is None else dev(np.asarray(rgba8).astype(np.uint32).view(np.int32), np.int32)
    dids = None if frame_ids is None else dev(frame_ids, np.int32)
    torch.cuda.synchronize()
    engine.cloud_merge_dev(dx, ds, dc, max_in, dd, dv, R, views.shape[1] - 1, W, H, len(P), dP, cell, origin, cap, oxyz, onrm, orgb,
                           oinf, rep, d_rgba8=dcol, F=0 if rgba8 is None else len(rgba8), d_frame_ids=dids, normal_step=k,
                           disc_tol=disc_tol, min_support=min_support, d_pt_normal=ptn if optional else None,
                           d_cell_of=cof if optional else None)
    err = None
    try:
        engine.check_status()
    except pg.CapacityError as e:
        if check:
            raise
        err = e
    return dict(xyz=oxyz.cpu().numpy(), normal=onrm.cpu().numpy(), rgba8=orgb.cpu().numpy().view(np.uint32), info=oinf.cpu().numpy(),
                pt_normal=ptn.cpu().numpy(), cell_of=cof.cpu().numpy(), report=rep.cpu().numpy(), err=err)


@functools.lru_cache(maxsize=None)
def rig():
    """two maps of 16 x 12 with smooth depths and their cameras, colours by slot"""
    W, H = 16, 12
    P = np.stack([depth_ref.scene_camera(c, W, H, 18.0).reshape(12) for c in [(0.0, 0.0, 0.0), (0.3, 0.1, 0.0)]])
    v, u = np.mgrid[0:H, 0:W]
    depth = np.stack([3.0 + 0.02 * u + 0.01 * v, 3.5 - 0.015 * u + 0.005 * v]).astype(np.float64)
    rgba8 = np.random.default_rng(1).integers(0, 2**32, (2, H, W), dtype=np.uint32)
    return dict(depth=depth, views=np.array([[0, 1], [1, 0]], np.int32), P=P, rgba8=rgba8, W=W, H=H)


def synth(n, seed, spread=2.0):
    """n points with random pixels of rig()'s maps, uniform in a box of `spread` (in scene units) about the origin"""
    rng = np.random.default_rng(seed)
    c = dict(rig())
    c["xyz"] = rng.uniform(-spread / 2, spread / 2, (n, 3))
    c["src"] = np.stack([rng.integers(0, 2, n), rng.integers(0, c["W"] * c["H"], n)], 1).astype(np.int32)
    return c
