"""What the GPU tests of the dense stage and of the host forms share (test_gpu_depth.py, test_gpu_host_forms.py): the run
wrappers of pgx_depth_maps_dev and pgx_depth_fuse_dev with sentinel-filled outputs, and the seeded noise case.  The engine is
always the caller's.  A plain helper module: no test module imports another."""
import numpy as np
import torch

import depth_ref as ref
import photogrammetry_amd as pg

DEV = "cuda:0"
BIG = 2**30


def dev(a, dtype):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).to(DEV)


def run_maps(engine, gray, P, views, ranges, D, a=2, min_views=1, max_cost=BIG, frame_ids=None, n_frames=None, optional=True):
    """pgx_depth_maps_dev on sentinel-filled outputs, one sync -> dict of host arrays"""
    gray = np.asarray(gray, dtype=np.float32)
    F, H, W = gray.shape
    views = np.asarray(views, dtype=np.int32)
    R, S = views.shape[0], views.shape[1] - 1
    nf = F if n_frames is None else n_frames
    dg, dP, dv, dr = dev(gray, np.float32), dev(np.reshape(P, (nf, 12)), np.float64), dev(views, np.int32), dev(np.reshape(ranges, (R, 2)), np.float64)
    ids = None if frame_ids is None else dev(frame_ids, np.int32)
    i32 = dict(dtype=torch.int32, device=DEV)
    kq8, fl, cost = torch.full((R, H, W), 77, **i32), torch.full((R, H, W), 77, **i32), torch.full((R, H, W), 77, **i32)
    dep = torch.full((R, H, W), 5.0, dtype=torch.float64, device=DEV)
    warp = torch.full((R, S, 12), 5.0, dtype=torch.float64, device=DEV)
    planes = torch.full((R, D), 5.0, dtype=torch.float64, device=DEV)
    summary = torch.full((8,), 77, **i32)
    torch.cuda.synchronize()
    engine.depth_maps_dev(dg, F, W, H, nf, dP, dv, R, S, dr, D, kq8, dep, fl, summary, agg_radius=a, min_views=min_views,
                          max_cost=max_cost, d_cost=cost if optional else None, d_warp=warp if optional else None,
                          d_planes=planes if optional else None, d_frame_ids=ids)
    engine.check_status()
    return dict(kq8=kq8.cpu().numpy(), depth=dep.cpu().numpy(), cost=cost.cpu().numpy(), flags=fl.cpu().numpy(),
                warp=warp.cpu().numpy(), planes=planes.cpu().numpy(), summary=summary.cpu().numpy())


def make_case(W, H, n, seed, f=None):
    """n frames of seeded noise and cameras R = I near the origin, the first at it; planes over depths [2, 6]"""
    rng = np.random.default_rng(seed)
    gray = rng.random((n, H, W)).astype(np.float32)
    C = np.c_[rng.uniform(-0.4, 0.4, (n, 2)), rng.uniform(-0.1, 0.1, n)]
    C[0] = 0.0
    f = 1.2 * max(W, H, 8) if f is None else f
    return gray, np.stack([ref.scene_camera(c, W, H, f).reshape(12) for c in C])


def run_fuse(engine, depth, views, P, rel_tol=0.05, min_agree=2, max_points=None, agree=True, check=True):
    depth = np.asarray(depth, dtype=np.float64)
    R, H, W = depth.shape
    views = np.asarray(views, dtype=np.int32)
    P = np.reshape(P, (-1, 12))
    cap = R * H * W if max_points is None else max_points
    i32 = dict(dtype=torch.int32, device=DEV)
    xyz = torch.full((max(cap, 1), 3), 5.0, dtype=torch.float64, device=DEV)
    src, ag, summary = torch.full((max(cap, 1), 2), 77, **i32), torch.full((R, H, W), 77, **i32), torch.full((4,), 77, **i32)
    dd, dv, dP = dev(depth, np.float64), dev(views, np.int32), dev(P, np.float64)
    torch.cuda.synchronize()
    engine.depth_fuse_dev(dd, dv, R, views.shape[1] - 1, W, H, len(P), dP, cap, xyz, src, summary, rel_tol=rel_tol,
                          min_agree=min_agree, d_agree=ag if agree else None)
    err = None
    try:
        engine.check_status()
    except pg.CapacityError as e:
        if check:
            raise
        err = e
    return dict(xyz=xyz.cpu().numpy(), src=src.cpu().numpy(), agree=ag.cpu().numpy(), summary=summary.cpu().numpy(), err=err)
