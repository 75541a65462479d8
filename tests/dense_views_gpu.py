"""What the GPU tests of the dense stage's plan and of the host forms share (test_gpu_dense_views.py,
test_gpu_host_forms.py): the device buffers, the call and the run wrapper of pgx_dense_views_dev with sentinel-filled
outputs.  The engine is always the caller's.  A plain helper module: no test module imports another."""
import numpy as np
import torch

import dense_views_ref as ref
import photogrammetry_amd as pg
from geom_gpu import DEV, F64, I32

KEYS = ("views", "range", "pair_counts", "ref_stats", "report")


def dev(a, dtype):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).to(DEV)


def buffers(off, nd, xyz, flags, P, refs, S, max_tracks=None, max_nodes=None, pair_counts=True):
    """the device inputs (points and flags padded to the capacity: 3.0 and 0 behind n_tracks) and sentinel-filled outputs"""
    off, nd = np.asarray(off, np.int32).reshape(-1), np.asarray(nd, np.int32).reshape(-1, 2)
    n, nf = len(off) - 1, len(np.reshape(P, (-1, 12)))
    mt = n if max_tracks is None else max_tracks
    rows = max(mt, n, 1)
    X = np.full((rows, 3), 3.0)
    X[:n] = np.reshape(xyz, (n, 3))
    fl = None
    if flags is not None:
        fl = np.zeros(rows, np.int32)
        fl[:n] = flags
    R = nf if refs is None else len(refs)
    b = dict(off=dev(off, np.int32), nodes=dev(nd if len(nd) else np.zeros((1, 2)), np.int32),
             tsum=torch.tensor([n, len(nd), 0, 0, 0, 0, 0, 0], **I32), max_tracks=mt, max_nodes=len(nd) if max_nodes is None else max_nodes,
             xyz=dev(X, np.float64), flags=None if fl is None else dev(fl, np.int32), nf=nf, P=dev(np.reshape(P, (nf, 12)), np.float64),
             refs=None if refs is None else dev(refs, np.int32), R=R, S=S,
             views=torch.full((R, 1 + S), 77, **I32), range=torch.full((R, 2), 5.0, **F64),
             pair_counts=torch.full((R, nf, 2), 77, **I32) if pair_counts else None, ref_stats=torch.full((R, 4), 77, **I32),
             report=torch.full((8,), 77, **I32))
    return b


def call(engine, b, **kw):
    engine.dense_views_dev(b["off"], b["nodes"], b["tsum"], b["max_tracks"], b["max_nodes"], b["xyz"], b["nf"], b["P"], b["R"], b["S"],
                           b["views"], b["range"], b["ref_stats"], b["report"], d_track_flags=b["flags"], d_refs=b["refs"],
                           d_pair_counts=b["pair_counts"], **dict(ref.DEFAULTS, **kw))


def outputs(b):
    return {k: (None if b[k] is None else b[k].cpu().numpy()) for k in KEYS}


def run(engine, off, nd, xyz, flags, P, refs, S, max_tracks=None, max_nodes=None, pair_counts=True, **kw):
    """pgx_dense_views_dev, one sync -> dict of host arrays and `status` as the yardstick names it"""
    b = buffers(off, nd, xyz, flags, P, refs, S, max_tracks, max_nodes, pair_counts)
    torch.cuda.synchronize()
    call(engine, b, **kw)
    status = set()
    try:
        engine.check_status()
    except pg.CapacityError:
        status.add("cap")
    except pg.ArgumentException:
        status.add("node")
    return dict(outputs(b), status=status)
