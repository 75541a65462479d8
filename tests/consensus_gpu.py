"""What the GPU tests of track consensus and of the host forms share (test_gpu_consensus.py, test_gpu_consensus_limits.py,
test_gpu_host_forms.py): the run wrapper of pgx_track_consensus_dev with sentinel-filled outputs.  The engine is always
the caller's.  A plain helper module: no test module imports another."""
import numpy as np
import pytest
import torch

from geom_gpu import DEV, F64, I32

DEFAULTS = dict(inlier_px=4.0, min_parallax_deg=1.0, min_inliers=2, min_len=2, max_hyp=256, seed=0)
IN_SUMMARY = (21, 22, 23, 99, 24, 5)       # slots 2 .. 7 of the input summary: 2, 3, 4, 6 are copied, 5 and 7 are not


def run(engine, d, P, max_tracks=None, track_of=None, raises=None, in_summary=IN_SUMMARY, **kw):
    """pgx_track_consensus_dev on synth.device_tracks' buffers, one sync -> dict of host arrays (sentinels cut off)"""
    kw = dict(DEFAULTS, **kw)
    nf, stride, n = d["nf"], d["stride"], d["n_tracks"]
    N = nf * stride
    mt = n if max_tracks is None else max_tracks
    tsum = d["tsum"].clone()
    tsum[2:8] = torch.tensor(in_summary, **I32)
    off_out, nodes_out = torch.full((mt + 1,), 77, **I32), torch.full((N, 2), 77, **I32)
    sum_out, report = torch.full((8,), 77, **I32), torch.full((8,), 77, **I32)
    tmap, stats = torch.full((max(mt, 1),), 77, **I32), torch.full((max(mt, 1), 4), 77, **I32)
    xyz, flags = torch.full((max(mt, 1), 3), 5.0, **F64), torch.full((max(mt, 1),), 77, **I32)
    dP = torch.from_numpy(np.ascontiguousarray(P, dtype=np.float64).reshape(nf, 12)).to(DEV)
    dto = None if track_of is None else torch.from_numpy(np.ascontiguousarray(track_of, np.int32)).to(DEV)
    torch.cuda.synchronize()
    engine.track_consensus_dev(d["kp"], d["F"], stride, nf, dP, d["off"], d["nodes"], tsum, mt, off_out, nodes_out, sum_out, tmap,
                               xyz, flags, stats, report, d_track_of=dto, d_frame_ids=None if d["identity"] else d["ids"], **kw)
    if raises is None:
        engine.check_status()
    else:
        with pytest.raises(raises):
            engine.check_status()
    s = sum_out.cpu().numpy()
    n_in = min(n, mt)
    assert (tmap.cpu().numpy()[n_in:] == 77).all() and (off_out.cpu().numpy()[s[0] + 1:] == 77).all()
    assert (nodes_out.cpu().numpy()[s[1]:] == 77).all() and (flags.cpu().numpy()[s[0]:] == 77).all()
    return dict(offsets=off_out.cpu().numpy()[:s[0] + 1], nodes=nodes_out.cpu().numpy()[:s[1]], summary=s,
                map=tmap.cpu().numpy()[:n_in], xyz=xyz.cpu().numpy()[:s[0]], flags=flags.cpu().numpy()[:s[0]],
                stats=stats.cpu().numpy()[:n_in], report=report.cpu().numpy(), track_of=None if dto is None else dto.cpu().numpy())
