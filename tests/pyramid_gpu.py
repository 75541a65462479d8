"""What the GPU tests of the scale pyramid and of steered BRIEF share (tests/test_gpu_pyramid.py,
tests/test_gpu_scale_limits.py): sentinel-filled output buffers and the run wrapper of the batched detect entry points.  The
engine is always the caller's; the comparison with the restatement is scale_limits_cases.check_lists (no torch).  A plain
helper module: no test module imports another."""
import pytest
import torch

from match_gpu import DEV, I32
from scale_limits_cases import SENT


def buffers(nf, cap, words, n_levels):
    return dict(kp=torch.full((nf, cap, 4), SENT, **I32), desc=torch.full((nf, cap, words), SENT, **I32),
                counts=torch.full((nf,), SENT, **I32), nraw=torch.full((nf,), SENT, **I32),
                origin=torch.full((nf, cap, 3), SENT, **I32), stats=torch.full((nf, n_levels, 2), SENT, **I32),
                bins=torch.full((nf, cap), SENT, **I32))


def host(b):
    return {k: v.cpu().numpy() for k, v in b.items()}


def run(eng, frames, cap, words, n_levels, entry="pyramid", bins=False, expect=None):
    """One of the batched entry points on host frames -> host arrays (sentinel-filled where nothing was written).  expect: an
    exception class check_status must raise."""
    nf, h, w = frames.shape[:3]
    d_frames = torch.from_numpy(frames).to(DEV)
    b = buffers(nf, cap, words, n_levels)
    torch.cuda.synchronize()   # torch's fills run on ITS stream; the engine's non-blocking stream does not order against it
    if entry == "pyramid":
        eng.detect_batch_pyramid_dev(d_frames, nf, w, h, b["kp"], b["desc"], b["counts"], b["nraw"], cap, b["origin"], b["stats"],
                                     b["bins"] if bins else None)
    elif entry == "plain":
        eng.detect_batch_dev(d_frames, nf, w, h, b["kp"], b["desc"], b["counts"], b["nraw"], cap)
    elif entry == "steered":
        eng.detect_batch_steered_dev(d_frames, nf, w, h, b["kp"], b["desc"], b["counts"], b["nraw"], cap, b["bins"])
    else:
        assert entry == "sequence"
        pl = torch.tensor([[0, 1]], **I32)
        out = torch.full((1, cap, 3), SENT, **I32)
        torch.cuda.synchronize()
        eng.sequence_step_dev(d_frames, nf, nf, w, h, b["kp"], b["desc"], b["counts"], b["nraw"], cap, pl, 1, 1, out)
    if expect is None:
        eng.check_status()
    else:
        with pytest.raises(expect):
            eng.check_status()
    return host(b)
