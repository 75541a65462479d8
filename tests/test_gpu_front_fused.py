"""GPU tests of the batch path's fused level 0: dewarp, grey and FAST in one tile kernel (photogrammetry_amd/csrc/k_fast.hip:
k_dewarp_fast) off the gather plan that is made when a map is installed (csrc/k_image.hip: k_dewarp_plan).
pgx_detect_batch_dev is held to the oracle chain cref.apply_distortion -> gray -> detect -> nms -> brief, bit for bit: the raw
count, the keypoints in NMS order, their scores, the bits of their grey values and their descriptors, and the rows behind a
list untouched.  The scenes are tests/front_fused_cases.py's (what each is for is asserted in tests/test_front_fused_cases.py
on the oracle alone): frame sizes on both sides of the 64 x 32 tile, batches on both sides of the kernel's frame group of
eight, maps without and with entries outside the image -- whose pixels are black and raise PGX_ST_OOB_SOURCE once per call,
as tests/test_gpu_parity.py and tests/test_gpu_front_limits.py check it for the unfused kernel -- and both source formats.
The expectation of a frame does not depend on the batch it is in, so it is computed once per (size, map) and shared."""
import numpy as np
import pytest

import front_fused_cases as ff
import pyramid_ref as pr
from match_gpu import detect_equal, run_detect
from oracle import cref
import photogrammetry_amd as pg
from pyramid_gpu import run as run_pyramid
from scale_limits_cases import check_lists

pytestmark = pytest.mark.gpu

SENT = -7


@pytest.fixture(scope="module")
def eng():
    e = pg.Engine(0)
    e.set_dewarp_map(None)
    yield e
    e.set_source_format(pg.api.PGX_SRC_RGBA64)
    e.close()


def _configure(eng, src8=0):
    eng.set_brief_pairs(ff.brief_pairs())
    eng.set_detect_params(ff.T, ff.RADIUS)
    eng.set_capacity(ff.RAW, 1 << 20)
    eng.set_pyramid(1, 92682)
    eng.set_source_format(pg.api.PGX_SRC_RGBA8 if src8 else pg.api.PGX_SRC_RGBA64)


def _run(eng, host, exp, oob):
    """one call on the first len(host) frames; every frame against the oracle's triple; the status word"""
    out = run_detect(eng, host, ff.CAP, sentinel=SENT)
    if oob:
        with pytest.raises(pg.IndexOutOfRangeException):
            eng.check_status()
        eng.check_status()                                                   # raised once: the word is clean again
    else:
        eng.check_status()
    out = [t.cpu() for t in out]                                             # one download per call, behind check_status' wait
    for f in range(len(host)):
        detect_equal(out, f, *exp[f], sentinel=SENT)


@pytest.mark.parametrize("src8", [0, 1])
@pytest.mark.parametrize("kind", ff.MAPS)
@pytest.mark.parametrize("w,h", ff.SIZES)
def test_batches_equal_the_oracle_chain(eng, w, h, kind, src8):
    frames, dmap, exp = ff.scene(w, h, kind)
    host = (frames // 257).astype(np.uint8) if src8 else frames
    oob = dmap is not None and bool(ff.outside(dmap).any())
    _configure(eng, src8)
    try:
        eng.set_dewarp_map(dmap)
        for F in ff.BATCHES:
            _run(eng, np.ascontiguousarray(host[:F]), exp, oob)
    finally:
        eng.set_source_format(pg.api.PGX_SRC_RGBA64)
        eng.set_dewarp_map(None)


@pytest.mark.parametrize("w,h", [(83, 60), (65, 33)])
def test_map_replaced_then_cleared(eng, w, h):
    """the plan is rebuilt behind every map and dropped with it: flip -> shift (entries outside: the status) -> flip again ->
    no map -> one entry outside, every call against its own oracle lists"""
    frames = ff.scene(w, h, "none")[0][:3]
    _configure(eng)
    try:
        for kind in ("flip", "shift", "flip", "none", "halo"):
            _, dmap, exp = ff.scene(w, h, kind)
            eng.set_dewarp_map(dmap)
            _run(eng, frames, exp, kind in ("shift", "halo"))
    finally:
        eng.set_dewarp_map(None)


def test_the_map_built_from_coefficients_gets_its_plan_too(eng):
    """pgx_set_dewarp_coeffs installs the map on the device; the chain then gathers through the plan of exactly that map"""
    w, h = 200, 131
    frames = ff.scene(w, h, "none")[0][:3]
    _configure(eng)
    try:
        eng.set_dewarp_coeffs(w, h, [3e-4, 1e-7, 0, 0, 0])
        dmap = eng.get_dewarp_map(w, h)
        assert not ff.outside(dmap).any()
        _run(eng, frames, [ff.chain(f, dmap, ff.brief_pairs()) for f in frames], False)
    finally:
        eng.set_dewarp_map(None)


def test_pyramid_level_0_fused_level_1_not(eng):
    """two levels: level 0 comes from the fused kernel, level 1 from k_pyr_down of the grey plane it stored and k_fast_planes"""
    w, h, step, P = 161, 140, 92682, 256
    from photogrammetry_amd import synth
    frames = np.stack([synth.make_frame(w, h, seed=1 + i) for i in range(3)])
    dmap = ff.make_map("flip", w, h)
    pairs = pg.make_brief_pairs(3, 8, P)
    T, radius, cap = np.float32(0.1), 4, 4096
    ref = [pr.detect_pyramid(cref.gray(ff.dewarp(f, dmap)), 2, step, T, radius, pairs) for f in frames]
    assert all((r["stats"][:2, 0] > 0).all() and r["count"] == r["total"] < cap for r in ref)   # both levels contribute
    eng.set_brief_pairs(pairs)
    eng.set_detect_params(T, radius)
    eng.set_capacity(1 << 16, 1 << 20)
    try:
        eng.set_dewarp_map(dmap)
        eng.set_pyramid(2, step)
        check_lists(run_pyramid(eng, frames, cap, 8, 2), ref, cap)
    finally:
        eng.set_pyramid(1, step)
        eng.set_dewarp_map(None)
