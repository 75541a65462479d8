"""The scale pyramid on the device (csrc/k_pyramid.hip: k_pyr_down, k_pyr_append; the launch site in csrc/pgx_api.hip) against
the numpy restatement tests/pyramid_ref.py, bit for bit: the resampler at every level for the shapes that reach its 16-byte
store, its row tail at every width modulo 4 and its clamped last row and column; the merged lists of the detect chain through
every entry point that writes them, upright and steered; the mode switched off again; the capacity rules per level and for
the merged list; and the matcher downstream of it on an image and its half-size copy."""
import functools

import numpy as np
import pytest
import torch

import photogrammetry_amd as pg
import pyramid_ref as pr
from match_gpu import run_nn, upload
from oracle import cref
from photogrammetry_amd import synth
from photogrammetry_amd._lib import PGX_E_BADARG, PGX_E_NOT_CONFIGURED
from pyramid_gpu import buffers as _buffers, host as _host, run as _run
from scale_limits_cases import SENT, check_lists as _check_lists

pytestmark = pytest.mark.gpu
W, H, F, T, RADIUS = 161, 140, 3, np.float32(0.1), 4
STEPS = [69632, 78643, 92682, 100000, 131071, 131072]
MODES = [(3, 92682), (8, 78643), (2, 131072)]


@pytest.fixture(scope="module")
def eng():
    e = pg.Engine(0)          # a context of its own: the mode set here stays out of the shared one
    yield e
    e.close()


# ---- the resampler ---------------------------------------------------------------------------------------------------------

def _grey16(w, h, seed):
    """Random float32 grey made from 16-bit values: no intermediate of rule 3 is subnormal."""
    return (np.random.default_rng(seed).integers(0, 65536, (h, w)) / 65535).astype(np.float32)


@pytest.mark.parametrize("step", STEPS)
def test_resampler_every_level(eng, step):
    eng.set_pyramid(8, step)
    h16 = -(-16 * step // 65536)                             # the smallest height whose level 1 has exactly 16 rows
    shapes = [(161, 140), (64, 48), (17, 16), (33, 250), (250, 33), (45, h16)] + [(w, 37) for w in range(128, 136)]
    assert pr.dims(45, h16, 2, step)[0][1, 1] == 16
    widths_mod4, levels_seen = set(), 0
    for i, (w, h) in enumerate(shapes):
        g = _grey16(w, h, 100 + i)
        ref = pr.levels(g, 8, step)
        for l, e in enumerate(ref):
            if e is None:
                with pytest.raises(pg.PgxError) as ex:       # an empty level has no image
                    eng.pyramid_level(g, l)
                assert ex.value.code == PGX_E_BADARG
                break
            got = eng.pyramid_level(g, l)
            assert got.shape == e.shape and got.dtype == np.float32
            assert (got.view(np.uint32) == e.view(np.uint32)).all(), (w, h, step, l)
            if l:
                widths_mod4.add(e.shape[1] % 4)
                levels_seen += 1
    assert widths_mod4 == {0, 1, 2, 3} and levels_seen >= len(shapes) - 1      # every shape but 17 x 16 has a level 1
    with pytest.raises(pg.PgxError) as ex:
        eng.pyramid_level(_grey16(64, 48, 1), 8)
    assert ex.value.code == PGX_E_BADARG
    with pytest.raises(pg.PgxError) as ex:
        eng.pyramid_level(_grey16(64, 48, 1), -1)
    assert ex.value.code == PGX_E_BADARG
    eng.set_pyramid(1, step)


def test_resampler_large_frame(eng):
    """More than one workgroup per row and per column block: 1030 x 70 (five 16-byte-aligned column blocks and a tail)."""
    eng.set_pyramid(3, 92682)
    g = _grey16(1030, 70, 9)
    ref = pr.levels(g, 3, 92682)
    for l in range(3):
        assert (eng.pyramid_level(g, l).view(np.uint32) == ref[l].view(np.uint32)).all()
    eng.set_pyramid(1, 92682)


# ---- the chain ---------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _frames(w=W, h=H, n=F):
    return np.stack([synth.make_frame(w, h, seed=1 + i) for i in range(n)])


@functools.lru_cache(maxsize=None)
def _tables(P):
    pairs = pg.make_brief_pairs(3, 8, P)
    rot, dirs = pg.make_steering(pairs, 32)
    return pairs, rot, dirs


@functools.lru_cache(maxsize=None)
def _ref(n_levels, step, P, steered, capacity=None, raw_cap=None, kp_cap=None, w=W, h=H):
    """The restatement's lists of the frames, computed once per configuration and left unchanged."""
    pairs, rot, dirs = _tables(P)
    return [pr.detect_pyramid(cref.gray(f), n_levels, step, T, RADIUS, pairs, capacity=capacity, raw_cap=raw_cap, kp_cap=kp_cap,
                              steer=(rot, dirs, 15) if steered else None) for f in _frames(w, h)]


def _configure(eng, P, steered, n_levels, step, raw_cap=1 << 16, kp_cap=1 << 20):
    pairs, rot, dirs = _tables(P)
    eng.set_detect_params(T, RADIUS)
    eng.set_capacity(raw_cap, kp_cap)
    eng.set_dewarp_map(None)
    eng.set_brief_pairs(pairs)                               # turns steering off
    if steered:
        eng.set_brief_steering(rot, dirs, 15)
    eng.set_pyramid(n_levels, step)


@pytest.mark.parametrize("steered", [False, True])
@pytest.mark.parametrize("P", [256, 33])
@pytest.mark.parametrize("n_levels,step", MODES)
def test_chain_equals_the_restatement(eng, n_levels, step, P, steered):
    cap, words = 4096, (P + 31) // 32
    ref = _ref(n_levels, step, P, steered)
    assert all(r["total"] < cap and r["count"] == r["total"] for r in ref)
    assert all((r["stats"][:min(n_levels, 3), 0] > 0).all() for r in ref)     # more than one level contributes
    _configure(eng, P, steered, n_levels, step)
    frames = _frames()
    got = _run(eng, frames, cap, words, n_levels, bins=steered)
    _check_lists(got, ref, cap, bins=steered)
    if not steered:
        assert (got["bins"] == SENT).all()
    # the other entry points share the launch site and give the same lists
    plain = _run(eng, frames, cap, words, n_levels, entry="plain")
    _check_lists(plain, ref, cap, origin=False)
    if steered:
        st = _run(eng, frames, cap, words, n_levels, entry="steered")
        _check_lists(st, ref, cap, origin=False, bins=True)
    if P == 256:                                             # the matcher behind it is not what this test is about
        seq = _run(eng, frames, cap, words, n_levels, entry="sequence")
        _check_lists(seq, ref, cap, origin=False)
    kp, desc, nraw = eng.detect(frames[1], capacity=cap)
    assert kp.tobytes() == ref[1]["kp"].tobytes() and (desc == ref[1]["desc"]).all() and nraw == ref[1]["nraw"]
    out = eng.detect_pyramid(frames[2], capacity=cap, bins=steered)
    assert out[0].tobytes() == ref[2]["kp"].tobytes() and (out[1] == ref[2]["desc"]).all()
    assert (out[2] == ref[2]["origin"]).all() and (out[3] == ref[2]["stats"]).all() and out[4] == ref[2]["nraw"]
    if steered:
        assert (out[5] == ref[2]["bins"]).all()
    eng.set_brief_steering(None)
    eng.set_pyramid(1, step)


def test_mode_off_is_bit_identical(eng):
    cap = 2048
    _configure(eng, 256, False, 1, 92682)
    frames = _frames()
    before = _run(eng, frames, cap, 8, 1, entry="plain")
    assert before["counts"].min() > 30
    one = _ref(1, 92682, 256, False)
    _check_lists(before, one, cap, origin=False)             # the single scale is the restatement's one-level list
    for fn in (lambda: _run(eng, frames, cap, 8, 3), lambda: eng.pyramid_level(np.zeros((H, W), np.float32), 0)):
        with pytest.raises(pg.PgxError) as ex:
            fn()
        assert ex.value.code == PGX_E_NOT_CONFIGURED
    eng.set_pyramid(3, 92682)
    on = _run(eng, frames, cap, 8, 3, entry="plain")
    assert (on["counts"] > before["counts"]).all()
    eng.set_pyramid(1, 92682)
    after = _run(eng, frames, cap, 8, 1, entry="plain")
    for k in before:
        assert before[k].tobytes() == after[k].tobytes(), k
    with pytest.raises(pg.PgxError) as ex:
        _run(eng, frames, cap, 8, 3)
    assert ex.value.code == PGX_E_NOT_CONFIGURED
    for n, step in [(0, 92682), (9, 92682), (3, 69631), (3, 131073)]:
        with pytest.raises(pg.ArgumentException):
            eng.set_pyramid(n, step)
    eng.set_pyramid(2, 131072)
    with pytest.raises(pg.PgxError) as ex:                   # bins asked for without steering
        _run(eng, frames, cap, 8, 2, bins=True)
    assert ex.value.code == PGX_E_NOT_CONFIGURED
    eng.set_pyramid(1, 92682)


# ---- limits ----------------------------------------------------------------------------------------------------------------------

def test_capacity_of_the_merged_list(eng):
    n_levels, step = 3, 92682
    totals = sorted(r["total"] for r in _ref(n_levels, step, 256, False))
    assert totals[0] < totals[1] < totals[2]
    _configure(eng, 256, False, n_levels, step)
    cap = totals[1]                                          # one frame below, one exactly at, one above the capacity
    ref = _ref(n_levels, step, 256, False, capacity=cap)
    got = _run(eng, _frames(), cap, 8, n_levels, expect=pg.CapacityError)
    assert sorted(got["counts"].tolist()) == [totals[0], cap, cap]
    _check_lists(got, ref, cap)
    cap = totals[2]                                          # the largest total fits exactly: no error
    got = _run(eng, _frames(), cap, 8, n_levels)
    _check_lists(got, _ref(n_levels, step, 256, False, capacity=cap), cap)
    eng.set_pyramid(1, step)


def test_survivor_limit_cuts_every_level(eng):
    n_levels, step, cap = 3, 92682, 1024
    ref = _ref(n_levels, step, 256, False, kp_cap=50)
    assert all((r["stats"][:, 0] == 50).all() for r in ref)  # every level had more than 50
    _configure(eng, 256, False, n_levels, step, kp_cap=50)
    _check_lists(_run(eng, _frames(), cap, 8, n_levels), ref, cap)
    eng.set_capacity(1 << 16, 1 << 20)
    eng.set_pyramid(1, step)


def test_raw_limit_exceeded_by_one_level(eng):
    n_levels, step, cap = 3, 92682, 4096
    raws = np.array([r["stats"][:, 1] for r in _ref(n_levels, step, 256, False)])
    top = np.sort(raws.reshape(-1))[::-1]
    assert top[0] > top[1] + 1
    raw_cap = int(top[0] + top[1]) // 2                      # exactly one level of one frame has more raw hits
    ref = _ref(n_levels, step, 256, False, raw_cap=raw_cap)
    assert sum(r["raw_over"] for r in ref) == 1 and (np.array([r["stats"][:, 1] for r in ref]) == raws).all()
    _configure(eng, 256, False, n_levels, step, raw_cap=raw_cap)
    got = _run(eng, _frames(), cap, 8, n_levels, expect=pg.CapacityError)
    _check_lists(got, ref, cap)
    eng.set_capacity(1 << 16, 1 << 20)
    eng.set_pyramid(1, step)


def test_small_frame_and_no_frames(eng):
    cap = 512
    _configure(eng, 256, False, 8, 131072)
    ref = _ref(8, 131072, 256, False, w=40, h=30)            # 20 x 15: empty from level 1
    assert all(r["stats"][1:].sum() == 0 for r in ref)
    got = _run(eng, _frames(40, 30), cap, 8, 8)
    _check_lists(got, ref, cap)
    assert (got["origin"][:, :, 0][got["origin"][:, :, 0] != SENT] == 0).all()
    b = _buffers(1, cap, 8, 8)
    torch.cuda.synchronize()
    eng.detect_batch_pyramid_dev(b["kp"], 0, 40, 30, b["kp"], b["desc"], b["counts"], b["nraw"], cap, b["origin"], b["stats"])
    eng.check_status()
    assert all((v == SENT).all() for v in _host(b).values())  # F = 0 writes nothing
    eng.set_pyramid(1, 131072)


# ---- downstream --------------------------------------------------------------------------------------------------------------------

def test_matcher_downstream_of_the_pyramid(eng):
    """The zoom case of tests/test_pyramid_ref.py (seed 5) through the device: A through the pyramid chain, its half-size copy B
    through the stage kernels on B's grey, both descriptor sets in one buffer, pgx_match_nn_batch_dev on the pair."""
    case = pr.quality_case(5)
    ra, rb = case["ref_a"], case["ref_b"]
    stride = 4608
    assert ra["count"] < stride
    eng.set_detect_params(T, 6)
    eng.set_capacity(1 << 16, 1 << 20)
    eng.set_dewarp_map(None)
    eng.set_brief_pairs(case["pairs"])
    eng.set_pyramid(4, 92682)
    a = _run(eng, case["frame"][None], stride, 8, 4)
    _check_lists(a, [ra], stride)
    hb, wb = case["B"].shape
    raw_b = eng.fast(case["B"])
    kept_b = raw_b[eng.nms(raw_b, wb, hb)]
    desc_b = eng.brief(case["B"], kept_b)
    assert kept_b.tobytes() == rb["kp"].tobytes() and (desc_b == rb["desc"]).all()
    na = int(a["counts"][0])
    dev = upload(stride, 8, [a["desc"][0, :na].view(np.uint32), desc_b])
    got = run_nn(eng, dev, stride, 8, [(0, 1)], 64, 0.8, True)[0, :na]
    assert (got == case["sel"]).all()
    kp_a = np.ascontiguousarray(a["kp"][0, :na]).view(pg.KEYPOINT_DTYPE).reshape(-1)
    assert pr.correct_matches(kp_a, kept_b, got) == case["pyramid"]
    assert case["pyramid"][1] >= 300
    eng.set_pyramid(1, 92682)
