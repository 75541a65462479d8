"""Steered BRIEF on the device (csrc/k_steer.hip: k_orient_list, k_steer_list, k_steer_kept) against the numpy restatement
tests/steered_ref.py, bit for bit: bins and descriptors of explicit keypoint lists at every border distance that changes what
the disc sees, for the radii, direction counts and table sizes that take different paths (P == 256: the per-direction sample
plans; other P: the turned tables themselves), the quantisation of awkward grey values, the tie rule, the fused detect chain
(both branches of its block -> frame map), switching the mode on and off, and the quarter-turn invariance the mode is for."""
import numpy as np
import pytest
import torch

import front_limits_cases as fc
import photogrammetry_amd as pg
import steered_ref as sr
from match_gpu import DEV
from oracle import cref
from photogrammetry_amd import synth
from photogrammetry_amd._lib import PGX_E_NOT_CONFIGURED
from photogrammetry_amd.api import _ptr
from scale_limits_cases import points as _points

pytestmark = pytest.mark.gpu
W, H = 161, 140


@pytest.fixture(scope="module")
def eng():
    e = pg.Engine(0)          # a context of its own: the tables set here stay out of the shared one
    yield e
    e.close()


@pytest.fixture(scope="module")
def image():
    """Smooth ground (a clear centroid) plus noise (descriptor bits that depend on the exact samples), float32 in [0, 1]."""
    noise = np.random.default_rng(1).random((H, W)).astype(np.float32)
    return np.ascontiguousarray((np.float32(0.6) * sr.smooth_image(W, H, 2) + np.float32(0.4) * noise).astype(np.float32))


def _kps(xy):
    k = np.zeros(len(xy), dtype=pg.KEYPOINT_DTYPE)
    if len(xy):
        k["x"], k["y"] = np.asarray(xy)[:, 0], np.asarray(xy)[:, 1]
    return k


def _table(P, seed=21, reach=20):
    return np.random.default_rng(seed + P).integers(-reach, reach + 1, (P, 4)).astype(np.int32)


def _set(eng, pairs, B, R):
    rot, dirs = pg.make_steering(pairs, B)
    eng.set_brief_pairs(pairs)
    eng.set_brief_steering(rot, dirs, R)
    return rot, dirs


def _check_list(eng, g, xy, rot, dirs, R):
    eb, ed = sr.describe(g, xy, rot, dirs, R)
    gb, gd = eng.orient(g, _kps(xy)), eng.brief(g, _kps(xy))
    assert gb.dtype == np.int32 and gb.tolist() == eb.tolist()
    assert gd.shape == ed.shape and (gd == ed).all()
    return eb, ed


@pytest.mark.parametrize("P", [33, 256, 320])
@pytest.mark.parametrize("B", [4, 32, 64])
@pytest.mark.parametrize("R", [1, 15, 31])
def test_list_form(eng, image, R, B, P):
    rot, dirs = _set(eng, _table(P), B, R)
    xy = _points(W, H, R)
    eb, ed = _check_list(eng, image, xy, rot, dirs, R)
    if R > 1:
        assert len(np.unique(eb)) >= 3 and ed.any()          # the case exercises more than one direction's table
    for n in (0, 1, 5, 9):                                   # an empty list, less than one workgroup, two and three of them
        _check_list(eng, image, xy[:n], rot, dirs, R)


def test_quantisation_of_awkward_grey_values(eng):
    rng = np.random.default_rng(3)
    ks = np.array([0, 1, 2, 3, 100, 101, 32766, 32767, 32768, 65533, 65534], np.float64)
    pool = np.concatenate([np.array([np.nan, np.inf, -np.inf, -1.0, 2.0, 1.0, 0.0, -0.0, 1e-40, -1e-40, 1.4e-45], np.float32),
                           ((ks + 0.5) / 65535).astype(np.float32), (ks / 65535).astype(np.float32)])
    g = pool[rng.integers(0, len(pool), (H, W))]
    mix = rng.random((H, W)) < 0.5
    g[mix] = rng.random((H, W)).astype(np.float32)[mix]
    g = np.ascontiguousarray(g, dtype=np.float32)
    assert np.isnan(g).sum() > 100 and np.isinf(g).sum() > 100
    q = sr.quantise(pool)
    assert q[:11].tolist() == [0, 65535, 0, 0, 65535, 65535, 0, 0, 0, 0, 0] and q.min() == 0 and q.max() == 65535
    for R, B, P in [(15, 32, 256), (31, 64, 33), (2, 4, 256)]:
        rot, dirs = _set(eng, _table(P), B, R)
        _check_list(eng, g, _points(W, H, R), rot, dirs, R)


def test_flat_patches_and_ties_take_the_smallest_bin(eng):
    pairs = _table(256)
    c = np.array([(80, 70)], np.int32)
    for B in (4, 8, 32):
        rot, dirs = _set(eng, pairs, B, 15)
        flat = np.full((H, W), 0.37, np.float32)
        assert sr.bins(flat, c, dirs, 15).tolist() == [0] and eng.orient(flat, _kps(c)).tolist() == [0]
        _check_list(eng, flat, c, rot, dirs, 15)
    # one bright pixel on a diagonal: with B = 4 its two neighbouring directions tie and the smaller k wins; with B = 8 the
    # diagonal is a direction of its own
    for B, want in [(4, [0, 1, 2, 0]), (8, [1, 3, 5, 7])]:
        rot, dirs = _set(eng, pairs, B, 15)
        for (dx, dy), k in zip([(3, 3), (-3, 3), (-3, -3), (3, -3)], want):
            g = np.zeros((H, W), np.float32)
            g[70 + dy, 80 + dx] = 1.0
            s = sr.scores(g, c, dirs, 15)[0]
            if B == 4:
                assert (s == s.max()).sum() == 2             # the case is a tie
            assert sr.bins(g, c, dirs, 15).tolist() == [k] and eng.orient(g, _kps(c)).tolist() == [k]
    # a tie between directions 0 and 1 of B = 8: m10 = 11585, m01 = 4799 give s_0 = 11585 * 16384 = (11585 + 4799) * 11585 = s_1
    rot, dirs = _set(eng, pairs, 8, 15)
    assert dirs[0].tolist() == [16384, 0] and dirs[1].tolist() == [11585, 11585]
    g = np.zeros((H, W), np.float32)
    g[70, 81], g[71, 80] = np.float32(11585 / 65535), np.float32(4799 / 65535)
    m10, m01 = sr.moments(g, c, 15)
    assert (int(m10[0]), int(m01[0])) == (11585, 4799)
    s = sr.scores(g, c, dirs, 15)[0]
    assert s[0] == s[1] == s.max()
    assert eng.orient(g, _kps(c)).tolist() == [0]
    g[70, 81], g[71, 80] = g[71, 80], g[70, 81]              # mirrored: directions 1 and 2 tie
    s = sr.scores(g, c, dirs, 15)[0]
    assert s[1] == s[2] == s.max() and eng.orient(g, _kps(c)).tolist() == [1]


@pytest.mark.parametrize("B,R,reach", [(4, 15, 9), (8, 15, 9), (32, 15, 14), (64, 31, 28)])
def test_a_bright_pixel_along_each_direction_gets_that_bin(eng, B, R, reach):
    """B = 4 and 8: the pixel lies exactly on the direction.  B = 32 and 64: at the nearest pixel `reach` away, whose angle is
    off by at most atan(0.71 / reach) -- 2.9 and 1.5 degrees, inside the half bins of 5.6 and 2.8."""
    rot, dirs = _set(eng, _table(256), B, R)
    c = np.array([(80, 70)], np.int32)
    for k in range(B):
        th = 2 * np.pi * k / B
        dx, dy = int(np.rint(reach * np.cos(th))), int(np.rint(reach * np.sin(th)))
        g = np.zeros((H, W), np.float32)
        g[70 + dy, 80 + dx] = 1.0
        assert sr.bins(g, c, dirs, R).tolist() == [k]
        assert eng.orient(g, _kps(c)).tolist() == [k]


@pytest.mark.parametrize("turns", [0, 1, 2, 3])
def test_half_plane_at_full_scale(eng, turns):
    """R = 31, B = 64 and a half plane of 1.0 through the keypoint: the largest |s_k| the rule can produce with make_steering's
    directions, 1.2 * 2^44 against the 2^46 the packed key allows (asserted on the restatement); the bin and the descriptor still come out as restated"""
    rot, dirs = _set(eng, _table(256), 64, 31)
    c = np.array([(80, 70)], np.int32)
    g = fc.half_plane(W, H, 80, 70, turns)
    s = sr.scores(g, c, dirs, 31)[0]
    assert 2 ** 44 < int(np.abs(s).max()) < 2 ** 46
    _check_list(eng, g, c, rot, dirs, 31)
    assert eng.orient(g, _kps(c)).tolist() == [int(s.argmax())]


def test_orient_of_keypoints_outside_the_image(eng, image):
    pts, _ = fc.outside_points(W, H)
    for R, B in [(15, 32), (31, 64)]:
        rot, dirs = _set(eng, _table(256), B, R)
        eb = sr.bins(image, pts, dirs, R)
        assert eng.orient(image, _kps(pts)).tolist() == eb.tolist()
        dx = np.maximum(np.maximum(-pts[:, 0].astype(np.int64), pts[:, 0].astype(np.int64) - (W - 1)), 0)
        dy = np.maximum(np.maximum(-pts[:, 1].astype(np.int64), pts[:, 1].astype(np.int64) - (H - 1)), 0)
        beyond = (dx > R) | (dy > R)                         # no pixel of the disc inside the image: every s_k is 0, bin 0
        assert beyond.sum() >= 6 and (eb[beyond] == 0).all() and len(np.unique(eb[~beyond])) >= 3


def _detect_dev(eng, d_frames, F, w, h, cap, words, steered):
    d_kp = torch.zeros((F, cap, 4), dtype=torch.int32, device=DEV)
    d_desc = torch.zeros((F, cap, words), dtype=torch.int32, device=DEV)
    d_counts = torch.full((F,), -1, dtype=torch.int32, device=DEV)
    d_nraw = torch.full((F,), -1, dtype=torch.int32, device=DEV)
    d_bins = torch.full((F, cap), -1, dtype=torch.int32, device=DEV)
    torch.cuda.synchronize()   # torch's fills run on ITS stream; the engine's non-blocking stream does not order against it
    if steered:
        eng.detect_batch_steered_dev(d_frames, F, w, h, d_kp, d_desc, d_counts, d_nraw, cap, d_bins)
    else:
        eng.detect_batch_dev(d_frames, F, w, h, d_kp, d_desc, d_counts, d_nraw, cap)
    eng.check_status()
    return (d_kp.cpu().numpy(), d_desc.cpu().numpy().view(np.uint32), d_counts.cpu().numpy(), d_nraw.cpu().numpy(),
            d_bins.cpu().numpy())


@pytest.mark.parametrize("F,P", [(3, 256), (9, 256), (3, 100)])
def test_fused_form(eng, F, P):
    w, h, cap, R, B = 320, 200, 2048, 15, 32
    pairs = pg.make_brief_pairs(3, 8, P)
    frames = np.stack([synth.make_frame(w, h, seed=70 + i) for i in range(F)])
    eng.set_detect_params(np.float32(0.1), 4)
    eng.set_capacity(1 << 16, cap)
    words = (P + 31) // 32
    d_frames = torch.from_numpy(frames).to(DEV)
    eng.set_brief_pairs(pairs)
    kp0, desc0, cnt0, nraw0, _ = _detect_dev(eng, d_frames, F, w, h, cap, words, steered=False)
    rot, dirs = _set(eng, pairs, B, R)
    kp1, desc1, cnt1, nraw1, bins1 = _detect_dev(eng, d_frames, F, w, h, cap, words, steered=True)
    kp2, desc2, cnt2, nraw2, bins2 = _detect_dev(eng, d_frames, F, w, h, cap, words, steered=False)   # the plain call, mode on
    assert (cnt0 == cnt1).all() and (cnt0 == cnt2).all() and (nraw0 == nraw1).all() and (nraw0 == nraw2).all()
    assert cnt0.min() >= 30 and cnt0.max() < cap
    assert (bins2 == -1).all()                               # the plain call writes no bins
    differs = 0
    for f in range(F):
        n = int(cnt0[f])
        assert kp1[f, :n].tobytes() == kp0[f, :n].tobytes() == kp2[f, :n].tobytes()     # keypoints and order unchanged
        g = eng.gray(frames[f])
        eb, ed = sr.describe(g, kp0[f, :n, :2], rot, dirs, R)
        assert bins1[f, :n].tolist() == eb.tolist() and (bins1[f, n:] == -1).all()
        assert (desc1[f, :n] == ed).all() and (desc2[f, :n] == ed).all()
        assert (desc0[f, :n] == cref.brief(g, kp0[f, :n, :2], pairs)).all()
        differs += int((desc1[f, :n] != desc0[f, :n]).any(axis=1).sum())
        assert len(np.unique(eb)) >= 8
    assert differs > 0
    kp, desc, nraw = eng.detect(frames[0], capacity=cap)     # the host form shares the launch site
    assert len(kp) == cnt0[0] and (desc == desc1[0, :len(kp)]).all()
    eng.set_brief_steering(None)


def test_switching(eng, image):
    a, b = _table(256, seed=31), _table(256, seed=32)
    xy = _points(W, H, 15)
    rot, dirs = _set(eng, a, 32, 15)
    _, steered_a = _check_list(eng, image, xy, rot, dirs, 15)
    plain_a = cref.brief(image, xy, a)
    assert (steered_a != plain_a).any()
    eng.set_brief_steering(None)                             # NULL restores the plain descriptors bit for bit
    assert (eng.brief(image, _kps(xy)) == plain_a).all()
    with pytest.raises(pg.PgxError) as e:
        eng.orient(image, _kps(xy))
    assert e.value.code == PGX_E_NOT_CONFIGURED
    eng.set_brief_steering(rot, dirs, 15)
    assert (eng.brief(image, _kps(xy)) == steered_a).all()
    eng.set_brief_pairs(b)                                   # a new table turns the mode off: the turned tables were a's
    assert (eng.brief(image, _kps(xy)) == cref.brief(image, xy, b)).all()
    with pytest.raises(pg.PgxError) as e:
        eng.orient(image, _kps(xy))
    assert e.value.code == PGX_E_NOT_CONFIGURED
    rot_b, dirs_b = pg.make_steering(b, 8)                   # a second table (other B, other R) takes effect
    eng.set_brief_steering(rot_b, dirs_b, 7)
    eb, _ = _check_list(eng, image, xy, rot_b, dirs_b, 7)
    assert eb.max() < 8
    eng.set_brief_steering(rot, dirs, 15)                    # and a third over it, without going through off
    eng.set_brief_pairs(a)
    eng.set_brief_steering(rot, dirs, 15)
    assert (eng.brief(image, _kps(xy)) == steered_a).all()
    eng.set_brief_steering(None)


@pytest.mark.parametrize("j", [1, 2, 3])
def test_quarter_turn_on_the_device(eng, j):
    R, B = 15, 32
    g = sr.smooth_image(W, H, 5)
    pairs = np.random.default_rng(12).integers(-12, 13, (256, 4)).astype(np.int32)
    rng = np.random.default_rng(13)
    xy = np.stack([rng.integers(20, W - 20, 60), rng.integers(20, H - 20, 60)], axis=1).astype(np.int32)
    rot, dirs = _set(eng, pairs, B, R)
    case = sr.quarter_turn_case(g, xy, rot, dirs, R, j)
    ok = case["qualifies"]
    assert ok.sum() >= 0.9 * len(xy)                         # the precondition, on the reference first
    assert (case["desc_turned"][ok] == case["desc"][ok]).all()
    d1 = eng.brief(g, _kps(xy))
    d2 = eng.brief(case["turned"], _kps(case["xy_turned"]))
    b1, b2 = eng.orient(g, _kps(xy)), eng.orient(case["turned"], _kps(case["xy_turned"]))
    assert (d1[ok] == d2[ok]).all() and (d1 == case["desc"]).all() and (d2 == case["desc_turned"]).all()
    assert ((b2[ok] - b1[ok] + j * (B // 4)) % B == 0).all()
    eng.set_brief_steering(None)


def test_errors():
    e = pg.Engine(0)
    try:
        pairs = _table(64)
        rot, dirs = pg.make_steering(pairs, 8)
        with pytest.raises(pg.PgxError) as ex:               # steering before any pair table
            e._chk(e._L.pgx_set_brief_steering(e._h, _ptr(rot), _ptr(dirs), 8, 15))
        assert ex.value.code == PGX_E_NOT_CONFIGURED
        e.set_brief_pairs(pairs)
        e.set_detect_params(np.float32(0.1), 4)
        d = torch.zeros(64 * 64 * 4, dtype=torch.int32, device=DEV)
        torch.cuda.synchronize()
        with pytest.raises(pg.PgxError) as ex:               # the steered detect call with the mode off
            e.detect_batch_steered_dev(d, 1, 32, 32, d, d, d, d, 16, d)
        assert ex.value.code == PGX_E_NOT_CONFIGURED
        for B in (0, 6, 68):
            big = np.zeros((max(B, 1), 64, 4), np.int32)
            with pytest.raises(pg.ArgumentException):
                e.set_brief_steering(big, np.zeros((B, 2), np.int32), 15)
        for radius in (0, 32):
            with pytest.raises(pg.ArgumentException):
                e.set_brief_steering(rot, dirs, radius)
        for v in (32768, -32768):
            bad = dirs.copy()
            bad[5, 1] = v
            with pytest.raises(pg.ArgumentException):
                e.set_brief_steering(rot, bad, 15)
        edge = dirs.copy()
        edge[5, 1] = -32767                                  # the limit itself is allowed
        e.set_brief_steering(rot, edge, 31)
        g = sr.smooth_image(40, 40, 6)
        xy = np.array([(20, 20), (0, 39)], np.int32)
        assert e.orient(g, _kps(xy)).tolist() == sr.bins(g, xy, edge, 31).tolist()
    finally:
        e.close()
