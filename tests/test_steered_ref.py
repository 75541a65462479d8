"""CPU tests (no GPU) of steered BRIEF's host side: the steering-table generator pgx_make_steering (direction 0, the exact
quarter-turn relation, the rounding bounds, its errors), the int32 bound that makes step 2 of the rule exact in any order,
and -- on the numpy restatement tests/steered_ref.py -- what the mode is for: the steered descriptors of an image and of its
exact quarter turns are bit-identical, where the upright descriptors of the same points differ like those of unrelated points."""
import numpy as np
import pytest

import photogrammetry_amd as pg
import steered_ref as sr

TOL = 0.5 + 1e-9


def _tables():
    neg = np.random.default_rng(11).integers(-40, 41, (100, 4)).astype(np.int32)
    return {"seeded": pg.make_brief_pairs(3, 50, 256), "negative": neg}


@pytest.mark.parametrize("B", [4, 8, 32, 64])
@pytest.mark.parametrize("name", ["seeded", "negative"])
def test_make_steering_properties(B, name):
    pairs = _tables()[name]
    rot, dirs = pg.make_steering(pairs, B)
    P, Q = len(pairs), B // 4
    assert rot.shape == (B, P, 4) and rot.dtype == np.int32 and dirs.shape == (B, 2) and dirs.dtype == np.int32
    assert (rot[0] == pairs).all() and tuple(dirs[0]) == (16384, 0)            # direction 0 is the input
    ends = rot.reshape(B, 2 * P, 2).astype(np.int64)
    for k in range(Q, B):                                                      # the exact quarter turn (x, y) -> (-y, x)
        assert (ends[k, :, 0] == -ends[k - Q, :, 1]).all() and (ends[k, :, 1] == ends[k - Q, :, 0]).all()
        assert dirs[k, 0] == -dirs[k - Q, 1] and dirs[k, 1] == dirs[k - Q, 0]
    src = pairs.reshape(2 * P, 2).astype(np.float64)
    for k in range(B):                                                         # rounding of the float64 rotation
        th = 2 * np.pi * k / B
        c, s = np.cos(th), np.sin(th)
        assert np.abs(ends[k, :, 0] - (c * src[:, 0] - s * src[:, 1])).max() <= TOL
        assert np.abs(ends[k, :, 1] - (s * src[:, 0] + c * src[:, 1])).max() <= TOL
        assert abs(dirs[k, 0] - 16384 * c) <= TOL and abs(dirs[k, 1] - 16384 * s) <= TOL
    assert np.abs(dirs).max() <= 32767


def test_make_steering_errors():
    pairs = _tables()["negative"]
    for B in (0, 2, 6, 68, -4):
        with pytest.raises(pg.ArgumentException):
            pg.make_steering(pairs, B)
    for v in (2**20 + 1, -(2**20) - 1):
        bad = pairs.copy()
        bad[7, 2] = v
        with pytest.raises(pg.ArgumentException):
            pg.make_steering(bad, 8)
    edge = pairs.copy()
    edge[7, 2], edge[8, 1] = 2**20, -(2**20)                                   # the limit itself is allowed
    rot, _ = pg.make_steering(edge, 8)
    assert rot[2, 7, 3] == 2**20 and rot[2, 8, 0] == 2**20                     # direction B / 4: (x, y) -> (-y, x)


def test_moments_stay_inside_int32_and_scores_inside_2_to_46():
    dx, dy = sr.disc(31)
    assert len(dx) == 3001                                                     # the disc of up to 3001 pixels
    pos = int((dx[dx > 0] * 65535).sum())
    assert pos == 1290253080 < 2**31                                           # the positive part of a moment, all pixels at 1.0
    assert int((dy[dy > 0] * 65535).sum()) == pos
    # |s_k| is largest on the half plane a direction points into; the maximum over the box of dirs is at a corner
    for cx, cy in [(32767, 32767), (32767, -32767), (32767, 0), (0, 32767)]:
        t = cx * dx + cy * dy
        assert int(t[t > 0].sum()) * 65535 < 2**46


@pytest.fixture(scope="module")
def turn_setup():
    W, H, R, B = 161, 140, 15, 32
    g = sr.smooth_image(W, H, 5)
    pairs = np.random.default_rng(12).integers(-12, 13, (256, 4)).astype(np.int32)
    rot, dirs = pg.make_steering(pairs, B)
    rng = np.random.default_rng(13)
    xy = np.stack([rng.integers(20, W - 20, 60), rng.integers(20, H - 20, 60)], axis=1).astype(np.int32)
    return g, xy, pairs, rot, dirs, R, B


@pytest.mark.parametrize("j", [1, 2, 3])
def test_quarter_turns_leave_the_steered_descriptor_unchanged(turn_setup, j):
    g, xy, pairs, rot, dirs, R, B = turn_setup
    case = sr.quarter_turn_case(g, xy, rot, dirs, R, j)
    ok = case["qualifies"]
    assert ok.sum() >= 0.9 * len(xy), int(ok.sum())
    # np.rot90 takes the offset (dx, dy) to (dy, -dx), the inverse of the table's quarter turn: the bin moves back by B / 4
    # per turn, and the table of the new bin samples the same physical pixels
    assert ((case["bins_turned"][ok] - case["bins"][ok] + j * (B // 4)) % B == 0).all()
    assert (case["desc_turned"][ok] == case["desc"][ok]).all()
    assert len(np.unique(case["bins"])) >= 4                                   # the points do not all look one way
    # the same points under the upright table: as far apart as unrelated points
    from oracle import cref
    plain = sr.hamming(cref.brief(g, xy[ok], pairs), cref.brief(case["turned"], case["xy_turned"][ok], pairs))
    assert plain.mean() > 64, plain.mean()


def test_reference_quantisation_and_tie_rule():
    g = np.array([[np.nan, -1.0, 2.0], [np.inf, -np.inf, 1.0], [1e-40, 0.5 / 65535, 1.5 / 65535]], np.float32)
    q = sr.quantise(g)
    assert q.tolist() == [[0, 0, 65535], [65535, 0, 65535], [0, int(np.rint(np.float32(0.5 / 65535) * np.float32(65535))),
                                                             int(np.rint(np.float32(1.5 / 65535) * np.float32(65535)))]]
    flat = np.full((9, 9), 0.25, np.float32)
    _, dirs = pg.make_steering(np.zeros((1, 4), np.int32), 8)
    assert sr.bins(np.pad(flat, 8, constant_values=0.25), [(12, 12)], dirs, 4).tolist() == [0]   # m10 = m01 = 0: every s_k is 0
