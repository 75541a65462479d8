"""BRIEF-256 on the row-sorted sample plan (brief_256 in csrc/k_brief.hip, plan: csrc/pgx_brief_plan.h) against the oracle, bit
for bit, through both kernels that use it: Engine.brief (k_brief_list, explicit keypoints) and Engine.detect (k_brief_kept,
the detect chain's survivors).  Small images on purpose: the plan's gathers are 64 sorted samples each, and what can break is
which of them fall outside the image, where equal values and equal points land, and whether the plan follows the table."""
import numpy as np
import pytest

import photogrammetry_amd as pg
from oracle import cref

pytestmark = pytest.mark.gpu
W, H = 96, 80
T, RADIUS = np.float32(0.05), 2


@pytest.fixture(scope="module")
def eng():
    e = pg.Engine(0)          # a context of its own: no dewarp map, and the tables set here stay out of the shared one
    e.set_detect_params(T, RADIUS)
    yield e
    e.close()


def _frame(w, h, seed, levels=None):
    """RGBA64 frame and its f32 grey image (the oracle's conversion; the chain's own is checked in test_gpu_parity)."""
    rng = np.random.default_rng(seed)
    if levels is None:
        f = rng.integers(0, 65536, (h, w, 4)).astype(np.uint16)
    else:
        lv = np.asarray(levels, np.uint16)[rng.integers(0, len(levels), (h, w))]
        f = np.repeat(lv[..., None], 4, axis=2)
    f[..., 3] = 65535
    f = np.ascontiguousarray(f)
    return f, cref.gray(f)


def _kps(xy):
    k = np.zeros(len(xy), dtype=pg.KEYPOINT_DTYPE)
    k["x"], k["y"] = np.asarray(xy)[:, 0], np.asarray(xy)[:, 1]
    return k


def _border_points(w, h):
    xs = sorted({0, 1, w // 2, w - 2, w - 1})
    ys = sorted({0, 1, h // 2, h - 2, h - 1})
    pts = [(x, y) for x in xs for y in (0, h - 1)] + [(x, y) for y in ys for x in (0, w - 1)]
    cx, cy = w - 1 - 50, h - 1 - 50           # a 0..50 window touches the right / bottom edge exactly here
    pts += [(max(0, cx + dx), max(0, cy + dy)) for dx in (-1, 0, 1) for dy in (-1, 0, 1)]
    return np.array(sorted(set(pts)), np.int32)


def _check_list(eng, g, xy, pairs):
    got = eng.brief(g, _kps(xy))
    exp = cref.brief(g, xy, pairs)
    assert got.shape == exp.shape and (got == exp).all()
    return exp


def _check_chain(eng, frame, g, pairs, at_least):
    kp, desc, nraw = eng.detect(frame, capacity=8192)
    raw = cref.detect(g, T)
    kept = raw[cref.nms(raw, RADIUS)]
    assert nraw == len(raw) and len(kp) == len(kept) >= at_least
    assert (kp["x"] == kept["x"]).all() and (kp["y"] == kept["y"]).all()
    exp = cref.brief(g, np.stack([kept["x"], kept["y"]], 1), pairs)
    assert (desc == exp).all()
    return kept, exp


def _window50():
    """Offsets in [0, 50], the reach the border cases are built around (make_brief_pairs's own go to about 200)."""
    return np.random.default_rng(50).integers(0, 51, (256, 4)).astype(np.int32)


@pytest.mark.parametrize("table", ["window50", "seed0", "seed7"])
def test_border_keypoints(eng, table):
    pairs = _window50() if table == "window50" else pg.make_brief_pairs(int(table[4:]), 50, 256)
    eng.set_brief_pairs(pairs)
    frame, g = _frame(W, H, 1)
    xy = _border_points(W, H)
    exp = _check_list(eng, g, xy, pairs)
    if table == "window50":
        # the cases are what they claim: at (W-51, H-51) every sample is inside, one pixel on some are not, at (W-1, H-1) a
        # pair survives only with both end points at offset (0, 0)
        inside = {(int(x), int(y)): bool(((x + pairs[:, [0, 2]] < W) & (y + pairs[:, [1, 3]] < H)).all()) for x, y in xy}
        assert inside[(W - 51, H - 51)] and inside[(W - 52, H - 52)] and not inside[(W - 50, H - 51)] and not inside[(W - 51, H - 50)]
        assert (exp[[tuple(p) == (W - 1, H - 1) for p in xy.tolist()]] == 0).all()
    kept, _ = _check_chain(eng, frame, g, pairs, at_least=50)
    assert (kept["x"] >= W - 8).any() and (kept["y"] >= H - 8).any() and (kept["x"] <= 8).any() and (kept["y"] <= 8).any()


def test_image_smaller_than_the_window(eng):
    pairs = _window50()
    eng.set_brief_pairs(pairs)
    frame, g = _frame(40, 30, 2)
    xy = np.array([(x, y) for x in (0, 1, 17, 38, 39) for y in (0, 1, 13, 28, 29)], np.int32)
    assert all(((x + pairs[:, [0, 2]] >= 40) | (y + pairs[:, [1, 3]] >= 30)).any() for x, y in xy)   # out-of-bounds samples everywhere
    _check_list(eng, g, xy, pairs)
    _check_chain(eng, frame, g, pairs, at_least=10)


def _awkward_tables():
    rng = np.random.default_rng(3)
    neg = rng.integers(-25, 26, (256, 4)).astype(np.int32)
    rep = neg.copy()
    rep[:, 2:] = rep[rng.integers(0, 8, 256), :2]                  # eight sample points shared by all second end points
    same = neg.copy()
    same[::2, 2:] = same[::2, :2]                                  # every other pair: identical end points -> bit 0
    one = np.tile(np.array([[-3, 2, 4, -1]], np.int32), (256, 1))  # all 256 pairs identical
    far = neg.copy()
    far[:, 0] += 1000                                              # first end point beyond the image: every bit 0
    far[::3, 3] -= 100000
    huge = neg.copy()
    huge[::4, 0] = np.iinfo(np.int32).max - 200                    # stays inside int32 when a coordinate < 200 is added
    huge[1::4, 3] = np.iinfo(np.int32).min + 200
    return {"negative": neg, "repeated_points": rep, "identical_end_points": same, "all_pairs_identical": one,
            "beyond_the_image": far, "huge": huge}


@pytest.mark.parametrize("name", ["negative", "repeated_points", "identical_end_points", "all_pairs_identical",
                                  "beyond_the_image", "huge"])
def test_awkward_tables(eng, name):
    pairs = _awkward_tables()[name]
    eng.set_brief_pairs(pairs)
    frame, g = _frame(W, H, 4)
    xy = np.concatenate([_border_points(W, H), np.random.default_rng(5).integers(0, [W, H], (24, 2)).astype(np.int32)])
    exp = _check_list(eng, g, xy, pairs)
    _, exp_chain = _check_chain(eng, frame, g, pairs, at_least=50)
    if name == "beyond_the_image":
        assert (exp == 0).all() and (exp_chain == 0).all()
    if name == "identical_end_points":        # pair p is bit 255 - p: the even pairs are the odd bits of every word
        assert (exp & 0xAAAAAAAA == 0).all() and (exp & 0x55555555 != 0).any()
    if name == "all_pairs_identical":
        assert set(np.unique(exp).tolist()) == {0, 0xFFFFFFFF}


@pytest.mark.parametrize("levels", [[30000], [20000, 40000]])
def test_equal_grey_values_stay_strictly_less(eng, levels):
    pairs = np.random.default_rng(6).integers(-25, 26, (256, 4)).astype(np.int32)
    eng.set_brief_pairs(pairs)
    frame, g = _frame(W, H, 7, levels=levels)
    assert len(np.unique(g)) == len(levels)
    xy = np.concatenate([_border_points(W, H), np.array([(W // 2, H // 2), (30, 30)], np.int32)])
    exp = _check_list(eng, g, xy, pairs)
    if len(levels) == 1:
        assert (exp == 0).all()                # v < v is false everywhere
        kp, desc, nraw = eng.detect(frame, capacity=64)
        assert nraw == 0 and len(kp) == 0      # nothing to detect on a constant image: the chain runs with an empty list
    else:
        _, exp_chain = _check_chain(eng, frame, g, pairs, at_least=10)   # two-level noise has few FAST arcs
        assert exp_chain.any()


def test_plan_follows_the_table_and_generic_path_is_unaffected(eng):
    a = pg.make_brief_pairs(0, 50, 256)
    b = np.random.default_rng(8).integers(-25, 26, (256, 4)).astype(np.int32)
    c = cref.gaussian_pairs(5, 10, 200)        # P != 256: the generic path, which has no plan
    frame, g = _frame(W, H, 9)
    xy = np.concatenate([_border_points(W, H), np.random.default_rng(10).integers(0, [W, H], (16, 2)).astype(np.int32)])
    seen = []
    for pairs in (a, b, a, c, b, c, a):
        eng.set_brief_pairs(pairs)
        seen.append(_check_list(eng, g, xy, pairs))
        _check_chain(eng, frame, g, pairs, at_least=50)
    assert (seen[0] == seen[2]).all() and (seen[0] == seen[6]).all() and (seen[1] == seen[4]).all()
    assert (seen[0] != seen[1]).any() and seen[3].shape[1] == 7
