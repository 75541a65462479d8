"""CPU tests of the dense stage's yardstick (tests/depth_ref.py), which the GPU tests hold the device to bit for bit: against an
independent loop-per-pixel formulation, against the truth of a rendered scene, and on exact special cases of the rule."""
import functools

import numpy as np
import pytest

import depth_ref as ref
from depth_ref import EDGE

BIG = 10**6


def bits(a):
    return np.ascontiguousarray(a).view(np.uint8).tobytes()


def test_vectorised_equals_loop_per_pixel():
    W, H, D = 24, 16, 5
    C = [(0.0, 0.0, 0.0), (0.25, 0.0, 0.0), (0.0, -0.2, 0.05)]
    gray = np.stack([ref.scene_render(c, 0.3, seed=3, W=W, H=H, f=30.0)[0] for c in C])
    gray[1, 5, 7] = np.nan
    P = np.stack([ref.scene_camera(c, W, H, 30.0).reshape(12) for c in C])
    views = np.array([[0, 1, 2], [2, 0, -1]], dtype=np.int32)
    ranges = [(2.0, 6.0), (2.5, 5.0)]
    a = ref.depth_maps(gray, None, 3, P, views, ranges, D, 1, 2, BIG)
    b = ref.depth_maps_loop(gray, None, 3, P, views, ranges, D, 1, 2, BIG)
    for k in ("kq8", "cost", "flags", "depth"):
        assert bits(a[k]) == bits(b[k]), k
    assert (a["flags"] == 0).any() and (a["flags"] != 0).any()


@functools.lru_cache(maxsize=None)
def solved(slant):
    sc = ref.scene(slant)
    out = ref.depth_maps(sc["gray"], None, 5, sc["P"], ref.all_views(), [sc["range"]] * 5, ref.SCENE_D, 2, 2, BIG)
    return sc, out


@pytest.mark.parametrize("slant", [0.0, 0.3])
def test_reference_at_the_origin_is_within_one_plane_of_the_truth(slant):
    sc, out = solved(slant)
    good = (out["flags"][0] == 0) & (np.abs(out["kq8"][0] / 256.0 - sc["ktrue"][0]) <= 1.0)
    print("slant %.1f: %.4f of the pixels within one plane" % (slant, good.mean()))
    assert good.mean() >= 0.95


@pytest.mark.parametrize("slant", [0.0, 0.3])
def test_cross_view_filter_removes_wrong_pixels(slant):
    sc, out = solved(slant)
    f = ref.fuse(out["depth"], ref.all_views(), 5, sc["P"], 0.05, 2)
    has = np.isfinite(out["depth"])
    wrong = has & ~(np.abs(out["kq8"] / 256.0 - sc["ktrue"]) <= 1.0)
    keep = f["keep"]
    before, after = 1.0 - wrong.sum() / has.sum(), 1.0 - (wrong & keep).sum() / keep.sum()
    print("slant %.1f: kept %.4f, wrong %d -> %d, correct %.4f -> %.4f" % (slant, keep.sum() / has.sum(), wrong.sum(),
                                                                          (wrong & keep).sum(), before, after))
    assert keep.sum() >= 0.90 * has.sum()
    assert 2 * (wrong & keep).sum() <= wrong.sum()
    assert after > before
    assert f["summary"][0] == keep.sum() == len(f["xyz"]) and f["summary"][1] == has.sum() and f["summary"][3] == 0
    # the kept points lie on the maps' depths along their pixels' rays
    r, pix = f["src"][:, 0], f["src"][:, 1]
    C = np.array(ref.SCENE_CENTRES)[r]
    z = out["depth"].reshape(5, -1)[r, pix]
    assert np.abs(f["xyz"][:, 2] - C[:, 2] - z).max() <= 1e-9 * 6.0


def test_constant_image_gives_plane_zero_and_edge():
    sc = ref.scene()
    out = ref.depth_maps(np.full((5, 64, 96), 0.5, np.float32), None, 5, sc["P"], ref.all_views()[:1], [sc["range"]], 8, 1, 1, BIG,
                         volumes=True)
    raw, nval, agg = out["volumes"][0]
    assert (raw == ref.PEN * (4 - nval)).all()          # a valid source costs 0: every census word is 0
    assert (out["flags"] == EDGE).all() or ((out["flags"] & EDGE) != 0).all()
    assert (out["kq8"] == -1).all() and np.isnan(out["depth"]).all()


def test_identical_source_costs_nothing_at_any_plane():
    sc = ref.scene()
    gray = np.stack([sc["gray"][0], sc["gray"][0]])
    P = np.stack([sc["P"][0], sc["P"][0]])
    out = ref.depth_maps(gray, None, 2, P, [[0, 1]], [sc["range"]], 16, 2, 1, BIG, volumes=True)
    raw, nval, agg = out["volumes"][0]
    assert (raw == 0).all() and (nval == 1).all() and (agg == 0).all()
    assert (out["cost"] == 0).all() and (out["flags"] == EDGE).all()


def test_subplane_offsets():
    assert ref.subplane(7, 7, 7) == 0                      # den == 0
    assert ref.subplane(9, 5, 5) == 128                    # n == den
    assert ref.subplane(5, 5, 9) == -128                   # n == -den
    assert ref.subplane(6, 5, 9) == -((3 * 128) // 5)      # negative n truncates towards zero: -76, not -77
    assert ref.subplane(9, 5, 6) == (3 * 128) // 5
    assert (ref.subplane(np.array([9, 5]), np.array([5, 5]), np.array([5, 9])) == [128, -128]).all()
