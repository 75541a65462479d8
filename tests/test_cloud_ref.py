"""CPU tests of the cloud merge's yardstick (tests/cloud_ref.py), which the GPU tests hold the device to bit for bit: the vectorised
form against the loop-per-point restatement, exact invariants of the rule, the normals against the truth of the rendered scene at
the true and at the estimated depths, and the PLY writer against its reader.  Conditions on the yardstick alone."""
import functools

import numpy as np
import pytest

import cloud_ref as ref
import depth_ref
from photogrammetry_amd import cloud

BIG = 10**6
CELL, ORIGIN = ref.CELL, ref.ORIGIN
TRUTH = (0.0, 0.0, -1.0)          # both planes of the scene face the cameras along -z


def run_both(c, **kw):
    args = (c["xyz"], c["src"], c["depth"], c["views"], len(c["P"]), c["P"], CELL, ORIGIN)
    kw = dict(dict(k=1, disc_tol=0.02, min_support=1, rgba8=c["rgba8"], frame_ids=c["frame_ids"]), **kw)
    return ref.merge(*args, **kw), ref.merge_loop(*args, **kw)


@pytest.mark.parametrize("kw", [dict(), dict(k=2, min_support=2), dict(disc_tol=0.0, rgba8=None, frame_ids=None), dict(count=57),
                                dict(count=10**6), dict(count=-3)])
def test_vectorised_equals_loop_per_point(kw):
    a, b = run_both(ref.boundary_case(), **kw)
    ref.assert_same(a, b)
    if not kw:
        rep = a["report"]
        print("report", rep)
        assert rep[2] >= 7 + 9 and rep[3] > 0 and rep[3] < rep[1] and 0 < rep[4] < rep[1] and rep[6] == rep[5] < rep[1]
        assert (a["cnt"] >= 2).any() and (a["nn"] == 0).any() and (a["nc"] == 0).any()


def test_exact_invariants():
    c = ref.boundary_case()
    a, _ = run_both(c)
    used = a["used"]
    assert a["cnt"].sum() == used.sum() == a["report"][1]
    # every used point lies in the box of its cell, and so does the output position
    o = np.array(ORIGIN)
    X, g = c["xyz"][used], a["g"][used]
    assert (X >= o + g * CELL).all() and (X < o + (g + 1) * CELL).all()
    assert (a["p"][used] >= 0).all() and (a["p"][used] <= 65535).all()
    gk = np.stack([(a["keys"] >> 42) & 0x1FFFFF, (a["keys"] >> 21) & 0x1FFFFF, a["keys"] & 0x1FFFFF], 1) - ref.GB
    assert (a["xyz"] >= o + gk * CELL).all() and (a["xyz"] <= o + (gk + 1) * CELL).all()
    # cell a power of two: origin and points moved by integer multiples of the cell change no integer output
    shift = np.array([3, -5, 17]) * CELL
    moved = ref.merge(c["xyz"] + shift, c["src"], c["depth"], c["views"], 4, c["P"], CELL, o + shift, rgba8=c["rgba8"], frame_ids=c["frame_ids"])
    ref.assert_same(moved, a, ref.INT_KEYS)
    assert ref.bits(moved["normal"]) == ref.bits(a["normal"])
    # a permuted list: the same cells and sums
    perm = np.random.default_rng(9).permutation(len(c["xyz"]))
    b = ref.merge(c["xyz"][perm], c["src"][perm], c["depth"], c["views"], 4, c["P"], CELL, ORIGIN, rgba8=c["rgba8"], frame_ids=c["frame_ids"])
    for k, x in ref.by_key(a).items():
        assert (x == ref.by_key(b)[k]).all(), k
    # ... in the order of their new first: the smallest new position of a cell's points
    inv = np.argsort(perm)
    want = np.full(len(a["keys"]), len(perm))
    np.minimum.at(want, a["cell_of"][used], inv[np.flatnonzero(used)])
    assert (np.diff(b["first"]) > 0).all()
    assert (b["first"][np.argsort(b["keys"])] == want[np.argsort(a["keys"])]).all()


@functools.lru_cache(maxsize=None)
def rotated_truth():
    sc = depth_ref.scene_rotated()
    f = depth_ref.fuse(sc["ztrue"], depth_ref.all_views(), 5, sc["P"], 0.05, 1)
    return sc, f


def test_sign_and_power_of_two_scales_change_no_integer():
    sc, f = rotated_truth()
    base = ref.merge(f["xyz"], f["src"], sc["ztrue"], depth_ref.all_views(), 5, sc["P"], CELL, ORIGIN)
    for P in (-sc["P"], depth_ref.scaled_cameras(sc["P"], depth_ref.ROT_SCALES_POW2)):
        other = ref.merge(f["xyz"], f["src"], sc["ztrue"], depth_ref.all_views(), 5, P, CELL, ORIGIN)
        ref.assert_same(other, base)


def test_truth_normals_at_the_true_depths():
    """scene_rotated() at its true depths, the filter at 0.05 / 1, cells of 1 / 32 at (-8, -8, -8), k = 1, disc_tol 0.02: every
    normal within 1e-4 rad of (0, 0, -1) (the quantisation to 1 / 32767 allows 2.7e-5), at most 4 points without one, fewer cells
    than points; without the gate the rectangle's edge gets normals more than 0.2 rad off."""
    sc, f = rotated_truth()
    assert len(f["xyz"]) == 29364
    m = ref.merge(f["xyz"], f["src"], sc["ztrue"], depth_ref.all_views(), 5, sc["P"], CELL, ORIGIN, k=1, disc_tol=0.02)
    has = m["has_normal"]
    pa = ref.angle_to(m["pt_normal"][has], TRUTH)
    ca = ref.angle_to(m["normal"][m["info"][:, 1] > 0], TRUTH)
    cells, seen2 = int(m["report"][5]), int((m["cnt"] >= 2).sum())
    print("points %d, without a normal %d, cells %d, cells with support >= 2 %d, worst angle %.3g (points) %.3g (cells)"
          % (len(has), (~has).sum(), cells, seen2, pa.max(), ca.max()))
    assert pa.max() <= 1e-4 and ca.max() <= 1e-4
    assert (~has).sum() <= 4
    assert cells < len(has) and seen2 > cells // 2
    assert (m["info"][:, 1] == 0).sum() <= (~has).sum()
    loose = ref.merge(f["xyz"], f["src"], sc["ztrue"], depth_ref.all_views(), 5, sc["P"], CELL, ORIGIN, k=1, disc_tol=1e9)
    la = ref.angle_to(loose["pt_normal"][loose["has_normal"]], TRUTH)
    print("without the gate: %d normals more than 0.2 rad off, worst %.3f" % ((la > 0.2).sum(), la.max()))
    assert (la > 0.2).sum() > 0


# ---- estimated depths -----------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def estimated(case):
    if case == "plain":
        sc = depth_ref.scene(0.0)
    else:
        sc = depth_ref.scene_rotated()
    out = depth_ref.depth_maps(sc["gray"], None, 5, sc["P"], depth_ref.all_views(), [sc["range"]] * 5, depth_ref.SCENE_D, 2, 2, BIG)
    f = depth_ref.fuse(out["depth"], depth_ref.all_views(), 5, sc["P"], 0.05, 2)
    return sc, out, f


def fractions(case, k):
    sc, out, f = estimated(case)
    m = ref.merge(f["xyz"], f["src"], out["depth"], depth_ref.all_views(), 5, sc["P"], CELL, ORIGIN, k=k, disc_tol=0.02)
    lim = np.radians(20.0)
    pts = (ref.angle_to(m["pt_normal"][m["has_normal"]], TRUTH) <= lim).mean()
    sel = (m["info"][:, 0] >= 3) & (m["info"][:, 1] > 0)
    cells = (ref.angle_to(m["normal"][sel], TRUTH) <= lim).mean()
    return float(pts), float(cells)


@pytest.mark.parametrize("case", ["plain", "rotated"])
def test_normals_at_the_estimated_depths(case):
    got = {k: fractions(case, k) for k in (1, 3)}
    for k in (1, 3):
        print("%s k = %d: %.4f of the points with a normal, %.4f of the cells with support >= 3 within 20 degrees" % ((case, k) + got[k]))
    for k in (1, 3):
        assert got[k][0] >= ref.FLOORS[(case, k)][0] and got[k][1] >= ref.FLOORS[(case, k)][1]
        assert got[k][1] > got[k][0]                  # cells with support >= 3 are better than points
    assert got[3][0] > got[1][0] and got[3][1] > got[1][1]   # k = 3 is better than k = 1


# ---- write_ply -------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("with_normal,with_colour", [(True, True), (True, False), (False, True), (False, False)])
def test_write_ply_round_trips_every_bit(tmp_path, with_normal, with_colour):
    rng = np.random.default_rng(4)
    n = 37
    xyz = rng.standard_normal((n, 3))
    xyz[0] = [np.nan, -0.0, np.inf]
    xyz[1] = np.nextafter(1.0, 2.0)
    normal = rng.standard_normal((n, 3)).astype(np.float32) if with_normal else None
    rgba8 = rng.integers(0, 2**32, n, dtype=np.uint32) if with_colour else None
    path = str(tmp_path / "cloud.ply")
    cloud.write_ply(path, xyz, normal, rgba8)
    head = open(path, "rb").read(64)
    assert head.startswith(b"ply\nformat binary_little_endian 1.0\nelement vertex 37\n")
    x2, n2, c2 = cloud.read_ply(path)
    assert ref.bits(x2) == ref.bits(xyz) and x2.dtype == np.float64
    assert (n2 is None) == (normal is None) and (c2 is None) == (rgba8 is None)
    if with_normal:
        assert ref.bits(n2) == ref.bits(normal) and n2.dtype == np.float32
    if with_colour:
        assert (c2 == rgba8).all() and c2.dtype == np.uint32
    cloud.write_ply(path, np.zeros((0, 3)), None, None)
    assert cloud.read_ply(path)[0].shape == (0, 3)
