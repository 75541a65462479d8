"""CPU tests of the yardstick of the dense stage's plan (tests/dense_views_ref.py), which the GPU tests hold the device to bit
for bit: its two restatements against each other, the invariances the rule promises, the plan of the two-plane scenes of
depth_ref.py against their truth, and a camera arc with planted bad neighbours."""
import functools

import numpy as np
import pytest

import dense_views_ref as ref
import depth_ref
import triangulate_ref

BIG = 10**6
GROW = 1.1
# The fraction of the origin reference's pixels that are unflagged and within one plane of the truth when the sweep runs over
# the PLANNED sources and ranges (S = 4, quantiles 0 / 1000, grow 1.1), one plane being a plane of the planned range.  Measured:
# 0.9924 on scene() (planned range (3 / 1.1, 4 * 1.1) for every frame), which is the figure of test_depth_ref.py's hand-configured
# call over (2, 6): the pixels lost are those at the occluding edge either way.  0.9450 on the rotated rig (hand-configured:
# 0.9645 over planes about 2.1 times coarser in 1/z).  The whole computation is deterministic and the device is held to it bit for
# bit, so the margin has to cover only another libm or numpy rounding the rendered textures differently, which moves single
# pixels of 6144: the floors are the figures less 0.01 (61 pixels), rounded down to 0.01.  A plan with one source fewer
# measures 0.8831 and 0.9285, one with two fewer 0.6071 and 0.8462.
PLANNED_FLOOR = 0.98
PLANNED_FLOOR_ROTATED = 0.93


def test_restatements_agree():
    off, nd, xyz, flags, P = ref.mixed_graph()
    for refs, S, kw in ((None, 3, {}), ([4, 0, 6, 4, 11, -1], 8, dict(min_shared=1, min_points=1, q_near_pm=0, q_far_pm=1000)),
                        ([2], 1, dict(min_angle_deg=0.0, max_angle_deg=20.0))):
        a = ref.plan(off, nd, xyz, flags, P, refs, S, **kw)
        b = ref.plan_loop(off, nd, xyz, flags, P, refs, S, **kw)
        ref.assert_equal(a, b)
        assert a["status"] == b["status"] == set()
    a = ref.plan(off, nd, xyz, flags, P, None, 3)
    assert (a["ref_stats"][6] == [0, 0, 0, ref.NOCAMERA]).all() and (a["views"][6, 1:] == -1).all()
    assert (a["views"][:, 1:] != 6).all() and a["report"][1] < 160 and a["report"][3] > 0
    assert np.isfinite(a["range"][[0, 3]]).all()    # the negated camera has a range like any other
    # the capacity and a node outside the frames
    nd2 = nd.copy()
    nd2[off[20], 0] = 9
    c, d = (f(off, nd2, xyz, None, P, None, 2, max_tracks=100) for f in (ref.plan, ref.plan_loop))
    ref.assert_equal(c, d)
    assert c["status"] == d["status"] == {"cap", "node"} and c["report"][0] == 100


def test_translation_decides_the_same_way():
    off, nd, xyz, flags, P = ref.mixed_graph()
    t = np.array([2e4, -1e4, 3e4])
    Pt = P.reshape(-1, 3, 4).copy()
    Pt[:, :, 3] -= Pt[:, :, :3] @ t
    a = ref.plan(off, nd, xyz, flags, P, None, 3)
    b = ref.plan(off, nd, xyz + t, flags, Pt.reshape(-1, 12), None, 3)
    ref.assert_equal(a, b, keys=("views", "pair_counts", "ref_stats", "report"))
    assert np.allclose(a["range"], b["range"], rtol=1e-9, equal_nan=True)


def test_negated_cameras_give_the_same_rows():
    off, nd, xyz, flags, P = ref.mixed_graph()
    ref.assert_equal(ref.plan(off, nd, xyz, flags, P, None, 3), ref.plan(off, nd, xyz, flags, -P, None, 3))


PLAN = dict(q_near_pm=0, q_far_pm=1000, grow=GROW)


@functools.lru_cache(maxsize=None)
def planned(rotated, triangulated=False):
    """the scene, its sparse model and its plan -> (sc, plan, maps of the sweep over the planned views and ranges).
    triangulated: the points are not the rendered ones but triangulate_ref's from the nodes' integer keypoints, which is what
    the chain of tests/test_gpu_dense_views.py plans from"""
    if rotated:
        sc = depth_ref.scene_rotated()
        X = sc["X"]
    else:
        sc = depth_ref.scene()
        X = ref.scene_points(sc, depth_ref.SCENE_CENTRES, depth_ref.SCENE_W, depth_ref.SCENE_H, depth_ref.SCENE_F)
    off, nd, xyz, kps = ref.sparse_from_scene(sc, X)
    flags = None
    if triangulated:
        t = triangulate_ref.triangulate(kps, sc["P"], off, nd, 1.0, float("inf"), 10)
        xyz, flags = t["xyz"], t["flags"]
    pl = ref.plan(off, nd, xyz, flags, sc["P"], None, 4, **PLAN)
    out = depth_ref.depth_maps(sc["gray"], None, 5, sc["P"], pl["views"], pl["range"], depth_ref.SCENE_D, 2, 2, BIG)
    return sc, pl, out


def planned_fractions(sc, pl, out):
    ktrue = np.stack([ref.planes_of(sc["ztrue"][r], pl["range"][r, 0], pl["range"][r, 1], depth_ref.SCENE_D) for r in range(5)])
    return depth_ref.within_one_plane(out["kq8"], out["flags"], ktrue)


@pytest.mark.parametrize("rotated", [False, True])
def test_planned_range_contains_the_truth(rotated):
    sc, pl, _ = planned(rotated)
    assert (pl["ref_stats"][:, 3] == 0).all() and (pl["ref_stats"][:, 2] == 4).all() and (np.sort(pl["views"], 1) == np.arange(5)).all()
    z = sc["ztrue"].reshape(5, -1)
    assert (pl["range"][:, 0] <= z.min(1)).all() and (z.max(1) <= pl["range"][:, 1]).all(), (pl["range"], z.min(1), z.max(1))
    assert (pl["range"][:, 0] > 2.0).all() and (pl["range"][:, 1] < 6.0).all()      # and is tighter than the hand-set (2, 6)


@pytest.mark.parametrize("rotated", [False, True])
def test_sweep_over_the_plan_against_the_truth(rotated):
    sc, pl, out = planned(rotated)
    frac = planned_fractions(sc, pl, out)
    print("planned, within one plane, per reference: " + ", ".join("%.4f" % f for f in frac))
    assert frac[0] >= (PLANNED_FLOOR_ROTATED if rotated else PLANNED_FLOOR)


def test_sweep_over_the_plan_from_triangulated_points():
    """scene() planned from points triangulated out of the nodes' integer keypoints.  The scene's disparities are whole pixels
    (120 * 0.6 / 4 = 18 and 120 * 0.6 / 3 = 24), so the keypoints are exact and the triangulated depths are the rendered ones
    to rounding: the range rounds to the same (2.7273, 4.4) and the figure is the same 0.9924."""
    sc, pl, out = planned(False, True)
    frac = planned_fractions(sc, pl, out)
    print("planned from triangulated points: range", pl["range"][0], "within one plane:", ", ".join("%.4f" % f for f in frac))
    z = sc["ztrue"].reshape(5, -1)
    assert (pl["range"][:, 0] <= z.min(1)).all() and (z.max(1) <= pl["range"][:, 1]).all()
    assert frac[0] >= PLANNED_FLOOR


def test_camera_arc_passes_over_planted_neighbours():
    """Reference at 0 degrees on an arc around the points; neighbours at 0.5 degrees (too narrow for min_angle_deg = 2) and at
    70 degrees (too wide for 45) see every point, four good ones at 8 .. 25 degrees see four in five: the planted two share
    the most points and are chosen last, so with S = 4 not at all, and with S = 6 behind the good ones."""
    rng = np.random.default_rng(3)
    ang = [0.0, 0.5, 70.0, 8.0, -12.0, 18.0, -25.0]
    P = ref.arc_cameras(ang, radius=8.0)
    n = 200
    xyz = 0.3 * rng.standard_normal((n, 3))
    tracks = [[0, 1, 2] + [f for f in (3, 4, 5, 6) if rng.random() < 0.8] for _ in range(n)]
    off = np.concatenate([[0], np.cumsum([len(t) for t in tracks])]).astype(np.int32)
    nd = np.array([(f, i) for i, t in enumerate(tracks) for f in t], dtype=np.int32)
    a = ref.plan(off, nd, xyz, None, P, [0], 4)
    assert sorted(a["views"][0, 1:]) == [3, 4, 5, 6] and a["ref_stats"][0].tolist()[1:] == [6, 4, 0]
    pc = a["pair_counts"][0]
    assert pc[1].tolist() == [n, 0] and pc[2].tolist() == [n, 0] and (pc[3:, 1] == pc[3:, 0]).all() and (pc[3:, 0] < n).all()
    b = ref.plan(off, nd, xyz, None, P, [0], 6)
    assert sorted(b["views"][0, 1:5]) == [3, 4, 5, 6] and b["views"][0, 5:].tolist() == [1, 2]
    ref.assert_equal(a, ref.plan_loop(off, nd, xyz, None, P, [0], 4))
