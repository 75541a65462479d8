"""CPU test (no GPU): tests/init_pair_ref.py -- the yardstick of the initial-pair stage -- against the truth of synthetic
scenes.  The inputs are what the stage is meant to get: the F and the verified list of tests/verify_ref.py (itself tied to the
truth by tests/test_verify_ref.py), the scene's intrinsics.

Bounds.  On true two-view geometry exactly one of the four decompositions puts a true match in front of both cameras, so the
winner holds every verified match; the prototype of the stage saw front = n on all the cases below, sigma_2 / sigma_1 >= 0.988,
a rotation error <= 0.44 degrees and a translation-direction error <= 2.3 degrees (the 8-point fit's own limit on keypoints
rounded to integers).  The tests hold the errors to those figures plus a margin of a third: 0.6 and 3.0 degrees, and the
singular values to 0.98."""
import numpy as np
import pytest

import init_pair_ref as ref
import verify_ref
from init_pair_ref import VER

ROT_DEG, DIR_DEG, SIGMA = 0.6, 3.0, 0.98


def verified(kpa, kpb, ca, cb, ml, a, b, stride):
    return verify_ref.verify_pair(kpa, kpb, ca, cb, ml, a, b, stride, VER["max_dist"], VER["n_samples"], VER["inlier_px"],
                                  VER["min_inliers"], VER["refit_iters"], VER["seed"])


@pytest.mark.parametrize("seed", [0, 3, 5])
@pytest.mark.parametrize("frames", [(1, 3), (2, 3), (0, 5)])
def test_one_candidate_holds_every_inlier_and_is_the_true_pose(seed, frames):
    c = verify_ref.scene_pair(seed, 300, 100, frames=frames)
    a, b, K = c["a"], c["b"], c["scene"]["K"]
    y = verified(c["kps"][a], c["kps"][b], c["counts"][a], c["counts"][b], c["ml"], a, b, c["stride"])
    assert y["stats"][4] == 0 and y["stats"][2] >= 296
    r = ref.relative_pose(c["kps"][a], c["kps"][b], c["counts"][a], c["counts"][b], y["out"], c["stride"], VER["max_dist"], y["F"],
                          K[a], K[b], 2.0, 0.7, 30)
    st = r["stats"]
    rot, direction = ref.pose_errors(r["Rt"], c["R"], c["t"])
    print("seed", seed, "frames", frames, "stats", st.tolist(), "sigma", r["sigma"], "rotation", rot, "direction", direction)
    assert st[0] == y["stats"][2] and st[7] == 0
    assert st[1 + st[6]] == st[0] and sorted(st[1:5])[:3] == [0, 0, 0]      # every inlier in front of one candidate, none of another
    assert st[5] == st[0]                                                   # 24 and 36 degrees of arc: all wide at 2 degrees
    assert r["sigma"] >= SIGMA
    assert rot <= ROT_DEG and direction <= DIR_DEG
    R = r["cand_Rt"][:, :9].reshape(4, 3, 3)
    assert np.abs(R @ R.transpose(0, 2, 1) - np.eye(3)).max() <= 1e-12 and np.abs(np.linalg.det(R) - 1.0).max() <= 1e-12
    assert np.abs(np.linalg.norm(r["cand_Rt"][:, 9:], axis=1) - 1.0).max() <= 1e-12


def test_the_essential_matrix_is_zero_on_the_bearings():
    c = verify_ref.scene_pair(0, 300, 0)
    a, b, K = c["a"], c["b"], c["scene"]["K"]
    y = verified(c["kps"][a], c["kps"][b], c["counts"][a], c["counts"][b], c["ml"], a, b, c["stride"])
    Gh = ref.essential(y["F"], K[a], K[b])
    e, pa, pb, _ = ref.candidates(c["kps"][a], c["kps"][b], c["counts"][a], c["counts"][b], y["out"], c["stride"], VER["max_dist"])
    ga, _ = ref.bearings(pa, K[a])
    gb, _ = ref.bearings(pb, K[b])
    r = np.abs(((gb @ Gh) * ga).sum(1)) / (np.linalg.norm(ga, axis=1) * np.linalg.norm(gb, axis=1))
    assert abs(np.sqrt((Gh * Gh).sum()) - 1.0) <= 1e-15 and r.max() <= 2e-3, r.max()     # 1.5 px at f = 1200 is 1.25e-3
    # and G is [t]x R of the truth, up to scale and sign
    Gt = np.cross(np.eye(3), c["t"]).T @ c["R"]          # [t]x R
    Gt = Gt / np.linalg.norm(Gt)
    assert min(np.abs(Gh - Gt).max(), np.abs(Gh + Gt).max()) <= 0.02


def test_score_signs_and_intrinsics_of_either_sign():
    """the same rays through K and through K with fy < 0 (v mirrored): the same front and wide decisions"""
    c = verify_ref.scene_pair(3, 300, 0)
    a, b = c["a"], c["b"]
    K = c["scene"]["K"][a]
    Km = K * [1, -1, 1, 1]
    e, pa, pb, _ = ref.candidates(c["kps"][a], c["kps"][b], c["counts"][a], c["counts"][b], c["ml"], c["stride"], VER["max_dist"])
    pam = np.stack([pa[:, 0], 2 * K[3] - pa[:, 1]], 1)           # v - cy changes sign, so (v - cy) / fy does not
    truth = np.r_[c["R"].reshape(9), c["t"] / np.linalg.norm(c["t"])]
    gb, sb = ref.bearings(pb, K)
    for p, k in ((pa, K), (pam, Km)):
        ga, sa = ref.bearings(p, k)
        f, w = ref.score(truth, ga, gb, sa, sb, ref.cos2_of(10.0))
        f2, _ = ref.score(np.r_[truth[:9], -truth[9:]], ga, gb, sa, sb, ref.cos2_of(10.0))
        # frames 1 and 3: centres 2.08 apart on the arc of radius 5, points 3.5 to 6.5 away: ray angles of 18 to 34 degrees
        assert f.all() and w.all() and not f2.any()
        assert not ref.score(truth, ga, gb, sa, sb, ref.cos2_of(45.0))[1].any()


@pytest.mark.parametrize("angle", [0.5, 1.0, 2.0])
def test_a_pure_rotation_has_no_wide_point(angle):
    pa, pb, ml, K = ref.rotation_pair()
    n = len(pa)
    y = verified(pa, pb, n, n, ml, 1, 2, n)
    assert n >= 450 and np.isfinite(y["F"]).all() and y["stats"][2] >= 0.9 * n       # some F fits: x_b = H x_a lies on any [e]x H
    r = ref.relative_pose(pa, pb, n, n, y["out"], n, VER["max_dist"], y["F"], K, K, angle, 0.7, 30)
    print("angle", angle, "stats", r["stats"].tolist(), "sigma", r["sigma"])
    assert r["stats"][5] == 0 and r["stats"][7] & ref.FEWPOINTS
    for f, w in zip(r["front"], r["wide"]):
        assert not w.any()                                       # whatever the t: the ray angle does not depend on it


def test_choice_on_six_frames():
    c = ref.scene6()
    g = ref.init_pair(c["kps"], c["counts"], c["pairs"], c["out"], c["stride"], VER["max_dist"], c["F"], c["scene"]["K"], 20.0, 0.7, 30)
    st = g["stats"]
    for m, (a, b) in enumerate(c["pairs"]):
        print((a, b), st[m].tolist(), g["sigma"][m])
        assert st[m, 1 + st[m, 6]] == st[m, 0] and st[m, 0] >= 460
        if b - a == 1:                                           # 12 degrees apart
            assert st[m, 5] <= 1 and st[m, 7] == ref.FEWPOINTS
        else:
            assert st[m, 7] == 0 and st[m, 5] >= 350
    # the yardstick's own numbers
    assert c["pairs"][g["ms"]] == (1, 5) and st[g["ms"], 5] == 477 and st[c["pairs"].index((0, 5)), 5] == 475
    assert g["report"].tolist() == [15, 10, 0, 0, 0, 5, g["ms"], 477]
    assert g["fixed_out"].tolist() == [0, 1, 0, 0, 0, 0] and g["register_out"].tolist() == [1, 0, 1, 1, 1, 0]
    assert np.isnan(g["Rt_out"][[0, 2, 3, 4]]).all() and (g["Rt_out"][1] == np.r_[np.eye(3).reshape(9), np.zeros(3)]).all()
    s = c["scene"]
    Ra, ta = s["Rt"][1, :9].reshape(3, 3), s["Rt"][1, 9:]
    Rb, tb = s["Rt"][5, :9].reshape(3, 3), s["Rt"][5, 9:]
    rot, direction = ref.pose_errors(g["Rt_out"][5], Rb @ Ra.T, tb - Rb @ Ra.T @ ta)
    assert rot <= ROT_DEG and direction <= DIR_DEG, (rot, direction)
    fx, fy, cx, cy = s["K"][1]
    assert g["P_out"][1].tolist() == [fx, 0, cx, 0, 0, fy, cy, 0, 0, 0, 1, 0] and np.isnan(g["P_out"][[0, 2, 3, 4]]).all()
    assert np.array_equal(g["P_out"][5], ref.make_P(s["K"][5], g["Rt_pair"][g["ms"]]))


def test_choice_ties_and_no_eligible_pair():
    st = np.zeros((5, 8), np.int64)
    st[:, 5] = [7, 9, 9, 9, 9]
    st[4, 7] = ref.FEWFRONT
    assert ref.choose(st, [0, 3, 2, 2, 0], [1, 4, 5, 4, 1]) == 3          # wide 9: frames (2, 4) before (2, 5) before (3, 4)
    assert ref.choose(st, [0, 2, 2, 2, 0], [1, 4, 4, 4, 1]) == 1          # all the same frames: the smaller m
    st[:, 7] = ref.FEWPOINTS
    assert ref.choose(st, [0, 3, 2, 2, 0], [1, 4, 5, 4, 1]) == -1
    Rt, P, fixed, reg = ref.frame_outputs(-1, [0], [1], np.zeros((1, 12)), np.ones((3, 4)), None, 3, 3)
    assert np.isnan(Rt).all() and np.isnan(P).all() and not fixed.any() and not reg.any()
