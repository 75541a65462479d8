"""CPU test (no GPU): the registration yardstick (tests/register_ref.py) is tied to the truth -- P3P finds the true pose of
exact triples, the Gauss-Newton Jacobian matches central differences, and on synth.make_scene scenes with two known
cameras every other frame is registered to the true pose, also far from the origin and with planted outliers."""
import math

import numpy as np

import register_ref as ref
import triangulate_ref as tri
from photogrammetry_amd import synth


def _rot(rng):
    q = rng.normal(size=4)
    q /= np.linalg.norm(q)
    w, x, y, z = q
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                     [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                     [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])


def test_p3p_finds_the_true_pose():
    rng = np.random.default_rng(11)
    hits, trials = 0, 10000
    for _ in range(trials):
        R = _rot(rng)
        t = rng.uniform(-1, 1, 3)
        while True:
            Xc = np.stack([rng.uniform(-1, 1, 3) + np.array([0, 0, 5.0]) for _ in range(3)])   # camera frame, in front
            a = np.linalg.norm(np.cross(Xc[1] - Xc[0], Xc[2] - Xc[0]))
            if a > 0.2:   # well conditioned: not near collinear
                break
        X = (Xc - t) @ R       # world points: Xc = R X + t
        y = Xc / np.linalg.norm(Xc, axis=1, keepdims=True)
        sols = [s for s in ref.p3p(y, X) if s is not None]
        if any(np.abs(np.array(Rs) - R.reshape(9)).max() <= 1e-9 and np.abs(np.array(ts) - t).max() <= 1e-9 for Rs, ts in sols):
            hits += 1
    assert hits >= 0.999 * trials, hits


def test_jacobian_matches_central_differences():
    rng = np.random.default_rng(2)
    R, t = _rot(rng).reshape(9), np.array([0.1, -0.2, 6.0])
    X = rng.uniform(-1, 1, (20, 3))
    cu, cv = rng.uniform(-50, 50, 20), rng.uniform(-50, 50, 20)
    fx, fy = 1100.0, 1000.0
    J = ref.jacobian(R, t, X, fx, fy)
    h = 1e-6
    for k in range(6):
        d = np.zeros(6)
        d[k] = h
        rp = ref.residuals(ref.rotate_left(d[:3], R), t + d[3:], X, cu, cv, fx, fy)
        rm = ref.residuals(ref.rotate_left(-d[:3], R), t - d[3:], X, cu, cv, fx, fy)
        num = (rp - rm) / (2 * h)
        assert np.abs(num - J[:, :, k]).max() <= 1e-6 * (1 + np.abs(J[:, :, k]).max()), k


def _setup(offset=(0.0, 0.0, 0.0), n_points=600, seed=3):
    s = synth.make_scene(n_points, 12, seed=seed, offset=offset)
    off, nodes, pid = synth.scene_tracks(s)
    P = s["P"].copy()
    P[2:] = np.nan
    tr = tri.triangulate(s["uv"], P, off, nodes, 0.0, 1e9, 5)
    reg = np.ones(12, np.int32)
    reg[:2] = 0
    return s, off, nodes, tr, reg


def test_registers_every_frame_to_the_truth():
    s, off, nodes, tr, reg = _setup()
    e = ref.register(s["uv"], s["K"], s["Rt"], reg, off, nodes, tr["xyz"], tr["flags"], n_samples=64, inlier_px=2.0)
    assert (e["frame_stats"][2:, 3] == 0).all(), e["frame_stats"]
    assert (e["Rt"][:2] == s["Rt"][:2]).all()
    assert np.abs(e["Rt"][2:] - s["Rt"][2:]).max() <= 1e-8
    assert e["report"][0] == 10 and e["report"][1] == 10


def test_offset_moves_the_centres_by_the_offset():
    off3 = np.array([2e4, -1e4, 3e4])
    s0, o0, n0, t0, reg = _setup()
    s1, o1, n1, t1, _ = _setup(offset=tuple(off3))
    e0 = ref.register(s0["uv"], s0["K"], s0["Rt"], reg, o0, n0, t0["xyz"], t0["flags"], n_samples=64)
    e1 = ref.register(s1["uv"], s1["K"], s1["Rt"], reg, o1, n1, t1["xyz"], t1["flags"], n_samples=64)
    assert (e1["frame_stats"][2:, 3] == 0).all()
    for f in range(2, 12):
        c0, c1 = ref.centre(e0["Rt"][f]), ref.centre(e1["Rt"][f])
        assert np.abs(c1 - (c0 + off3)).max() <= 1e-9 * np.abs(off3).max(), (f, c1 - c0 - off3)


def test_moved_keypoints_are_outliers():
    s, off, nodes, tr, reg = _setup()
    rng = np.random.default_rng(5)
    uv = [u.copy() for u in s["uv"]]
    f = 7
    moved = rng.choice(len(uv[f]), size=len(uv[f]) // 5, replace=False)
    uv[f][moved] = rng.uniform([0, 0], [1920, 1080], size=(len(moved), 2))
    ip = 2.0
    e = ref.register(uv, s["K"], s["Rt"], reg, off, nodes, tr["xyz"], tr["flags"], n_samples=128, inlier_px=ip)
    assert e["frame_stats"][f, 3] == 0
    far = set(int(k) for k in moved if np.linalg.norm(uv[f][k] - s["uv"][f][k]) > ip)
    ni = e["node_inlier"]
    for o in range(len(nodes)):
        if nodes[o, 0] == f and int(nodes[o, 1]) in far:
            assert ni[o] == 0, o
    assert np.abs(e["Rt"][f] - s["Rt"][f]).max() <= 1e-8
    assert not math.isnan(e["frame_err"][f, 0])
