"""GPU tests of bundle adjustment (pgx_bundle_adjust_dev / pgx_bundle_adjust; include/pgx.h).  Scenes are synth.make_scene's
with their true tracks, cameras and points perturbed by synth.perturb (0.3 degrees of rotation, 1 % of the radius on the
centres, 1 % of the box on the points).  Results are held to the numpy yardstick of tests/bundle_ref.py, which also sets
every accuracy threshold here, to the truth, to themselves across runs, capacities, slot layouts and the host form (bit for
bit), and every error the contract lists is provoked through an argument."""
import numpy as np
import pytest
import torch

import bundle_ref as ref
import geom_gpu as g
import photogrammetry_amd as pg
from geom_gpu import DEV, F64, I32, INF, bits, device_problem
from geom_gpu import ba_check_against_yardstick as check_against_yardstick
from geom_gpu import ba_run as run
from photogrammetry_amd import synth

pytestmark = pytest.mark.gpu


def same_bits(a, b):
    g.same_bits(a, b, g.BA_KEYS)


def problem(n_points=2000, nf=12, seed=5, offset=(0.0, 0.0, 0.0), fixed_frames=(0, 11), perturb_seed=7, pairs=None):
    s = synth.make_scene(n_points, nf, seed=seed, offset=offset, pairs=pairs)
    off, nodes, pid = synth.scene_tracks(s)
    fixed = np.zeros(nf, np.int32)
    fixed[list(fixed_frames)] = 1
    Rt, X = synth.perturb(s["Rt"], s["points"][pid], seed=perturb_seed, fixed=fixed)
    return s, off, nodes, pid, fixed, Rt, X


def test_against_yardstick_truth_and_offset(engine):
    """At offset (2e4, -1e4, 3e4) the contract's rotation about the world origin couples omega and tau by the 3.7e4-unit
    centre distance: the yardstick itself does not converge in 100 iterations there, so the shifted
    scene is held to the yardstick step for step and the truth checks run on the unshifted one."""
    for offset in [(0.0, 0.0, 0.0), (2e4, -1e4, 3e4)]:
        s, off, nodes, pid, fixed, Rt, X = problem(offset=offset)
        d = device_problem(s["kps"], off, nodes)
        got = run(engine, d, s["K"], Rt, fixed, X)
        e = ref.bundle_adjust(s["kps"], s["K"], Rt, fixed, off, nodes, X, max_iters=20)
        scale = 5.0 + np.abs(offset).max()
        dg, de = check_against_yardstick(got, e, scale)
        print("offset", offset, "gpu", dg, got["report"].tolist(), "yardstick", de, e["report"].tolist())
        free = fixed == 0
        assert np.abs(ref.camera_centres(got["Rt"])[free] - ref.camera_centres(e["Rt"])[free]).max() <= 1e-8 * scale
        if offset != (0.0, 0.0, 0.0):
            continue
        # truth: the rms reprojection error is the rounding noise's (the yardstick's optimum: 0.381 px), the free centres move
        # toward the true ones by the yardstick's factor (187)
        rms = np.sqrt(np.nanmean(got["node_err"] ** 2))
        rms_ref = np.sqrt(np.nanmean(e["node_err"] ** 2))
        assert abs(rms - rms_ref) <= 1e-9 * rms_ref and rms <= 0.41, (rms, rms_ref)
        err0 = np.linalg.norm(ref.camera_centres(Rt)[free] - s["centres"][free], axis=1).max()
        err_ref = np.linalg.norm(ref.camera_centres(e["Rt"])[free] - s["centres"][free], axis=1).max()
        err = np.linalg.norm(ref.camera_centres(got["Rt"])[free] - s["centres"][free], axis=1).max()
        assert err0 / err >= 0.99 * (err0 / err_ref) and err0 / err_ref > 50, (err0, err, err_ref)


def test_huber_resists_wrong_keypoints(engine):
    s, off, nodes, pid, fixed, Rt, X = problem(n_points=1500, seed=6)
    rng = np.random.default_rng(3)
    nodes = nodes.copy()
    bad = rng.random(len(nodes)) < 0.03
    for i in np.flatnonzero(bad):
        f, k = nodes[i]
        nodes[i, 1] = (k + 1 + rng.integers(0, s["counts"][f] - 1)) % s["counts"][f]
    # the same frame may now hold two nodes of one track only if the wrong keypoint is another node of it: never, since each
    # keypoint belongs to one point and one track
    d = device_problem(s["kps"], off, nodes)
    free = fixed == 0

    def cerr(R):
        return np.linalg.norm(ref.camera_centres(R)[free] - s["centres"][free], axis=1).max()
    g_h, g_l = run(engine, d, s["K"], Rt, fixed, X, huber=2.0), run(engine, d, s["K"], Rt, fixed, X)
    e_h = ref.bundle_adjust(s["kps"], s["K"], Rt, fixed, off, nodes, X, max_iters=20, huber_px=2.0)
    e_l = ref.bundle_adjust(s["kps"], s["K"], Rt, fixed, off, nodes, X, max_iters=20)
    factor_ref = cerr(e_l["Rt"]) / cerr(e_h["Rt"])
    print("camera error: +inf %.3g, huber 2 %.3g; yardstick %.3g / %.3g" % (cerr(g_l["Rt"]), cerr(g_h["Rt"]), cerr(e_l["Rt"]),
                                                                            cerr(e_h["Rt"])))
    assert factor_ref > 3.0
    assert cerr(g_l["Rt"]) / cerr(g_h["Rt"]) >= 0.9 * factor_ref


def test_identical_bits_across_runs_capacity_slots_and_host_form(engine):
    s, off, nodes, pid, fixed, Rt, X = problem(n_points=800, nf=9, seed=8, fixed_frames=(1, 6), perturb_seed=2)
    flags = np.zeros(len(off) - 1, np.int32)
    flags[::11] = 8
    d = device_problem(s["kps"], off, nodes)
    a = run(engine, d, s["K"], Rt, fixed, X, huber=2.0, flags=flags)
    assert a["report"][1] >= 2
    same_bits(a, run(engine, d, s["K"], Rt, fixed, X, huber=2.0, flags=flags))
    same_bits(a, run(engine, d, s["K"], Rt, fixed, X, huber=2.0, flags=flags, max_tracks=d["n_tracks"] + 777))
    slots = np.random.default_rng(0).permutation(9 + 3)[:9]
    same_bits(a, run(engine, device_problem(s["kps"], off, nodes, slots=slots, n_slots=12), s["K"], Rt, fixed, X, huber=2.0,
                     flags=flags))
    h = engine.bundle_adjust(s["kps"], s["K"], Rt, fixed, off, nodes, X, track_flags=flags, max_iters=20, huber_px=2.0)
    same_bits(a, h)


def test_edge_cases(engine):
    s, off, nodes, pid, fixed, Rt, X = problem(n_points=600, nf=8, seed=4, fixed_frames=(0, 7))
    d = device_problem(s["kps"], off, nodes)
    # max_iters = 0: nothing moves, P_out = K [R | t], trace[0] = C0
    z = run(engine, d, s["K"], Rt, fixed, X, iters=0)
    assert bits(z["Rt"]) == bits(Rt) and bits(z["xyz"]) == bits(X)
    e0 = ref.bundle_adjust(s["kps"], s["K"], Rt, fixed, off, nodes, X, max_iters=0)
    assert bits(z["P"]) == bits(e0["P"])
    assert abs(z["trace"][0, 0] - e0["trace"][0, 0]) <= 1e-12 * e0["trace"][0, 0] and z["trace"][0, 1] == 1e-3
    assert z["report"][2] == 1 and z["report"][0] == 0
    # fixed frames bit-unchanged, a NaN frame skipped (its rows copied, P NaN, its nodes' errors NaN)
    Rt2 = Rt.copy()
    Rt2[3] = np.nan
    g = run(engine, d, s["K"], Rt2, fixed, X)
    assert bits(g["Rt"][[0, 7]]) == bits(Rt2[[0, 7]]) and np.isnan(g["Rt"][3]).all() and np.isnan(g["P"][3]).all()
    assert np.isnan(g["node_err"][nodes[:, 0] == 3]).all() and g["report"][3] == 5
    e = ref.bundle_adjust(s["kps"], s["K"], Rt2, fixed, off, nodes, X, max_iters=20)
    check_against_yardstick(g, e, 5.0)
    # one fixed frame: the scale is free, the trace does not increase and the call ends
    f1 = np.zeros(8, np.int32)
    f1[0] = 1
    o = run(engine, d, s["K"], Rt, f1, X, iters=30)
    C = o["trace"][:o["report"][0] + 1, 0]
    assert (np.diff(C) <= 0).all() and o["report"][2] in (1, 2, 3, 4) and np.isnan(o["trace"][o["report"][0] + 1:]).all()


def test_chain_on_one_stream(engine):
    """tracks_dev -> triangulate from perturbed cameras -> bundle_adjust_dev with the triangulation's flags -> triangulate on
    P_out, one sync at the end: the second triangulation's rms is lower"""
    from photogrammetry_amd._lib import PGX_DIST_NONE
    nf = 10
    pairs = [(a, a + k) for k in (1, 2) for a in range(nf - k)]
    s = synth.make_scene(1200, nf, seed=12, pairs=pairs)
    fixed = np.zeros(nf, np.int32)
    fixed[[0, nf - 1]] = 1
    Rt, _ = synth.perturb(s["Rt"], np.zeros((1, 3)), seed=4, fixed=fixed)
    Kf = [np.array([[k[0], 0, k[2]], [0, k[1], k[3]], [0, 0, 1.0]]) for k in s["K"]]
    P = np.stack([(Kf[f] @ np.c_[Rt[f, :9].reshape(3, 3), Rt[f, 9:]]).reshape(12) for f in range(nf)])
    stride = max(len(k) for k in s["kps"])
    kp = np.zeros((nf, stride), dtype=pg.KEYPOINT_DTYPE)
    counts = np.zeros(nf, np.int32)
    for f, k in enumerate(s["kps"]):
        kp[f, :len(k)] = k
        counts[f] = len(k)
    m = np.zeros((len(pairs), stride, 3), np.int32)
    m[:, :, 2] = PGX_DIST_NONE
    for i, rows in enumerate(s["lists"]):
        m[i, :len(rows)] = np.stack([rows["k1"], rows["k2"], rows["dist"]], 1)
    N = nf * stride
    dkp = torch.from_numpy(kp.view(np.int32).reshape(nf, stride, 4)).to(DEV)
    dm, dc = torch.from_numpy(m).to(DEV), torch.from_numpy(counts).to(DEV)
    dpl = torch.tensor(pairs, **I32)
    track_of, offsets, nodes = torch.empty((nf, stride), **I32), torch.empty((N + 1,), **I32), torch.empty((N, 2), **I32)
    tsum = torch.empty(8, **I32)
    xyz, q, fl, summ = torch.empty((N, 3), **F64), torch.empty((N, 3), **F64), torch.empty(N, **I32), torch.empty(8, **I32)
    xyz2, q2, fl2, summ2 = torch.empty((N, 3), **F64), torch.empty((N, 3), **F64), torch.empty(N, **I32), torch.empty(8, **I32)
    dP = torch.from_numpy(P).to(DEV)
    dK, dRt, dfx = torch.from_numpy(s["K"]).to(DEV), torch.from_numpy(Rt).to(DEV), torch.from_numpy(fixed).to(DEV)
    Rt_out, P_out, X_out = torch.empty((nf, 12), **F64), torch.empty((nf, 12), **F64), torch.empty((N, 3), **F64)
    trace, report = torch.empty((21, 2), **F64), torch.empty(8, **I32)
    torch.cuda.synchronize()
    engine.tracks_dev(dm, dc, dpl, len(pairs), nf, stride, nf, 0, 2, track_of, offsets, nodes, tsum)
    engine.triangulate_tracks_dev(dkp, nf, stride, nf, dP, offsets, nodes, tsum, N, xyz, q, fl, summ, 1.0, INF, 10)
    engine.bundle_adjust_dev(dkp, nf, stride, nf, dK, dRt, dfx, offsets, nodes, tsum, N, xyz, Rt_out, P_out, X_out, trace, report,
                             20, INF, 1e-3, d_track_flags=fl)
    engine.triangulate_tracks_dev(dkp, nf, stride, nf, P_out, offsets, nodes, tsum, N, xyz2, q2, fl2, summ2, 1.0, INF, 10)
    engine.check_status()
    n = int(tsum[0].item())
    f1, f2 = fl.cpu().numpy()[:n], fl2.cpu().numpy()[:n]
    ok = (f1 == 0) & (f2 == 0)
    r1, r2 = q.cpu().numpy()[:n, 0][ok], q2.cpu().numpy()[:n, 0][ok]
    rms1, rms2 = np.sqrt(np.mean(r1 ** 2)), np.sqrt(np.mean(r2 ** 2))
    print("triangulation rms before %.4f after %.4f, report %s" % (rms1, rms2, report.cpu().tolist()))
    assert ok.sum() > 500 and rms2 < rms1 and rms2 <= 0.45


def test_errors(engine):
    s, off, nodes, pid, fixed, Rt, X = problem(n_points=300, nf=6, seed=2, fixed_frames=(0, 5))
    d = device_problem(s["kps"], off, nodes)
    # reported through pgx_check_status
    bad = Rt.copy()
    bad[2, 0] *= 1.01                       # not a rotation
    with pytest.raises(pg.ArgumentException):
        run(engine, d, s["K"], bad, fixed, X)
    refl = Rt.copy()
    refl[2, 6:9] *= -1.0                    # det R = -1
    with pytest.raises(pg.ArgumentException):
        run(engine, d, s["K"], refl, fixed, X)
    d2 = dict(d, identity=False, ids=torch.tensor([0, 1, 2, 3, 4, 4], **I32))
    with pytest.raises(pg.ArgumentException):
        run(engine, d2, s["K"], Rt, fixed, X)
    with pytest.raises(pg.ArgumentException):
        run(engine, d, s["K"], Rt, np.zeros(6, np.int32), X)        # no fixed frame
    with pytest.raises(pg.CapacityError):
        run(engine, d, s["K"], Rt, fixed, X, max_tracks=d["n_tracks"] - 3)
    # a track with two nodes in one frame
    dn = nodes.copy()
    dn[off[0] + 1, 0] = dn[off[0], 0]
    with pytest.raises(pg.ArgumentException):
        run(engine, device_problem(s["kps"], off, dn), s["K"], Rt, fixed, X)
    # 129 free frames (+ 1 fixed): capacity, no iteration
    nf = 130
    Kb = np.tile(s["K"][0], (nf, 1))
    Rb = np.tile(Rt[0], (nf, 1))
    fb = np.zeros(nf, np.int32)
    fb[0] = 1
    kb = [s["kps"][0]] + [s["kps"][0][:0]] * (nf - 1)
    db = device_problem(kb, [0, 2], np.array([[0, 0], [1, 0]], np.int32))
    with pytest.raises(pg.CapacityError):
        run(engine, db, Kb, Rb, fb, np.zeros((1, 3)))
    # returned at once
    nf = 6
    t = dict(K=torch.from_numpy(s["K"]).to(DEV), Rt=torch.from_numpy(Rt).to(DEV), fx=torch.from_numpy(fixed).to(DEV))
    n = d["n_tracks"]
    Xd, o1, o2, o3 = torch.zeros((n, 3), **F64), torch.zeros((nf, 12), **F64), torch.zeros((nf, 12), **F64), torch.zeros((n, 3), **F64)
    tr, rep = torch.zeros((102, 2), **F64), torch.zeros(8, **I32)
    torch.cuda.synchronize()

    def call(**kw):
        args = dict(max_iters=5, huber_px=INF, lambda0=1e-3)
        args.update(kw)
        engine.bundle_adjust_dev(d["kp"], nf, d["stride"], nf, t["K"], t["Rt"], t["fx"], d["off"], d["nodes"], d["tsum"], n, Xd, o1,
                                 o2, o3, args.pop("trace", tr), rep, **args)
    for kw in (dict(max_iters=-1), dict(max_iters=101), dict(huber_px=0.0), dict(huber_px=float("nan")), dict(huber_px=-1.0),
               dict(lambda0=0.0), dict(lambda0=INF), dict(lambda0=float("nan")), dict(trace=0)):
        with pytest.raises(pg.ArgumentException):
            call(**kw)
    with pytest.raises(pg.ArgumentException):
        engine.bundle_adjust_dev(d["kp"], nf, d["stride"], nf + 1, t["K"], t["Rt"], t["fx"], d["off"], d["nodes"], d["tsum"], n, Xd,
                                 o1, o2, o3, tr, rep)
    with pytest.raises(pg.ArgumentException):
        engine.bundle_adjust_dev(d["kp"], nf, d["stride"], nf, t["K"], t["Rt"], t["fx"], d["off"], d["nodes"], d["tsum"], -1, Xd,
                                 o1, o2, o3, tr, rep)
    engine.check_status()
