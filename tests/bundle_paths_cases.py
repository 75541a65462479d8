"""Scenes that take bundle adjustment (include/pgx.h) past its first rejected step and to every stop, for
tests/test_bundle_paths_cases.py (CPU, the yardstick alone) and tests/test_gpu_bundle_paths.py.  A plain helper module
without torch.

Small scenes of synth.make_scene (6 frames, 200 points, tracks cut to one length) perturbed hard (8 degrees, 1.0 on the
centres, 1.5 on the points), so that Levenberg-Marquardt rejects steps by a wide margin before it converges, and hand-made
problems for the stops.  `case(name)` gives a problem, `yard(name)` the yardstick's result on it (tests/bundle_ref.py),
computed once and left unchanged.

MARGIN and the compared attempts.  margin_i = |trial_i - C_i| / C_i, the yardstick's trial cost of attempt i against the
cost it is compared with.  An attempt is compared when margin_i >= MARGIN = 1e-6: 1000 x the 1e-9 to which the device's
costs are held, so a device trial cost within that tolerance cannot flip the decision.  Comparison of decisions ends at the
first attempt below MARGIN (the two states may separate from there); a non-PD or small-step attempt has no trial cost and
ends it too, except in nonpd_then_solve, whose non-PD verdicts are exact by construction.

Admission.  Hard starts are often chaotic: two correct solvers drift apart by metres (a variant of reject_ls with two-node
tracks: 1.5e3 on the points).  An iterative scene is admitted only if the yardstick with its Schur solve and with the dense
normal equations (tests/bundle_dense.py) take the same compared decisions, their traces agree to ADMIT_TRACE over the
compared rows and their Rt and xyz to ADMIT_X * SCALE: 1/100 of the bounds to which the device is then held.  SPREADS
records what tests/test_bundle_paths_cases.py measures, which asserts admission and the table.

Not here: a failing Cholesky of the reduced system (s_fail of k_ba_solve).  With every point block positive definite the
reduced system is positive definite in exact arithmetic; an input fails it only by rounding, which two correct solvers need
not share, so no such scene passes admission with both yardstick solvers failing at the same attempt."""
import functools

import numpy as np

import bundle_ref as ref
from bundle_dense import dense_solver
from photogrammetry_amd import synth

MARGIN = 1e-6
SCALE = 5.0                 # the scene scale of the make_scene scenes at offset 0 (tests/test_gpu_bundle.py)
ADMIT_TRACE = 1e-11         # Schur against dense: trace, relative, over the compared rows
ADMIT_X = 1e-10             # ... Rt and xyz, x SCALE
TRACE_TOL = 1e-9            # the device against the yardstick: cost column, relative (geom_gpu)
X_TOL = 1e-8                # ... Rt and xyz, x SCALE (geom_gpu)

REJECT = ("reject_ls", "reject_huber", "reject_gauge")
REJECTING = REJECT + ("reject_ls_roles",)
ITERATIVE = REJECTING + ("nonpd_then_solve",)
# reject_gauge: the scene first tried (make_scene seed 6, 30 iterations) fails admission on its trace (3.7e-11 > ADMIT_TRACE),
# cut short too (its points then differ by 6e-10).  Of the seeds 0 .. 59 searched by the same rule, 33, 35 and 44 pass; all
# three converge, so they are cut short to stop by max_iters (reason 1).  A free scale amplifies rounding: with 1, 2, 4 and
# 16 BLAS threads the trace spread of 35 reaches 1.8e-11 (not admitted), of 33 at 14 iterations 3.5e-12, of 44 at 10
# iterations 1.7e-12.  44 it is: aaaarrrrra
STOPS = ("nonpd_to_lambda_stop", "lambda_stop_at_start", "lambda0_1e16", "zero_cost_start", "behind_at_iters_0")

# make_scene seed, track length, fixed frames, Huber px, max_iters
_SCENES = {
    "reject_ls": (5, 3, (0, 5), np.inf, 25),
    "reject_huber": (7, 6, (0, 5), 2.0, 30),
    "reject_gauge": (44, 3, (0,), 5.0, 10),
    "reject_ls_roles": (5, 3, (0, 5), np.inf, 14),
}

# the yardstick's decisions (first letters), its report, the number of compared attempts, and the Schur-against-dense spreads
# as measured: trace (relative, compared rows), Rt, xyz (absolute), node_err (px).  Asserted by test_bundle_paths_cases.py to
# a factor of SPREAD_SLACK above, or a tenth of the admission bound where that is more (figures rounded up; a few ulp, and
# another BLAS may round differently.  Admission itself has no slack)
SPREAD_SLACK = 10.0
SPREADS = {
    "reject_ls": dict(decisions="aarrrraraaaaaaaa", report=[16, 11, 2, 4, 200, 600, 0, 0], compared=14,
                      trace=1.3e-13, Rt=1.8e-15, xyz=3.8e-15, node_err=2.4e-13),
    "reject_huber": dict(decisions="aaarrrraaaaaarrrrrrra", report=[21, 10, 2, 4, 200, 1200, 0, 0], compared=12,
                         trace=1.1e-13, Rt=3.3e-12, xyz=5.6e-12, node_err=1.3e-9),
    "reject_gauge": dict(decisions="aaaarrrrra", report=[10, 5, 1, 5, 200, 600, 0, 0], compared=10,
                         trace=1.7e-12, Rt=1.4e-12, xyz=4.4e-12, node_err=1.8e-9),
    "reject_ls_roles": dict(decisions="aarrrraraaaaaa", report=[14, 9, 1, 5, 199, 596, 0, 0], compared=14,
                            trace=2.7e-13, Rt=8.9e-16, xyz=5.5e-15, node_err=4.3e-13),
    "nonpd_then_solve": dict(decisions="nnnnaaa", report=[7, 3, 1, 1, 13, 40, 0, 4], compared=7,
                             trace=4.5e-15, Rt=1.8e-15, xyz=1.5e-14, node_err=8.9e-14),
}
# node_err has no project tolerance: the device is held to 100 x the largest Schur-against-dense spread over the admitted
# scenes, at least 1e-9 px
NODE_ERR_TOL = max(1e-9, 100.0 * max(v["node_err"] for v in SPREADS.values()))


def _reject_scene(seed, L, fixed_frames, nf=6):
    s = synth.make_scene(200, nf, seed=seed)
    off, nodes, pid = synth.cut_tracks(s, np.full(200, L), seed=1)
    fixed = np.zeros(nf, np.int32)
    fixed[list(fixed_frames)] = 1
    Rt, X = synth.perturb(s["Rt"], s["points"][pid], seed=7, rot_deg=8.0, centre_sigma=1.0, point_sigma=1.5, fixed=fixed)
    return s, off, nodes, pid, fixed, Rt, X


def _problem(kps, K, Rt, fixed, off, nodes, X, flags=None, max_iters=25, huber=np.inf, lambda0=1e-3, **more):
    return dict(kps=list(kps), K=np.ascontiguousarray(K, np.float64), Rt=np.ascontiguousarray(Rt, np.float64),
                fixed=np.asarray(fixed, np.int32), off=np.asarray(off, np.int32), nodes=np.asarray(nodes, np.int32).reshape(-1, 2),
                X=np.ascontiguousarray(X, np.float64), flags=flags, max_iters=max_iters, huber=huber, lambda0=lambda0, **more)


def _roles():
    """reject_ls with: frame 6 known and free but seen by no track; frame 7 UNKNOWN by a NaN in its K, with one keypoint that
    track `t_unknown` gets as a fourth node; track `t_fixed` cut to its two nodes in the fixed frames 0 and 5 (its point is
    seen in both); track `t_flag` flagged.  Cut at 14 iterations, all of them compared: the last step before the rounding floor
    still moves a point by 1e-9, and whether the first step at the floor is taken depends on the BLAS (reject_ls runs on to
    its stop)"""
    s, off, nodes, pid, fixed, Rt, X = _reject_scene(5, 3, (0, 5))
    where = [dict(zip(p.tolist(), range(len(p)))) for p in s["point_id"]]
    t_fixed = next(t for t in range(len(pid)) if int(pid[t]) in where[0] and int(pid[t]) in where[5])
    t_unknown, t_flag = (t_fixed + 50) % len(pid), (t_fixed + 100) % len(pid)
    tracks = [nodes[off[t]:off[t + 1]].tolist() for t in range(len(pid))]
    tracks[t_fixed] = [[0, where[0][int(pid[t_fixed])]], [5, where[5][int(pid[t_fixed])]]]
    tracks[t_unknown] = tracks[t_unknown] + [[7, 0]]
    off2 = np.concatenate([[0], np.cumsum([len(t) for t in tracks])]).astype(np.int32)
    nodes2 = np.array([n for t in tracks for n in t], np.int32)
    kps = list(s["kps"]) + [s["kps"][0][:0], s["kps"][0][:1]]
    K = np.concatenate([s["K"], s["K"][:2]])
    K[7, 2] = np.nan
    Rt2 = np.concatenate([Rt, Rt[2:3], s["Rt"][3:4]])
    flags = np.zeros(len(pid), np.int32)
    flags[t_flag] = 4
    return _problem(kps, K, Rt2, np.concatenate([fixed, [0, 0]]), off2, nodes2, X, flags=flags, max_iters=14,
                    t_fixed=t_fixed, t_unknown=t_unknown, t_flag=t_flag)


def _three_frames(tz=0.0):
    """K dyadic, R = I, t dyadic: frame 0 at the origin, frames 1 and 2 beside it and tz behind.  12 points on a 1/32 grid at
    z = 4 or 8, seen by all three; keypoints at the rounded projections.  At tz = 0 these are the exact projections (every
    product and sum of the projection is exact in float64, in any order and under FMA)"""
    K = np.tile([1024.0, 1024.0, 512.0, 384.0], (3, 1))
    Rt = np.zeros((3, 12))
    Rt[:, [0, 4, 8]] = 1.0
    Rt[1, 9:] = (-0.5, 0.25, tz)
    Rt[2, 9:] = (0.5, -0.25, tz)
    rng = np.random.default_rng(3)
    X = np.concatenate([rng.integers(-24, 25, (12, 2)) / 32.0, np.where(np.arange(12) % 2 == 0, 4.0, 8.0)[:, None]], 1)
    kps = []
    for f in range(3):
        p = X + Rt[f, 9:]
        uv = np.stack([K[f, 0] * (p[:, 0] / p[:, 2]) + K[f, 2], K[f, 1] * (p[:, 1] / p[:, 2]) + K[f, 3]], 1)
        assert (uv >= 0).all() and (tz != 0.0 or (uv == np.round(uv)).all())
        kps.append(np.round(uv))
    off = np.arange(0, 37, 3)
    nodes = np.array([[f, t] for t in range(12) for f in range(3)], np.int32)
    return kps, K, Rt, off, nodes, X


@functools.lru_cache(maxsize=None)
def case(name):
    """-> dict(kps, K, Rt, fixed, off, nodes, X, flags, max_iters, huber, lambda0 [, roles]) of a named scene; left unchanged"""
    if name in REJECT:
        seed, L, ff, huber, iters = _SCENES[name]
        s, off, nodes, pid, fixed, Rt, X = _reject_scene(seed, L, ff)
        return _problem(s["kps"], s["K"], Rt, fixed, off, nodes, X, max_iters=iters, huber=huber)
    if name == "reject_ls_roles":
        return _roles()
    if name == "reject_ls_100":           # the full-length trace
        return dict(case("reject_ls"), max_iters=100)
    if name == "lambda_stop_at_start":
        return dict(case("reject_ls"), lambda0=1e17)
    if name == "lambda0_1e16":            # not > 1e16: one attempt, whose step is far below the small-step bound
        return dict(case("reject_ls"), lambda0=1e16)
    if name == "behind_at_iters_0":
        # three points put 2 units behind the camera of their track's first node: p = R (X - C) = (0, 0, -2) there
        c = dict(case("reject_ls"), max_iters=0)
        X = c["X"].copy()
        for t in (10, 90, 170):
            f = c["nodes"][c["off"][t], 0]
            R = c["Rt"][f, :9].reshape(3, 3)
            X[t] = -R.T @ c["Rt"][f, 9:] - 2.0 * R[2]
        return dict(c, X=X, behind=(10, 90, 170))
    if name == "zero_cost_start":
        kps, K, Rt, off, nodes, X = _three_frames()
        return _problem(kps, K, Rt, [1, 0, 0], off, nodes, X, max_iters=25)
    if name == "nonpd_to_lambda_stop":
        # the three-frame problem with keypoints a few pixels off (a cost to work on) and track 5's point put at (a, b, 0.0),
        # a, b != 0: frame 0 (fixed, R = I, t = 0 exactly; frames 1 and 2 stand 4 behind it) sees it at z = 0 in every summation
        # order and under FMA, its residual is +inf in both coordinates, the cost +inf and the point block NaN.  Every attempt is
        # non-PD until lambda passes 1e16
        kps, K, Rt, off, nodes, X = _three_frames(tz=4.0)
        rng = np.random.default_rng(4)
        kps = [k + rng.integers(-3, 4, k.shape) for k in kps]
        X = X.copy()
        X[5] = (0.5, 0.25, 0.0)
        return _problem(kps, K, Rt, [1, 1, 0], off, nodes, X, max_iters=25)
    if name == "nonpd_then_solve":
        # Non-PD attempts followed by solved ones: the non-PD flag has to be cleared.  In exact arithmetic a damped block is
        # always positive definite, so the non-PD verdict is made by absorption instead: frames 3 .. 6 are fixed copies of frame
        # 0 and track 12 sees the point (4, 0, 4) in all four at its exact projection.  Its block is 2^18 [[1, 0, -1], [0, 1, 0],
        # [-1, 0, 1]]: singular, every entry and every Cholesky step exact (pivots 512, 512, then a22 - 2^18).  Below lambda =
        # 1.1e-16 the damped diagonal v + lambda v rounds to v and the last pivot is exactly 0 in any implementation; at 1e-15
        # it is 8 ulp (4.7e-10) against a rounding bound of 2e-10.  The track's gradient is exactly 0 and its cameras are fixed, so
        # its point does not move whatever the inverse.  lambda0 = 1e-19: four non-PD attempts, then Gauss-Newton steps on the rest
        kps, K, Rt, off, nodes, X = _three_frames(tz=4.0)
        rng = np.random.default_rng(5)
        kps = [k + rng.integers(-3, 4, k.shape) for k in kps] + [np.array([[1536.0, 384.0]])] * 4
        X = np.concatenate([X + rng.normal(scale=0.05, size=X.shape), [[4.0, 0.0, 4.0]]])
        K, Rt = np.concatenate([K, np.tile(K[0], (4, 1))]), np.concatenate([Rt, np.tile(Rt[0], (4, 1))])
        off = np.concatenate([off, [off[-1] + 4]])
        nodes = np.concatenate([nodes, [[3, 0], [4, 0], [5, 0], [6, 0]]])
        return _problem(kps, K, Rt, [1, 1, 0, 1, 1, 1, 1], off, nodes, X, max_iters=7, lambda0=1e-19, nonpd_compared=True)
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def yard(name, dense=False):
    """The yardstick's result on case(name), with its Schur solve or with the dense normal equations; left unchanged"""
    c = case(name)
    with np.errstate(all="ignore"):
        return ref.bundle_adjust(c["kps"], c["K"], c["Rt"], c["fixed"], c["off"], c["nodes"], c["X"], track_flags=c["flags"],
                                 max_iters=c["max_iters"], huber_px=c["huber"], lambda0=c["lambda0"],
                                 solver=dense_solver if dense else None)


def margins(e):
    """margin_i of every attempt of a yardstick result (NaN where the attempt has no trial cost)"""
    C = e["trace"][:len(e["trial"]), 0]
    with np.errstate(all="ignore"):
        return np.abs(e["trial"] - C) / C


def compared(e, margin=MARGIN, nonpd=False):
    """The number of leading attempts whose decision is compared.  nonpd: non-PD attempts count as compared (a scene whose
    non-PD verdicts are exact by construction: nonpd_then_solve)"""
    n = 0
    for m, d in zip(margins(e), e["decisions"]):
        if not (m >= margin or nonpd and d == "nonpd"):
            break
        n += 1
    return n


def letters(decisions):
    return "".join(d[0] for d in decisions)


def spreads(name):
    """Schur against dense on an iterative scene -> dict(compared, same (the compared decisions are equal), trace, Rt, xyz,
    node_err)"""
    a, b = yard(name), yard(name, dense=True)
    npd = case(name).get("nonpd_compared", False)
    n = min(compared(a, nonpd=npd), compared(b, nonpd=npd))
    ta, tb = a["trace"][:n + 1], b["trace"][:n + 1]
    return dict(compared=n, same=a["decisions"][:n] == b["decisions"][:n] and compared(a, nonpd=npd) == compared(b, nonpd=npd),
                trace=float((np.abs(ta - tb) / np.abs(ta)).max()), Rt=float(np.nanmax(np.abs(a["Rt"] - b["Rt"]))),
                xyz=float(np.abs(a["xyz"] - b["xyz"]).max()), node_err=float(np.nanmax(np.abs(a["node_err"] - b["node_err"]))),
                nan_same=bool((np.isnan(a["Rt"]) == np.isnan(b["Rt"])).all()
                              and (np.isnan(a["node_err"]) == np.isnan(b["node_err"])).all()))
