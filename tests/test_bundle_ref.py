"""CPU tests (no GPU): the bundle-adjustment yardstick (tests/bundle_ref.py) against an independent dense formulation.  The
dense side (tests/bundle_dense.py) builds the full Jacobian of every used observation over all free-camera and point
parameters; here it is checked against central differences of the contract's parametrisation (R' = Exp(omega) R,
t' = t + tau, X' = X + dX), and the full damped normal equations are solved without a Schur complement.  Step for step both
must agree; on unrounded projections with two true fixed frames the yardstick must recover the truth."""
import numpy as np
import pytest

import bundle_ref as ref
from bundle_dense import dense_jacobian, dense_solver
from photogrammetry_amd import synth


def _scene(n_points=150, n_frames=5, seed=3, fixed_frames=(0, 4), perturb_seed=9, unrounded=False):
    s = synth.make_scene(n_points, n_frames, seed=seed)
    off, nodes, pid = synth.scene_tracks(s)
    fixed = np.zeros(n_frames, np.int32)
    fixed[list(fixed_frames)] = 1
    Rt, X = synth.perturb(s["Rt"], s["points"][pid], seed=perturb_seed, fixed=fixed)
    kps = s["uv"] if unrounded else s["kps"]
    return s, kps, off, nodes, pid, fixed, Rt, X


def _residual_vector(pb, Rt, X):
    r, _, _, _ = pb.residuals(Rt, X)
    return r.reshape(-1)


def numeric_jacobian(pb, Rt, X, h=1e-6):
    nfr, npt = pb.n_free, len(pb.tracks)
    cols = []
    for k in range(6 * nfr + 3 * npt):
        d = np.zeros(6 * nfr + 3 * npt)
        d[k] = h
        Rp, Xp = pb.apply(Rt, X, d[:6 * nfr], d[6 * nfr:].reshape(-1, 3))
        Rm, Xm = pb.apply(Rt, X, -d[:6 * nfr], -d[6 * nfr:].reshape(-1, 3))
        cols.append((_residual_vector(pb, Rp, Xp) - _residual_vector(pb, Rm, Xm)) / (2 * h))
    return np.stack(cols, 1)


def test_jacobian_matches_central_differences():
    s, kps, off, nodes, pid, fixed, Rt, X = _scene(n_points=40, n_frames=4, fixed_frames=(0,))
    pb = ref.Problem(kps, s["K"], Rt, fixed, off, nodes, X)
    Xp = X[pb.tracks]
    lin = pb.linearise(pb.Rt0, Xp, np.inf)
    Ja = dense_jacobian(pb, lin)
    Jn = numeric_jacobian(pb, pb.Rt0, Xp)
    err = np.abs(Ja - Jn).max(axis=0) / np.maximum(np.abs(Ja).max(axis=0), 1e-300)
    assert err.max() <= 1e-6, err.max()


@pytest.mark.parametrize("huber_px,lambda0", [(np.inf, 1e-3), (2.0, 1e-3), (np.inf, 1e2)])
def test_schur_yardstick_matches_dense_normal_equations(huber_px, lambda0):
    s, kps, off, nodes, pid, fixed, Rt, X = _scene()
    a = ref.bundle_adjust(kps, s["K"], Rt, fixed, off, nodes, X, max_iters=12, huber_px=huber_px, lambda0=lambda0)
    b = ref.bundle_adjust(kps, s["K"], Rt, fixed, off, nodes, X, max_iters=12, huber_px=huber_px, lambda0=lambda0,
                          solver=dense_solver)
    assert a["report"][1] >= 3
    # decisions agree wherever the cost change is resolved (beyond 1e-12 C: a step within rounding of C may go either way)
    n = min(len(a["decisions"]), len(b["decisions"]))
    C = a["trace"][:, 0]
    for i in range(n):
        if not np.isfinite(C[i + 1]) or abs(C[i] - C[i + 1]) <= 1e-12 * C[i] and a["decisions"][i] == "accept":
            break
        assert a["decisions"][i] == b["decisions"][i], (i, a["decisions"], b["decisions"])
    k = n + 1
    fin = np.isfinite(a["trace"][:k, 0]) & np.isfinite(b["trace"][:k, 0])
    assert np.allclose(a["trace"][:k][fin], b["trace"][:k][fin], rtol=1e-9, atol=0)
    scale = np.abs(s["points"]).max() + 5.0
    assert np.abs(a["Rt"] - b["Rt"]).max() <= 1e-9 * scale
    assert np.abs(a["xyz"] - b["xyz"]).max() <= 1e-9 * scale


def test_recovers_the_truth_from_unrounded_projections():
    s, kps, off, nodes, pid, fixed, Rt, X = _scene(n_points=300, n_frames=6, fixed_frames=(0, 5), unrounded=True)
    e = ref.bundle_adjust(kps, s["K"], Rt, fixed, off, nodes, X, max_iters=30)
    assert e["report"][2] in (2, 3), e["report"]
    assert np.abs(e["Rt"] - s["Rt"]).max() <= 1e-8
    assert np.abs(ref.camera_centres(e["Rt"]) - s["centres"]).max() <= 1e-8
    assert np.abs(e["xyz"] - s["points"][pid]).max() <= 1e-8
    assert np.nanmax(e["node_err"]) <= 1e-6


def test_fixed_unknown_and_flagged_frames_and_tracks():
    s, kps, off, nodes, pid, fixed, Rt, X = _scene(n_points=120, n_frames=6, fixed_frames=(0, 5))
    Rt = Rt.copy()
    Rt[2] = np.nan
    flags = np.zeros(len(off) - 1, np.int32)
    flags[::7] = 4
    e = ref.bundle_adjust(kps, s["K"], Rt, fixed, off, nodes, X, track_flags=flags, max_iters=10)
    assert (e["Rt"][[0, 5]].view(np.uint64) == Rt[[0, 5]].view(np.uint64)).all()
    assert np.isnan(e["Rt"][2]).all() and np.isnan(e["P"][2]).all()
    assert (e["xyz"][flags != 0].view(np.uint64) == X[flags != 0].view(np.uint64)).all()
    assert np.isnan(e["node_err"][nodes[:, 0] == 2]).all()
    assert e["report"][3] == 3 and e["report"][4] == int((flags == 0).sum())
    # max_iters = 0: nothing moves, trace[0] is the start cost
    z = ref.bundle_adjust(kps, s["K"], Rt, fixed, off, nodes, X, max_iters=0)
    assert (z["Rt"][np.isfinite(Rt)] == Rt[np.isfinite(Rt)]).all() and (z["xyz"] == X).all()
    assert z["report"][2] == 1 and z["trace"].shape == (1, 2)


def test_one_fixed_frame_terminates_with_a_non_increasing_trace():
    s, kps, off, nodes, pid, fixed, Rt, X = _scene(n_points=120, n_frames=5, fixed_frames=(0,))
    e = ref.bundle_adjust(kps, s["K"], Rt, fixed, off, nodes, X, max_iters=25)
    C = e["trace"][:, 0]
    C = C[np.isfinite(C)]
    assert (np.diff(C) <= 0).all() and e["report"][2] in (1, 2, 3, 4)
