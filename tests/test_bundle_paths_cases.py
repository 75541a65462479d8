"""CPU tests (no GPU, the yardstick alone): every scene of tests/bundle_paths_cases.py reaches the path it is named for, the
iterative ones pass the admission rule (Schur solve against dense normal equations; see that module), and the recorded
spreads are what is measured here."""
import numpy as np
import pytest

import bundle_paths_cases as c
import bundle_ref as ref


def bits(a):
    return np.ascontiguousarray(a).view(np.uint8).tobytes()


@pytest.mark.parametrize("name", c.ITERATIVE)
def test_admission_and_recorded_spreads(name):
    a, b, s, rec = c.yard(name), c.yard(name, dense=True), c.spreads(name), c.SPREADS[name]
    print(name, c.letters(a["decisions"]), c.letters(b["decisions"]), a["report"].tolist(), s)
    print("margins", ["%.1e" % m for m in c.margins(a)])
    assert s["same"] and s["nan_same"]
    assert s["trace"] <= c.ADMIT_TRACE
    assert s["Rt"] <= c.ADMIT_X * c.SCALE and s["xyz"] <= c.ADMIT_X * c.SCALE
    # the table
    assert c.letters(a["decisions"]) == rec["decisions"] and a["report"].tolist() == rec["report"]
    assert s["compared"] == c.compared(a, nonpd=c.case(name).get("nonpd_compared", False)) == rec["compared"]
    floor = dict(trace=0.1 * c.ADMIT_TRACE, Rt=0.1 * c.ADMIT_X * c.SCALE, xyz=0.1 * c.ADMIT_X * c.SCALE, node_err=0.01 * c.NODE_ERR_TOL)
    for k in ("trace", "Rt", "xyz", "node_err"):
        assert s[k] <= max(c.SPREAD_SLACK * rec[k], floor[k]), (k, s[k], rec[k])
    assert c.SPREAD_SLACK * s["node_err"] <= c.NODE_ERR_TOL
    assert rec["trace"] <= c.ADMIT_TRACE and max(rec["Rt"], rec["xyz"]) <= c.ADMIT_X * c.SCALE


def test_node_err_bound_is_the_recorded_spreads():
    assert c.NODE_ERR_TOL == max(1e-9, 100.0 * max(v["node_err"] for v in c.SPREADS.values()))
    assert set(c.SPREADS) == set(c.ITERATIVE)


@pytest.mark.parametrize("name", c.REJECTING)
def test_reject_scenes_reject_with_a_margin(name):
    e = c.yard(name)
    n = c.compared(e)
    d = e["decisions"][:n]
    assert d.count("reject") >= 3
    first = d.index("reject")
    assert "accept" in d[first:]                                            # an accept after a compared reject
    assert any(x == y == "reject" for x, y in zip(d, d[1:]))                 # a second solve on the stale linearisation
    assert e["report"][7] == 0 and "small" not in d


def test_reject_scenes_cover_huber_and_least_squares():
    assert any(np.isinf(c.case(n)["huber"]) for n in c.REJECT)
    below = 0
    for n in c.REJECT:
        k, e = c.case(n), c.yard(n)
        if np.isfinite(k["huber"]):
            pb = e["problem"]
            w0 = pb.linearise(pb.Rt0, pb.xyz_in[pb.tracks], k["huber"])["w"]
            w1 = pb.linearise(e["Rt"], e["xyz"][pb.tracks], k["huber"])["w"]
            print(n, "weights below 1: %d of %d at the start, %d at the end" % ((w0 < 1).sum(), len(w0), (w1 < 1).sum()))
            assert (w0 < 1.0).any() and (w1 == 1.0).any()           # both branches of the weight over the run
            below += 1
    assert below >= 1
    assert c.yard("reject_ls")["report"][2] == 2 and c.yard("reject_gauge")["report"][2] == 1
    assert c.case("reject_gauge")["fixed"].sum() == 1


def test_roles_are_present():
    k, e = c.case("reject_ls_roles"), c.yard("reject_ls_roles")
    pb = e["problem"]
    # frame 6: known, free, observed by nothing (the last free camera)
    assert pb.state[6] == pb.n_free - 1 == 4 and not (pb.ob_f == 6).any() and not (k["nodes"][:, 0] == 6).any()
    assert bits(e["Rt"][6]) == bits(k["Rt"][6])             # its block is lambda * 1e-6 with a zero right-hand side: no move
    # frame 7: unknown by its K
    assert pb.state[7] == ref.UNKNOWN and np.isnan(k["K"][7]).any() and np.isfinite(k["Rt"][7]).all()
    assert np.isnan(e["P"][7]).all() and bits(e["Rt"][7]) == bits(k["Rt"][7])
    t = k["t_unknown"]
    o = np.arange(k["off"][t], k["off"][t + 1])
    assert (k["nodes"][o, 0] == 7).sum() == 1 and len(o) == 4
    assert np.isnan(e["node_err"][o]).sum() == 1 and np.isnan(e["node_err"][o[-1]])
    j = int(np.flatnonzero(pb.tracks == t)[0])
    assert (pb.ob_t == j).sum() == 3
    # a track in the two fixed frames only: a point-only update, and the point does move
    t = k["t_fixed"]
    j = int(np.flatnonzero(pb.tracks == t)[0])
    assert (pb.ob_cf[pb.ob_t == j] == ref.FIXED).all() and (pb.ob_t == j).sum() == 2
    assert np.abs(e["xyz"][t] - k["X"][t]).max() > 0.1
    # a flagged track: no part, point unchanged, errors NaN
    t = k["t_flag"]
    assert k["flags"][t] != 0 and t not in pb.tracks and bits(e["xyz"][t]) == bits(k["X"][t])
    assert np.isnan(e["node_err"][k["off"][t]:k["off"][t + 1]]).all()
    assert e["report"][3:6].tolist() == [5, 199, 3 * 198 + 2]


def test_nonpd_then_solve():
    """non-PD verdicts by absorption, exact in any implementation, then solved attempts: see the case"""
    k, e = c.case("nonpd_then_solve"), c.yard("nonpd_then_solve")
    assert c.letters(e["decisions"]) == "nnnnaaa" and e["report"].tolist() == [7, 3, 1, 1, 13, 40, 0, 4]
    assert c.letters(c.yard("nonpd_then_solve", dense=True)["decisions"]) == "nnnnaaa"
    assert c.compared(e, nonpd=True) == 7 and c.compared(e) == 0
    pb = e["problem"]
    lin = pb.linearise(pb.Rt0, pb.xyz_in[pb.tracks], np.inf)
    m = pb.ob_t == 12
    assert m.sum() == 4 and (pb.ob_cf[m] == ref.FIXED).all() and (lin["r"][m] == 0.0).all()
    V = np.einsum("mki,mkj->ij", lin["Jp"][m], lin["Jp"][m])
    assert (V == 2.0**18 * np.array([[1, 0, -1], [0, 1, 0], [-1, 0, 1]])).all()
    for lam, pd in zip(e["trace"][:5, 1], (False, False, False, False, True)):
        d = np.diag(V) + lam * np.diag(V)
        assert (d == np.diag(V)).all() != pd                      # absorbed below 1.1e-16
        if pd:
            l00 = np.sqrt(d[0])
            assert d[2] - (V[0, 2] / l00) ** 2 >= 6 * np.spacing(2.0**18)     # the last pivot: 8 ulp in exact arithmetic
    assert bits(e["xyz"][12]) == bits(k["X"][12]) and (e["node_err"][-4:] == 0.0).all()
    assert e["trace"][5, 1] == 1e-12                                # the floor of lambda, by fmax


def test_nonpd_to_lambda_stop():
    k, e = c.case("nonpd_to_lambda_stop"), c.yard("nonpd_to_lambda_stop")
    assert (k["Rt"][0] == [1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0]).all() and k["fixed"][0] == 1
    assert k["X"][5, 2] == 0.0 and k["X"][5, 0] != 0.0 and k["X"][5, 1] != 0.0
    assert e["decisions"] == ["nonpd"] * 20 and np.isnan(e["trial"]).all()
    assert e["report"].tolist()[:3] == [20, 0, 4] and e["report"][7] == 20 and e["report"][6] >= 1 and e["report"][4] == 12
    lam = 1e-3
    for i in range(21):
        assert e["trace"][i, 0] == np.inf and e["trace"][i, 1] == lam
        lam *= 10.0
    assert e["trace"][19, 1] <= 1e16 < e["trace"][20, 1] and np.isnan(e["trace"][21:]).all()
    assert bits(e["Rt"]) == bits(k["Rt"]) and bits(e["xyz"]) == bits(k["X"])
    pb = e["problem"]
    with np.errstate(all="ignore"):
        lin = pb.linearise(pb.Rt0, pb.xyz_in[pb.tracks], np.inf)
    V = np.zeros((12, 3, 3))
    np.add.at(V, pb.ob_t, np.einsum("mki,mkj->mij", lin["Jp"], lin["Jp"]))
    assert np.isnan(V[5]).all() and np.isfinite(np.delete(V, 5, 0)).all()
    assert np.isinf(e["node_err"]).sum() == 1 and np.isfinite(e["node_err"]).sum() == 35


def test_lambda_stops():
    k, e = c.case("lambda_stop_at_start"), c.yard("lambda_stop_at_start")
    assert e["report"].tolist()[:3] == [0, 0, 4] and e["decisions"] == []
    assert e["trace"][0, 1] == 1e17 and e["trace"][0, 0] == c.yard("reject_ls")["trace"][0, 0] and np.isnan(e["trace"][1:]).all()
    assert bits(e["Rt"]) == bits(k["Rt"]) and bits(e["xyz"]) == bits(k["X"])
    # 1e16 is not > 1e16: one attempt, a step 1000 times below the small-step bound, not applied
    k, e = c.case("lambda0_1e16"), c.yard("lambda0_1e16")
    assert e["decisions"] == ["small"] and e["report"].tolist()[:3] == [1, 0, 3] and e["report"][7] == 0
    assert e["small_ratio"] <= 1e-3, e["small_ratio"]
    assert bits(e["trace"][1]) == bits(e["trace"][0]) and e["trace"][1, 1] == 1e16 and np.isnan(e["trace"][2:]).all()
    assert bits(e["Rt"]) == bits(k["Rt"]) and bits(e["xyz"]) == bits(k["X"])
    assert c.yard("reject_ls")["small_ratio"] is None


def test_zero_cost_start():
    k, e = c.case("zero_cost_start"), c.yard("zero_cost_start")
    assert e["trace"][0, 0] == 0.0 and e["report"].tolist() == [0, 0, 2, 2, 12, 36, 0, 0] and e["decisions"] == []
    assert (e["node_err"] == 0.0).all() and bits(e["Rt"]) == bits(k["Rt"]) and bits(e["xyz"]) == bits(k["X"])
    # exact in any order: dyadic K and t, R = I, z a power of two, integer keypoints
    z = k["X"][:, 2]
    assert set(z.tolist()) == {4.0, 8.0} and (k["X"][:, :2] * 32 == np.round(k["X"][:, :2] * 32)).all()
    assert (k["Rt"][:, 9:] * 4 == np.round(k["Rt"][:, 9:] * 4)).all()


def test_behind_at_iters_0():
    k, e = c.case("behind_at_iters_0"), c.yard("behind_at_iters_0")
    assert e["report"].tolist()[:3] == [0, 0, 1] and e["report"][6] >= 3 and e["report"][4] == 200
    pb = e["problem"]
    _, z, _, _ = pb.residuals(pb.Rt0, pb.xyz_in[pb.tracks])
    assert (np.abs(z) >= 0.5).all()                        # no depth near 0: the count does not hinge on rounding
    for t in k["behind"]:
        assert z[pb.ob_t == t].min() <= -1.0
    assert e["report"][6] == (z <= -0.5).sum()
    assert e["trace"].shape == (1, 2) and bits(e["Rt"]) == bits(k["Rt"]) and bits(e["xyz"]) == bits(k["X"])
