"""GPU tests of bundle adjustment (pgx_bundle_adjust_dev / pgx_bundle_adjust; include/pgx.h) past its first rejected step and
at every stop: the control flow around the step, which tests/test_gpu_bundle.py leaves to scenes that reject only at the
rounding floor.  The scenes and the rule that admits them are tests/bundle_paths_cases.py's; tests/test_bundle_paths_cases.py
shows on the yardstick alone that each reaches its path.  On a rejection the device skips the linearisation, solves again on
the stale node data with lambda * 10, keeps `sel` and overwrites the trial halves of its buffers: held here decision for
decision, with the lambda column bit for bit, against tests/bundle_ref.py."""
import numpy as np
import pytest

import bundle_paths_cases as c
import geom_gpu as g
from geom_gpu import ba_run, bits, device_problem

pytestmark = pytest.mark.gpu


def run(engine, name, d=None, **kw):
    k = c.case(name)
    d = d or device_problem(k["kps"], k["off"], k["nodes"])
    return ba_run(engine, d, k["K"], k["Rt"], k["fixed"], k["X"], iters=k["max_iters"], huber=k["huber"], lam0=k["lambda0"],
                  flags=k["flags"], **kw)


@pytest.mark.parametrize("name", c.ITERATIVE + ("reject_ls_100",))
def test_rejected_steps_against_yardstick(engine, name):
    got, e = run(engine, name), c.yard(name)
    dg, de, n = g.ba_check_paths(got, e, c.SCALE, nonpd_compared=c.case(name).get("nonpd_compared", False))
    print(name, "compared", n, "gpu", c.letters(dg), got["report"].tolist(), "yardstick", c.letters(de), e["report"].tolist())
    assert de[:n].count("reject") >= 3 and n == c.SPREADS.get(name, c.SPREADS["reject_ls"])["compared"]
    assert got["trace"].shape == (c.case(name)["max_iters"] + 1, 2)


def test_reject_ls_identical_bits_across_runs_capacity_slots_and_host_form(engine):
    k = c.case("reject_ls")
    a = run(engine, "reject_ls")
    assert "reject" in g.decisions(a["trace"], a["report"])
    g.same_bits(a, run(engine, "reject_ls"), g.BA_KEYS)
    g.same_bits(a, run(engine, "reject_ls", max_tracks=len(k["off"]) - 1 + 777), g.BA_KEYS)
    slots = np.random.default_rng(0).permutation(6 + 3)[:6]
    g.same_bits(a, run(engine, "reject_ls", d=device_problem(k["kps"], k["off"], k["nodes"], slots=slots, n_slots=9)), g.BA_KEYS)
    h = engine.bundle_adjust(k["kps"], k["K"], k["Rt"], k["fixed"], k["off"], k["nodes"], k["X"], max_iters=k["max_iters"],
                             huber_px=k["huber"], lambda0=k["lambda0"])
    g.same_bits(a, h, g.BA_KEYS)


@pytest.mark.parametrize("name", c.STOPS)
def test_stops_against_yardstick(engine, name):
    k, e = c.case(name), c.yard(name)
    got = run(engine, name)                 # checks the status: the NaN block and the +inf cost must leave no bit
    engine.check_status()
    print(name, got["report"].tolist(), e["report"].tolist(), got["trace"][:int(got["report"][0]) + 1].tolist())
    assert got["report"].tolist() == e["report"].tolist()
    tg, te = got["trace"], e["trace"]
    assert tg.shape == te.shape
    assert (np.isnan(tg) == np.isnan(te)).all() and (np.isinf(tg) == np.isinf(te)).all()
    fin = np.isfinite(te[:, 0])
    assert (tg[np.isinf(te)] == te[np.isinf(te)]).all()
    assert np.allclose(tg[fin, 0], te[fin, 0], rtol=c.TRACE_TOL, atol=0)
    assert bits(tg[:, 1]) == bits(te[:, 1])
    assert g.decisions(tg, got["report"]) == g.yard_decisions(e)
    # nothing moved
    assert bits(e["Rt"]) == bits(k["Rt"]) and bits(e["xyz"]) == bits(k["X"])
    assert bits(got["Rt"]) == bits(k["Rt"]) and bits(got["xyz"]) == bits(k["X"])
    pb = e["problem"]
    assert bits(got["P"]) == bits(g.ba_camera_rows(pb.K, got["Rt"], pb.state)) == bits(e["P"])
    ng, ne = got["node_err"], e["node_err"]
    assert (np.isnan(ng) == np.isnan(ne)).all() and (np.isinf(ng) == np.isinf(ne)).all()
    fin = np.isfinite(ne)
    assert np.abs(ng[fin] - ne[fin]).max() <= c.NODE_ERR_TOL
    if name == "zero_cost_start":
        assert tg[0, 0] == 0.0 and (ng == 0.0).all()
