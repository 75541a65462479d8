"""GPU tests of the dense stage (pgx_gray_batch_dev, pgx_depth_maps_dev, pgx_depth_fuse_dev and the two host forms; k_depth.hip)
against tests/depth_ref.py: every integer output and every bit of d_depth equals the yardstick's, which is evaluated on the
device's own d_warp and d_planes; those two are held to the yardstick's at 1e-9 of their largest entry (they differ by the
rounding of a 3 x 3 adjugate at the most), and on the rotated rig to exact rationals within a derived bound, block by block
(ref.exact_warp), with the maps and the filter against the rendered truth.  The shapes are the smallest at which the kernels
can go wrong: the sweep's and the census' tiles and the filter's scan block and grid are read from the kernel source."""
import functools
import os
import re

import numpy as np
import pytest
import torch

import depth_ref as ref
import photogrammetry_amd as pg
from depth_gpu import BIG, DEV, dev, make_case, run_fuse, run_maps
from photogrammetry_amd import _lib

pytestmark = pytest.mark.gpu

SRC = open(os.path.join(_lib.CSRC, "k_depth.hip")).read()
CONST = {k: int(v) for k, v in re.findall(r"\b(DEP_NT|DEP_TW|DEP_TH|DEP_KC|CEN_TW|CEN_TH|FUSE_GRID_MAX) = (\d+)", SRC)}
TW, TH, NT, GRID = CONST["DEP_TW"], CONST["DEP_TH"], CONST["DEP_NT"], CONST["FUSE_GRID_MAX"]
MAP_KEYS = ("kq8", "depth", "cost", "flags", "warp", "planes", "summary")


def bits(a):
    return np.ascontiguousarray(a).view(np.uint8).tobytes()


def close_tables(got, exp):
    assert (np.isnan(got) == np.isnan(exp)).all()
    if np.isfinite(exp).any():
        assert np.nanmax(np.abs(got - exp)) <= 1e-9 * np.nanmax(np.abs(exp))


def check_maps(got, gray, P, views, ranges, D, a=2, min_views=1, max_cost=BIG, frame_ids=None, n_frames=None):
    nf = len(gray) if n_frames is None else n_frames
    e0 = ref.depth_maps(gray, frame_ids, nf, P, views, ranges, D, a, min_views, max_cost)
    close_tables(got["warp"], e0["warp"])
    close_tables(got["planes"], e0["planes"])
    e = ref.depth_maps(gray, frame_ids, nf, P, views, ranges, D, a, min_views, max_cost, warp=got["warp"], planes=got["planes"])
    for k in ("kq8", "flags", "summary"):
        assert (got[k] == e[k]).all(), (k, np.argwhere(got[k] != e[k])[:5])
    assert bits(got["depth"]) == bits(e["depth"])
    assert (got["cost"] == np.where(e["flags"] & ref.NOCAMERA, 77, e["cost"])).all()
    return e


def star_views(n, S):
    return np.array([[r] + [(r + 1 + j) % n for j in range(S)] for r in range(n)], dtype=np.int32)


def rot(axis, deg):
    c, s = np.cos(np.radians(deg)), np.sin(np.radians(deg))
    return {"y": np.array([[c, 0, s], [0, 1, 0], [-s, 0, c]]), "z": np.array([[c, -s, 0], [s, c, 0], [0, 0, 1.0]])}[axis]


def posed(Rm, C, W, H, f):
    K = np.array([[f, 0, W / 2], [0, f, H / 2], [0, 0, 1.0]])
    return (K @ np.hstack([Rm, -(Rm @ np.asarray(C, dtype=np.float64))[:, None]])).reshape(12)


# ---- the chain on the 96 x 64 scene ---------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def chain(engine):
    """grey from pgx_gray_batch_dev -> depth maps of five references -> the filter, everything left on the device between"""
    sc = ref.scene()
    W, H = ref.SCENE_W, ref.SCENE_H
    g16 = np.round(sc["gray"].astype(np.float64) * 65535.0).astype(np.uint16)
    rgba = np.stack([g16, g16, g16, np.full_like(g16, 65535)], -1)
    d_rgba = dev(rgba, np.uint16)
    d_gray = torch.zeros((5, H, W), dtype=torch.float32, device=DEV)
    torch.cuda.synchronize()
    engine.gray_batch_dev(d_rgba, 5, W, H, d_gray)
    engine.check_status()
    gray = d_gray.cpu().numpy()
    views, ranges = ref.all_views(), [sc["range"]] * 5
    got = run_maps(engine, gray, sc["P"], views, ranges, ref.SCENE_D, 2, 2, BIG)
    return sc, gray, views, ranges, got


def check_fuse(got, e, scale, cap=None):
    n = len(e["xyz"]) if cap is None else min(cap, len(e["xyz"]))
    assert (got["summary"] == e["summary"]).all(), (got["summary"], e["summary"])
    assert (got["agree"] == e["agree"]).all()
    assert (got["src"][:n] == e["src"][:n]).all()
    assert np.abs(got["xyz"][:n] - e["xyz"][:n]).max(initial=0) <= 1e-9 * scale
    assert (got["src"][n:] == 77).all() and (got["xyz"][n:] == 5.0).all()      # nothing behind the list


def test_chain_gray_depth_fuse(engine):
    sc, gray, views, ranges, got = chain(engine)
    assert np.abs(gray - sc["gray"]).max() <= 1.0 / 65535.0
    check_maps(got, gray, sc["P"], views, ranges, ref.SCENE_D, 2, 2, BIG)
    good = (got["flags"][0] == 0) & (np.abs(got["kq8"][0] / 256.0 - sc["ktrue"][0]) <= 1.0)
    assert good.mean() >= 0.95
    f = run_fuse(engine, got["depth"], views, sc["P"])
    e = ref.fuse(got["depth"], views, 5, sc["P"], 0.05, 2)
    check_fuse(f, e, 6.0)
    assert e["summary"][0] >= 0.9 * e["summary"][1] > 0


def test_offset_scene_gives_the_same_kq8(engine):
    sc, gray, views, ranges, got = chain(engine)
    T = np.array([2e4, -1e4, 3e4])
    P = np.stack([ref.scene_camera(np.array(C) + T).reshape(12) for C in ref.SCENE_CENTRES])
    moved = run_maps(engine, gray, P, views, ranges, ref.SCENE_D, 2, 2, BIG)
    assert (moved["kq8"] == got["kq8"]).all() and (moved["flags"] == got["flags"]).all()


def test_permuted_slots_give_the_same_bits(engine):
    sc, gray, views, ranges, got = chain(engine)
    perm = np.array([3, 0, 4, 1, 2])                      # slot s shows frame perm[s]; a sixth slot shows no frame
    g2 = np.concatenate([gray[perm], np.full_like(gray[:1], 0.25)])
    ids = np.concatenate([perm, [-1]])
    again = run_maps(engine, g2, sc["P"], views, ranges, ref.SCENE_D, 2, 2, BIG, frame_ids=ids, n_frames=5)
    for k in MAP_KEYS:
        assert bits(again[k]) == bits(got[k]), k


def test_two_runs_and_a_used_workspace_give_the_same_bits(engine):
    sc, gray, views, ranges, got = chain(engine)
    g, P = make_case(70, 41, 4, seed=5)
    run_maps(engine, g, P, star_views(4, 3), [(2.0, 6.0)] * 4, 19, 3)
    again = run_maps(engine, gray, sc["P"], views, ranges, ref.SCENE_D, 2, 2, BIG)
    for k in MAP_KEYS:
        assert bits(again[k]) == bits(got[k]), k
    f1, f2 = run_fuse(engine, got["depth"], views, sc["P"]), run_fuse(engine, got["depth"], views, sc["P"])
    for k in ("xyz", "src", "agree", "summary"):
        assert bits(f1[k]) == bits(f2[k]), k


def test_host_forms_give_the_same_bits(engine):
    sc, gray, views, ranges, got = chain(engine)
    h = engine.depth_maps(gray, sc["P"], views, ranges, D=ref.SCENE_D, agg_radius=2, min_views=2, max_cost=BIG)
    for k in ("kq8", "depth", "flags", "warp", "planes", "summary"):
        assert bits(h[k]) == bits(got[k]), k
    assert (h["cost"] == got["cost"]).all()
    f = run_fuse(engine, got["depth"], views, sc["P"])
    hf = engine.depth_fuse(got["depth"], views, sc["P"], 0.05, 2)
    n = int(f["summary"][0])
    assert len(hf["xyz"]) == n and bits(hf["xyz"]) == bits(f["xyz"][:n]) and bits(hf["src"]) == bits(f["src"][:n])
    assert bits(hf["agree"]) == bits(f["agree"]) and bits(hf["summary"]) == bits(f["summary"])
    # every optional output NULL, both forms; empty inputs
    h0 = engine.depth_maps(gray, sc["P"], views, ranges, D=ref.SCENE_D, min_views=2, cost=False, warp=False, planes=False)
    d0 = run_maps(engine, gray, sc["P"], views, ranges, ref.SCENE_D, 2, 2, BIG, optional=False)
    for k in ("kq8", "depth", "flags", "summary"):
        assert bits(h0[k]) == bits(got[k]) == bits(d0[k]), k
    assert (d0["cost"] == 77).all() and (d0["warp"] == 5.0).all() and (d0["planes"] == 5.0).all()
    assert bits(engine.depth_fuse(got["depth"], views, sc["P"], 0.05, 2, agree=False)["xyz"]) == bits(hf["xyz"])
    f0 = run_fuse(engine, got["depth"], views, sc["P"], agree=False)
    assert bits(f0["xyz"]) == bits(f["xyz"]) and (f0["agree"] == 77).all()
    empty = engine.depth_maps(gray, sc["P"], np.zeros((0, 5), np.int32), np.zeros((0, 2)), D=ref.SCENE_D)
    assert (empty["summary"] == 0).all() and empty["kq8"].shape[0] == 0
    ef = engine.depth_fuse(np.zeros((0, ref.SCENE_H, ref.SCENE_W)), np.zeros((0, 5), np.int32), sc["P"])
    assert (ef["summary"] == 0).all() and len(ef["xyz"]) == 0


# ---- shapes and parameters ------------------------------------------------------------------------------------------------

SHAPES = [(TW - 1, TH + 1), (TW, TH), (TW + 1, TH - 1), (2 * TW + 1, TH), (TW, 2 * TH + 1), (1, 1), (1, 9),
          (CONST["CEN_TW"] + 1, CONST["CEN_TH"] + 1)]


@pytest.mark.parametrize("W,H", SHAPES)
def test_frame_sizes_round_the_tiles(engine, W, H):
    gray, P = make_case(W, H, 3, seed=W * 100 + H)
    views, ranges = star_views(3, 2), [(2.0, 6.0), (2.5, 7.0), (1.5, 5.0)]
    got = run_maps(engine, gray, P, views, ranges, 9, 2)
    check_maps(got, gray, P, views, ranges, 9, 2)


@pytest.mark.parametrize("a", [0, 1, 2, 3])
def test_aggregation_radius(engine, a):
    gray, P = make_case(TW + 3, TH + 2, 3, seed=40 + a)
    views, ranges = star_views(3, 2), [(2.0, 6.0)] * 3
    got = run_maps(engine, gray, P, views, ranges, 2 * CONST["DEP_KC"] + 3, a)
    check_maps(got, gray, P, views, ranges, 2 * CONST["DEP_KC"] + 3, a)


@pytest.mark.parametrize("D", [3, 4, 255, 256])
def test_plane_counts(engine, D):
    gray, P = make_case(TW + 1, 9, 2, seed=D)
    views, ranges = np.array([[0, 1], [1, 0]], np.int32), [(2.0, 6.0)] * 2
    got = run_maps(engine, gray, P, views, ranges, D, 1)
    check_maps(got, gray, P, views, ranges, D, 1)


@pytest.mark.parametrize("S", [1, 4, 8])
def test_source_counts(engine, S):
    gray, P = make_case(TW + 2, TH + 1, 9, seed=60 + S)
    views, ranges = star_views(9, S)[:2], [(2.0, 6.0)] * 2
    got = run_maps(engine, gray, P, views, ranges, 6, 1, min_views=S)
    check_maps(got, gray, P, views, ranges, 6, 1, min_views=S)


def test_view_rows_with_gaps_repeats_and_the_reference_itself(engine):
    gray, P = make_case(21, 18, 3, seed=7)
    views = np.array([[0, 1, -1, 1], [1, 1, 0, 2], [2, -1, -1, -1]], np.int32)
    ranges = [(2.0, 6.0)] * 3
    got = run_maps(engine, gray, P, views, ranges, 7, 1)
    e = check_maps(got, gray, P, views, ranges, 7, 1)
    assert ((e["flags"][2] & ref.NOVIEWS) != 0).all() and np.isnan(got["warp"][2]).all()


def test_sources_that_see_nothing_lie_behind_or_are_turned(engine):
    W, H, f = 24, 20, 30.0
    rng = np.random.default_rng(11)
    gray = rng.random((4, H, W)).astype(np.float32)
    P = np.stack([posed(np.eye(3), (0, 0, 0), W, H, f), posed(np.eye(3), (100.0, 0, 0), W, H, f),
                  posed(rot("y", 180.0), (0.1, 0, 0), W, H, f), posed(rot("z", 90.0), (0.1, 0.05, 0), W, H, f)])
    views, ranges = np.array([[0, 1, 2, 3], [3, 0, 1, 2]], np.int32), [(2.0, 6.0)] * 2
    got = run_maps(engine, gray, P, views, ranges, 8, 1)
    e = ref.depth_maps(gray, None, 4, P, views, ranges, 8, 1, 1, BIG, warp=got["warp"], planes=got["planes"], volumes=True)
    check_maps(got, gray, P, views, ranges, 8, 1)
    raw, nval, agg = e["volumes"][0]
    assert nval.max() == 1 and nval[:, H // 2, W // 2].min() == 1      # only the turned source sees the reference


@pytest.mark.parametrize("min_views", [2, 3])
def test_min_views_at_and_above_the_valid_sources(engine, min_views):
    gray, P = make_case(20, 17, 3, seed=13)
    views, ranges = np.array([[0, 1, -1, 2]], np.int32), [(2.0, 6.0)]
    got = run_maps(engine, gray, P, views, ranges, 8, 1, min_views=min_views)
    e = check_maps(got, gray, P, views, ranges, 8, 1, min_views=min_views)
    if min_views == 3:
        assert ((e["flags"] & ref.NOVIEWS) != 0).all()
    else:
        assert ((e["flags"] & ref.NOVIEWS) == 0).any()


def test_max_cost_at_and_below_a_best_cost(engine):
    gray, P = make_case(20, 17, 3, seed=17)
    views, ranges = star_views(3, 2)[:1], [(2.0, 6.0)]
    free = run_maps(engine, gray, P, views, ranges, 8, 1)
    y, x = np.argwhere(free["flags"][0] == 0)[0]
    c = int(free["cost"][0, y, x])
    for mc, flagged in ((c, False), (c - 1, True)):
        got = run_maps(engine, gray, P, views, ranges, 8, 1, max_cost=mc)
        check_maps(got, gray, P, views, ranges, 8, 1, max_cost=mc)
        assert bool(got["flags"][0, y, x] & ref.HIGHCOST) == flagged


def test_nan_and_inf_inputs(engine):
    gray, P = make_case(22, 19, 4, seed=19)
    gray[0, 3, 4], gray[1, 10, 10], gray[2, 0, 0], gray[0, 18, 21] = np.nan, np.inf, -np.inf, np.nan
    P[3, 5] = np.nan
    views = np.array([[0, 1, 3], [3, 0, 1], [1, 2, 0], [2, 0, 1]], np.int32)
    ranges = [(2.0, 6.0), (2.0, 6.0), (6.0, 6.0), (7.0, 2.0)]
    got = run_maps(engine, gray, P, views, ranges, 8, 1)
    e = check_maps(got, gray, P, views, ranges, 8, 1)
    assert (e["flags"][1:] == ref.NOCAMERA).all() and e["summary"][6] == 3 and np.isnan(got["planes"][1:]).all()
    assert np.isnan(got["warp"][0, 1]).all() and np.isfinite(got["warp"][0, 0]).all()


def test_frames_without_a_slot(engine):
    gray, P = make_case(20, 17, 5, seed=23)
    ids = np.array([3, 0, 1], np.int32)                      # frames 2 and 4 have no slot
    views, ranges = np.array([[0, 1, 4], [2, 0, 1], [3, 2, 0]], np.int32), [(2.0, 6.0)] * 3
    got = run_maps(engine, gray[ids], P, views, ranges, 8, 1, frame_ids=ids, n_frames=5)
    e = check_maps(got, gray[ids], P, views, ranges, 8, 1, frame_ids=ids, n_frames=5)
    assert (e["flags"][1] == ref.NOCAMERA).all() and np.isnan(got["warp"][0, 1]).all() and np.isnan(got["warp"][2, 0]).all()


def test_bad_arguments_are_refused_at_once(engine):
    gray, P = make_case(8, 8, 2, seed=1)
    views, ranges = np.array([[0, 1]], np.int32), [(2.0, 6.0)]
    for kw in (dict(D=2), dict(D=257), dict(a=4), dict(a=-1), dict(min_views=0), dict(min_views=2), dict(max_cost=-1)):
        args = dict(D=8, a=1, min_views=1, max_cost=BIG)
        args.update(kw)
        with pytest.raises(pg.ArgumentException):
            run_maps(engine, gray, P, views, ranges, args["D"], args["a"], args["min_views"], args["max_cost"])
    with pytest.raises(pg.ArgumentException):
        run_maps(engine, gray, P, np.zeros((1, 10), np.int32), ranges, 8)          # S = 9


# ---- the filter -----------------------------------------------------------------------------------------------------------

def test_fuse_capacity(engine):
    sc, gray, views, ranges, got = chain(engine)
    e = ref.fuse(got["depth"], views, 5, sc["P"], 0.05, 2)
    n = len(e["xyz"])
    for cap in (n - 1, n, n + 1):
        f = run_fuse(engine, got["depth"], views, sc["P"], max_points=cap, check=False)
        assert (f["err"] is not None) == (cap < n)
        check_fuse(f, e, 6.0, cap)
    engine.check_status()                                      # the status word was cleared


@pytest.mark.parametrize("rel_tol,min_agree", [(0.05, 0), (0.05, 5), (0.0, 1)])
def test_fuse_thresholds(engine, rel_tol, min_agree):
    sc, gray, views, ranges, got = chain(engine)
    f = run_fuse(engine, got["depth"], views, sc["P"], rel_tol=rel_tol, min_agree=min_agree)
    e = ref.fuse(got["depth"], views, 5, sc["P"], rel_tol, min_agree)
    check_fuse(f, e, 6.0)
    assert e["summary"][0] == {0: e["summary"][1], 5: 0}.get(min_agree, e["summary"][0])


def test_fuse_one_map_and_a_frame_named_twice(engine):
    sc, gray, views, ranges, got = chain(engine)
    for rows, ma in (([0], 0), ([0], 1), ([0, 1, 0, 2], 1)):
        d, v = got["depth"][rows], views[rows]
        f = run_fuse(engine, d, v, sc["P"], min_agree=ma)
        e = ref.fuse(d, v, 5, sc["P"], 0.05, ma)
        check_fuse(f, e, 6.0)
    assert e["summary"][0] > 0
    # a map with an unknown camera and one whose frame is no frame number are skipped
    P = sc["P"].copy()
    P[1, 0] = np.inf
    v = views.copy()
    v[2, 0] = 9
    f = run_fuse(engine, got["depth"], v, P)
    e = ref.fuse(got["depth"], v, 5, P, 0.05, 2)
    check_fuse(f, e, 6.0)
    assert e["summary"][3] == 2


def test_fuse_compaction_past_a_scan_block_and_a_grid_pass(engine):
    W, H, R = 256, 208, 5
    assert R * W * H > GRID * NT and (R * W * H + NT - 1) // NT > NT       # a second grid pass; a second chunk of block sums
    rng = np.random.default_rng(3)
    P = np.stack([ref.scene_camera(C, W, H, 300.0).reshape(12) for C in ref.SCENE_CENTRES])
    depth = 4.0 + 0.05 * rng.standard_normal((R, H, W))
    depth[rng.random((R, H, W)) < 0.3] = np.nan
    views = ref.all_views()
    f = run_fuse(engine, depth, views, P, rel_tol=0.01, min_agree=2)
    e = ref.fuse(depth, views, 5, P, 0.01, 2)
    check_fuse(f, e, 6.0)
    assert NT < e["summary"][0] < e["summary"][1]


def test_fuse_inputs_that_are_finite_but_no_depths(engine):
    """0.0, negative and infinite entries among the rendered depths of the rotated rig, as the pixel's own z (0 and negatives
    count as depths: the rule asks for finite only) and as the z_j a valid pixel projects onto."""
    sc = ref.scene_rotated()
    rng = np.random.default_rng(31)
    depth = sc["ztrue"].copy()
    bad = np.array([0.0, -0.0, -3.5, -1e-300, np.inf, -np.inf])
    pick = rng.random(depth.shape) < 0.25
    depth[pick] = rng.choice(bad, pick.sum())
    # pixels of map 1 that keep their depth and see map 2 where it holds such a value: every kind occurs as a z_j
    P2 = sc["P"][2].reshape(3, 4)
    q = sc["X"][1] @ P2[:, :3].T + P2[:, 3]
    ok, iu, iv = ref.pixel(q[..., 0], q[..., 1], q[..., 2], ref.SCENE_W, ref.SCENE_H)
    zj = depth[2][iv, iu][ok & ~pick[1]]
    assert all((zj == b).any() for b in bad) and (np.signbit(zj) & (zj == 0)).any()
    for views, ma in ((ref.all_views(), 1), (ref.ROT_VIEWS, 0)):
        f = run_fuse(engine, depth, views, sc["P"], rel_tol=0.05, min_agree=ma)
        e = ref.fuse(depth, views, 5, sc["P"], 0.05, ma)
        check_fuse(f, e, 6.0)
        assert 0 < e["summary"][0] and e["summary"][1] == np.isfinite(depth).sum() < depth.size
    assert e["summary"][0] == e["summary"][1]                  # min_agree 0 keeps 0.0 and the negatives too


def fuse_refused(engine, R=2, S=1, W=8, H=8, rel_tol=0.05, min_agree=1, max_points=16, alloc=None):
    """pgx_depth_fuse_dev with these arguments over sentinel-filled buffers of size alloc = (R, W, H): refused, nothing written"""
    aR, aW, aH = alloc or (R, W, H)
    i32 = dict(dtype=torch.int32, device=DEV)
    dd = torch.full((aR, aH, aW), 4.0, dtype=torch.float64, device=DEV)
    dv, dP = torch.zeros((aR, 1 + S), **i32), torch.zeros((2, 12), dtype=torch.float64, device=DEV)
    xyz, src = torch.full((16, 3), 5.0, dtype=torch.float64, device=DEV), torch.full((16, 2), 77, **i32)
    ag, summary = torch.full((aR, aH, aW), 77, **i32), torch.full((4,), 77, **i32)
    torch.cuda.synchronize()
    with pytest.raises(pg.ArgumentException):
        engine.depth_fuse_dev(dd, dv, R, S, W, H, 2, dP, max_points, xyz, src, summary, rel_tol=rel_tol, min_agree=min_agree, d_agree=ag)
    torch.cuda.synchronize()
    engine.check_status()
    assert (xyz == 5.0).all() and (src == 77).all() and (ag == 77).all() and (summary == 77).all()


@pytest.mark.parametrize("kw", [dict(S=0), dict(S=9), dict(rel_tol=-1e-300), dict(rel_tol=float("nan")), dict(rel_tol=float("inf")),
                                dict(rel_tol=float("-inf")), dict(min_agree=-1), dict(max_points=-1), dict(R=65536, W=1, H=1),
                                dict(R=1, W=32768, H=32769, alloc=(1, 8, 8))], ids=lambda kw: ",".join("%s=%s" % i for i in kw.items()))
def test_fuse_refusals(engine, kw):
    """fuse_args checks everything before the workspace is sized and a kernel launched, so the call over 2^30 pixels returns
    without touching its (small) buffers."""
    fuse_refused(engine, **kw)


def maps_refused(engine, F=2, W=8, H=8, R=1, S=1, n_frames=None, alloc=None):
    """pgx_depth_maps_dev with these sizes over sentinel-filled buffers of size alloc = (F, W, H, R): refused, nothing written"""
    aF, aW, aH, aR = alloc or (F, W, H, R)
    nf = F if n_frames is None else n_frames
    i32 = dict(dtype=torch.int32, device=DEV)
    f64 = dict(dtype=torch.float64, device=DEV)
    dg, dP = torch.zeros((aF, aH, aW), dtype=torch.float32, device=DEV), torch.zeros((max(nf, aF), 12), **f64)
    dv, dr = torch.zeros((aR, 1 + S), **i32), torch.ones((aR, 2), **f64)
    out = [torch.full((aR, aH, aW), 77, **i32) for _ in range(3)] + [torch.full((8,), 77, **i32)]
    dep, warp, planes = torch.full((aR, aH, aW), 5.0, **f64), torch.full((aR, S, 12), 5.0, **f64), torch.full((aR, 8), 5.0, **f64)
    torch.cuda.synchronize()
    with pytest.raises(pg.ArgumentException):
        engine.depth_maps_dev(dg, F, W, H, nf, dP, dv, R, S, dr, 8, out[0], dep, out[1], out[3], agg_radius=1, min_views=1,
                              max_cost=BIG, d_cost=out[2], d_warp=warp, d_planes=planes)
    torch.cuda.synchronize()
    engine.check_status()
    assert all((o == 77).all() for o in out) and all((o == 5.0).all() for o in (dep, warp, planes))


@pytest.mark.parametrize("kw", [dict(R=65536, W=1, H=1), dict(F=65536, W=1, H=1), dict(F=1, R=1, W=32768, H=32769, alloc=(1, 8, 8, 1)),
                                dict(F=1, R=3, W=32768, H=16384, alloc=(1, 8, 8, 3)), dict(F=3, R=1, W=16384, H=32768, alloc=(3, 8, 8, 1)),
                                dict(n_frames=3), dict(n_frames=1)], ids=lambda kw: ",".join("%s=%s" % i for i in kw.items()))
def test_maps_refusals(engine, kw):
    """depth_args checks everything before the workspace is sized and a kernel launched: R and F one above their limit at
    1 x 1, max(F, R) W H above 2^30 through R, through F and by one row, n_frames on either side of F without ids."""
    maps_refused(engine, **kw)


# ---- general cameras: rotated, rolled, skewed, scaled, mirrored --------------------------------------------------------

ROT_FLOOR = 0.81       # tests/test_depth_ref.py: 0.05 below the yardstick's lowest fraction of references 1 to 4, rounded down


@functools.lru_cache(maxsize=None)
def rotated(engine):
    """ref.scene_rotated() and the device's maps of it at scale 1 over ROT_VIEWS"""
    sc = ref.scene_rotated()
    ranges = [sc["range"]] * 5
    return sc, ranges, run_maps(engine, sc["gray"], sc["P"], ref.ROT_VIEWS, ranges, ref.SCENE_D, 2, 2, BIG)


def test_rotated_rig_with_mixed_scales(engine):
    """Cameras lam K [R | -R C] at scales (-2.5, 1, 1e-3, 40, 0.3): the integers and depth bits against the yardstick on the
    device's tables, the tables per (r, s) block against exact rationals within the forward bound of rule 3 in float64, the
    planes within 4 u of the exact scale, the maps against the rendered truth.  Measured on an MI355X: the worst warp entry at
    0.0991 of its bound, the worst plane at 1.982 u, which are the yardstick's figures; within one plane 0.9645, 0.8742,
    0.8296, 0.8571, 0.8812 of the five references' pixels (ROT_VIEWS keep the negated frame 0 out of the other rows)."""
    sc, ranges, _ = rotated(engine)
    P = ref.scaled_cameras(sc["P"], ref.ROT_SCALES)
    got = run_maps(engine, sc["gray"], P, ref.ROT_VIEWS, ranges, ref.SCENE_D, 2, 2, BIG)
    check_maps(got, sc["gray"], P, ref.ROT_VIEWS, ranges, ref.SCENE_D, 2, 2, BIG)
    w, p = ref.plan_against_exact(P, ref.ROT_VIEWS, ranges, ref.SCENE_D, got["warp"], got["planes"])
    frac = ref.within_one_plane(got["kq8"], got["flags"], sc["ktrue"])
    print("device: worst warp error %.4f of its bound, worst plane error %.3f u; within one plane %s" % (w, p, np.round(frac, 4)))
    assert w <= 1.0 and p <= 4.0
    assert (got["planes"][0] < 0).all() and (got["planes"][1:] > 0).all()
    assert frac[0] >= 0.95 and (frac[1:] >= ROT_FLOOR).all()


def test_power_of_two_scales_change_no_bit(engine):
    sc, ranges, plain = rotated(engine)
    check_maps(plain, sc["gray"], sc["P"], ref.ROT_VIEWS, ranges, ref.SCENE_D, 2, 2, BIG)
    P = ref.scaled_cameras(sc["P"], ref.ROT_SCALES_POW2)
    got = run_maps(engine, sc["gray"], P, ref.ROT_VIEWS, ranges, ref.SCENE_D, 2, 2, BIG)
    ref.assert_scaled_tables(plain, got, ref.ROT_VIEWS, ref.ROT_SCALES_POW2)
    assert (got["planes"][0] == -4.0 * plain["planes"][0]).all()
    for k in ("kq8", "flags", "cost", "depth", "summary"):
        assert bits(got[k]) == bits(plain[k]), k
    assert plain["summary"][1] > 0.8 * plain["summary"][0]
    f1, f2 = (run_fuse(engine, plain["depth"], ref.ROT_VIEWS, p) for p in (sc["P"], P))
    check_fuse(f1, ref.fuse(plain["depth"], ref.ROT_VIEWS, 5, sc["P"], 0.05, 2), 6.0)
    for k in ("xyz", "src", "agree", "summary"):
        assert bits(f1[k]) == bits(f2[k]), k
    assert f1["summary"][0] > 0.8 * f1["summary"][1] > 0


def test_a_negated_source_is_an_absent_source(engine):
    """-P is the same camera with det M < 0: q_2 < 0 for every point in front of it, so rule 4 passes over it as a source, in
    both calls, while its warp is finite.  As a reference it still gives its own points, bit for bit."""
    sc, ranges, _ = rotated(engine)
    P = sc["P"].copy()
    P[4] = -P[4]
    views = ref.ROT_VIEWS[:4]                                    # frame 4 is a source of every row and the reference of none
    absent = np.where(views == 4, -1, views)
    got = run_maps(engine, sc["gray"], P, views, ranges[:4], ref.SCENE_D, 2, 2, BIG)
    exp = run_maps(engine, sc["gray"], sc["P"], absent, ranges[:4], ref.SCENE_D, 2, 2, BIG)
    check_maps(got, sc["gray"], P, views, ranges[:4], ref.SCENE_D, 2, 2, BIG)
    for k in ("kq8", "flags", "cost", "depth", "summary"):
        assert bits(got[k]) == bits(exp[k]), k
    at = views[:, 1:] == 4
    assert at.sum() == 4 and np.isfinite(got["warp"][at]).all() and np.isnan(exp["warp"][at]).all()
    assert np.isfinite(got["warp"][views[:, 1:] >= 0]).all() and np.isnan(got["warp"][views[:, 1:] < 0]).all()
    assert got["summary"][1] > 0
    # the filter: frame 4 named by no row (passed over either way), then as the reference of a row of its own
    for v in (views, ref.ROT_VIEWS):
        gone = np.c_[v[:, 0], np.where(v[:, 1:] == 4, -1, v[:, 1:])]
        f = run_fuse(engine, sc["ztrue"][:len(v)], v, P, min_agree=1)
        e = run_fuse(engine, sc["ztrue"][:len(v)], gone, sc["P"], min_agree=1)
        check_fuse(f, ref.fuse(sc["ztrue"][:len(v)], v, 5, P, 0.05, 1), 6.0)
        for k in ("xyz", "src", "agree", "summary"):
            assert bits(f[k]) == bits(e[k]), k
        assert f["summary"][0] > 0
    assert (f["src"][:f["summary"][0], 0] == 4).any()


@pytest.mark.parametrize("scales", [(1.0,) * 5, ref.ROT_SCALES_POW2], ids=["scale1", "pow2"])
def test_fuse_at_the_true_depths_of_the_rotated_rig(engine, scales):
    """The filter fed the rendered depths: every kept point is the rendered X of its pixel, one agreeing view at 5 % keeps at
    least 0.95 of the pixels (the yardstick: 29249 of 30720), and powers of two change no bit."""
    sc = ref.scene_rotated()
    f = run_fuse(engine, sc["ztrue"], ref.ROT_VIEWS, ref.scaled_cameras(sc["P"], scales), min_agree=1)
    e = ref.fuse(sc["ztrue"], ref.ROT_VIEWS, 5, sc["P"], 0.05, 1)
    check_fuse(f, e, 6.0)
    n = int(f["summary"][0])
    X = sc["X"].reshape(5, -1, 3)[f["src"][:n, 0], f["src"][:n, 1]]
    print("kept %d of %d, worst |xyz - X| %.2e" % (n, f["summary"][1], np.abs(f["xyz"][:n] - X).max()))
    assert np.abs(f["xyz"][:n] - X).max() <= 1e-9 * 6.0
    assert f["summary"][1] == sc["ztrue"].size and n >= 0.95 * f["summary"][1]
    if scales[0] != 1.0:
        plain = run_fuse(engine, sc["ztrue"], ref.ROT_VIEWS, sc["P"], min_agree=1)
        for k in ("xyz", "src", "agree", "summary"):
            assert bits(f[k]) == bits(plain[k]), k


def test_saturated_costs(engine):
    """The 9-bit raw field of the sweep at the most it can be asked to hold, 8 x 62 = 496 with nvalid = 8 above it, and the
    7 x 7 box of it, 24304: at exactly the yardstick's 702 pixels; all planes tie, so k* = 0 and EDGE everywhere; max_cost at
    and one below."""
    gray, P, views, ranges, kw = ref.saturated_case()
    runs = {}
    for mc in (BIG, 24304, 24303):
        got = run_maps(engine, gray, P, views, ranges, kw["D"], kw["a"], kw["min_views"], mc)
        e = check_maps(got, gray, P, views, ranges, kw["D"], kw["a"], kw["min_views"], mc)
        runs[mc] = got
        assert (got["cost"] == e["cost"]).all() and got["cost"].max() == 49 * 496 == 24304
        assert ((got["cost"] == 24304) == (e["cost"] == 24304)).all() and (got["cost"] == 24304).sum() == 702
        assert ((got["flags"] & ~ref.HIGHCOST) == ref.EDGE).all() and (got["kq8"] == -1).all()
    assert (runs[BIG]["flags"] == ref.EDGE).all() and (runs[24304]["flags"] == ref.EDGE).all()
    assert ((runs[24303]["flags"] & ref.HIGHCOST) != 0).sum() == 702
    assert (((runs[24303]["flags"] & ref.HIGHCOST) != 0) == (runs[BIG]["cost"] == 24304)).all()


# ---- grey images ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("fmt", [_lib.PGX_SRC_RGBA64, _lib.PGX_SRC_RGBA8])
@pytest.mark.parametrize("with_map", [False, True])
def test_gray_batch_equals_gray_per_frame(fmt, with_map):
    W, H, F = 37, 23, 3
    rng = np.random.default_rng(29)
    dt = np.uint8 if fmt == _lib.PGX_SRC_RGBA8 else np.uint16
    frames = rng.integers(0, np.iinfo(dt).max + 1, (F, H, W, 4)).astype(dt)
    eng = pg.Engine(0)
    try:
        eng.set_source_format(fmt)
        if with_map:
            eng.set_dewarp_map(np.stack([rng.integers(0, W, (H, W)), rng.integers(0, H, (H, W))], -1))   # any source pixel
        d_gray = torch.full((F, H, W), 5.0, dtype=torch.float32, device=DEV)
        d_rgba = torch.from_numpy(frames).to(DEV)
        torch.cuda.synchronize()
        eng.gray_batch_dev(d_rgba, F, W, H, d_gray)
        eng.check_status()
        got = d_gray.cpu().numpy()
        for i in range(F):
            if with_map:
                dw = eng.dewarp(frames[i])                    # 16-bit whatever the source format
                eng.set_source_format(_lib.PGX_SRC_RGBA64)
                want = eng.gray(dw)
                eng.set_source_format(fmt)
            else:
                want = eng.gray(frames[i])
            assert bits(got[i]) == bits(want), i
    finally:
        eng.close()
