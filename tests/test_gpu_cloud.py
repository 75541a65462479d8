"""GPU tests of the cloud merge (pgx_rgba8_batch_dev, pgx_cloud_merge_dev and the two host forms; k_image.hip, k_cloud.hip)
against tests/cloud_ref.py: every integer output and every bit of the float outputs equals the yardstick's.  The shapes are the
smallest at which the kernels can go wrong: the scan block, the grid, the table's size and the hash are read or restated from
the kernel source (cloud_ref.kernel_constants, table_hash)."""
import functools

import numpy as np
import pytest
import torch

import cloud_ref as ref
import depth_ref
import photogrammetry_amd as pg
from cloud_gpu import CELL, DEV, ORIGIN, dev, rig, run_merge, synth
from photogrammetry_amd import _lib

pytestmark = pytest.mark.gpu

BIG = 2**30
K = ref.kernel_constants(_lib.CSRC)
NT, GRID = K["CLD_NT"], K["CLD_GRID_MAX"]
OUT_KEYS = ("xyz", "normal", "rgba8", "info")
bits = ref.bits


def check_merge(got, e, cap=None, n=None):
    """the device's outputs against the yardstick's: the first min(kept, cap) rows, nothing behind them, the per-point rows < n"""
    kept = len(e["xyz"])
    m = kept if cap is None else min(cap, kept)
    assert (got["report"] == e["report"]).all(), (got["report"], e["report"])
    n = int(e["report"][0]) if n is None else n
    assert (got["pt_normal"][:n] == e["pt_normal"]).all(), np.argwhere(got["pt_normal"][:n] != e["pt_normal"])[:5]
    assert (got["cell_of"][:n] == e["cell_of"]).all(), np.argwhere(got["cell_of"][:n] != e["cell_of"])[:5]
    assert (got["pt_normal"][n:] == 77).all() and (got["cell_of"][n:] == 77).all()
    assert (got["info"][:m] == e["info"][:m]).all(), np.argwhere(got["info"][:m] != e["info"][:m])[:5]
    assert (got["rgba8"][:m] == e["rgba8"][:m]).all()
    assert bits(got["xyz"][:m]) == bits(e["xyz"][:m]), np.argwhere(got["xyz"][:m] != e["xyz"][:m])[:5]
    assert bits(got["normal"][:m]) == bits(e["normal"][:m]), np.argwhere(got["normal"][:m] != e["normal"][:m])[:5]
    assert (got["xyz"][m:] == 5.0).all() and (got["normal"][m:] == 5.0).all() and (got["rgba8"][m:] == 77).all() and (got["info"][m:] == 77).all()


def run_and_check(engine, c, **kw):
    """the device and the yardstick on case c (xyz, src, depth, views, P, rgba8 and frame_ids or absent), compared"""
    col, ids = c.get("rgba8"), c.get("frame_ids")
    got = run_merge(engine, c["xyz"], c["src"], c["depth"], c["views"], c["P"], rgba8=col, frame_ids=ids, **kw)
    ekw = {k: v for k, v in kw.items() if k in ("k", "disc_tol", "min_support", "count")}
    e = ref.merge(c["xyz"], c["src"], c["depth"], c["views"], len(np.reshape(c["P"], (-1, 12))), c["P"], CELL, ORIGIN, rgba8=col,
                  frame_ids=ids, **ekw)
    check_merge(got, e, kw.get("max_points"))
    return got, e


# ---- counts and cells -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", [0, 1, NT - 1, NT, NT + 1, NT * NT + 1, (GRID + 16) * NT])
def test_list_lengths_round_the_scan_block_and_the_grid(engine, n):
    """0, 1 and the scan block's 255, 256, 257 points; 65 537 = more than 256 block counts (a second chunk of the scan); 266 240 =
    more than one pass of the 1024-workgroup grid.  About four points per cell."""
    assert NT * NT + 1 == 65537 and (GRID + 16) * NT == 266240
    c = synth(n + 3, seed=n, spread=CELL * max(2.0, (n / 4.0) ** (1.0 / 3.0)))
    got, e = run_and_check(engine, c, count=n)
    assert e["report"][0] == n and (n < 10 or e["report"][6] < n)


def test_seventy_thousand_points_in_one_cell(engine):
    c = synth(70000, seed=3, spread=CELL / 4)
    c["xyz"] += CELL / 2
    got, e = run_and_check(engine, c)
    assert e["report"][5] == 1 and e["info"][0, 0] == 70000 and e["info"][0, 3] == 0


def test_every_point_in_its_own_cell(engine):
    c = synth(3000, seed=4)
    g = np.arange(3000)
    c["xyz"] = np.array(ORIGIN) + (np.stack([g % 17, g // 17 % 13, g // 221], 1) + 0.37) * CELL
    got, e = run_and_check(engine, c)
    assert e["report"][5] == e["report"][6] == 3000 and (e["info"][:, 0] == 1).all()


def colliding_keys(max_in, runs, tail):
    """cells (5, -3, g2) found by search whose first probe is the same table entry, in runs of the given lengths, and `tail` cells
    whose first probe is one of the table's last two entries (their chain wraps past the end)"""
    lg = ref.table_lg(max_in, K)
    T = 1 << lg
    g2 = np.arange(-200000, 200000)
    keys = np.array([ref.key_of((5, -3, 0))], dtype=np.uint64) + g2.astype(np.int64).astype(np.uint64)
    h = (keys * np.uint64(K["CLD_HASH_MUL"])) >> np.uint64(64 - lg)           # uint64 products wrap modulo 2^64
    assert int(h[7]) == ref.table_hash(ref.key_of((5, -3, int(g2[7]))), lg, K)
    cells = []
    full = [b for b in np.argsort(-np.bincount(h.astype(np.int64), minlength=T)) if b < T - 64]
    for L, b in zip(sorted(runs, reverse=True), full):
        hit = g2[h == np.uint64(b)][:L]
        assert len(hit) == L, (L, len(hit))
        cells += [(5, -3, int(x)) for x in hit]
    last = [(5, -3, int(x)) for x in g2[h >= np.uint64(T - 2)][:tail]]
    assert len(last) == tail
    return cells + last, lg


def test_keys_that_collide_in_the_first_probe_and_a_chain_that_wraps(engine):
    runs = list(range(2, 41))
    max_in = 2 * (sum(runs) + 8)
    cells, lg = colliding_keys(max_in, runs, 8)
    hs = [ref.table_hash(ref.key_of(g), lg, K) for g in cells]
    assert max(np.bincount(hs)) >= 40 and sum(h >= (1 << lg) - 2 for h in hs) == 8
    rng = np.random.default_rng(6)
    g = np.array(cells + cells)[rng.permutation(2 * len(cells))]              # every cell twice, shuffled
    assert len(g) == max_in and ref.table_lg(len(g), K) == lg
    c = synth(len(g), seed=6)
    c["xyz"] = np.array(ORIGIN) + (g + rng.uniform(0.05, 0.95, g.shape)) * CELL
    got, e = run_and_check(engine, c)
    assert e["report"][5] == len(cells) and (e["info"][:, 0] == 2).all()


# ---- coordinates and the list -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kw", [dict(), dict(count=10**6), dict(count=57), dict(count=-1), dict(k=2, min_support=2),
                                dict(disc_tol=0.0), dict(optional=False)], ids=lambda kw: ",".join("%s=%s" % i for i in kw.items()) or "plain")
def test_boundary_cells_bad_points_a_skipped_map_and_permuted_slots(engine, kw):
    """cloud_ref.boundary_case: g at -2^20 and 2^20 - 1 and one cell outside on every axis, coordinates on a cell face,
    non-finite coordinates, src out of range, a map with an unknown camera, a frame without a slot, slots in another order;
    d_count above max_in, below it, negative and NULL."""
    c = ref.boundary_case()
    if kw.get("optional") is False:
        got = run_merge(engine, c["xyz"], c["src"], c["depth"], c["views"], c["P"], rgba8=c["rgba8"], frame_ids=c["frame_ids"], optional=False)
        e = ref.merge(c["xyz"], c["src"], c["depth"], c["views"], 4, c["P"], CELL, ORIGIN, rgba8=c["rgba8"], frame_ids=c["frame_ids"])
        assert (got["pt_normal"] == 77).all() and (got["cell_of"] == 77).all()
        for k in OUT_KEYS:
            assert bits(got[k][:len(e[k])]) == bits(e[k]), k
        return
    got, e = run_and_check(engine, c, **kw)
    if not kw:
        assert e["report"][2] > 0 and 0 < e["report"][3] < e["report"][1] and 0 < e["report"][4] < e["report"][1]


def test_capacity_at_the_kept_count_and_to_either_side(engine):
    c = ref.boundary_case()
    e = ref.merge(c["xyz"], c["src"], c["depth"], c["views"], 4, c["P"], CELL, ORIGIN, rgba8=c["rgba8"], frame_ids=c["frame_ids"])
    kept = int(e["report"][6])
    for cap in (kept, kept + 1, kept - 1, 0):
        got = run_merge(engine, c["xyz"], c["src"], c["depth"], c["views"], c["P"], rgba8=c["rgba8"], frame_ids=c["frame_ids"],
                        max_points=cap, check=False)
        assert (got["err"] is not None) == (cap < kept), cap
        check_merge(got, e, cap)
    with pytest.raises(pg.CapacityError):
        run_merge(engine, c["xyz"], c["src"], c["depth"], c["views"], c["P"], max_points=kept - 1)


def test_min_support_at_a_cells_count_and_one_above(engine):
    c = ref.boundary_case()
    e = ref.merge(c["xyz"], c["src"], c["depth"], c["views"], 4, c["P"], CELL, ORIGIN)
    top = int(e["cnt"].max())
    assert top >= 2
    got, e1 = run_and_check(engine, c, min_support=top)
    assert e1["report"][6] == (e["cnt"] == top).sum() > 0 and (e1["cell_of"] == -2).any()
    got, e2 = run_and_check(engine, c, min_support=top + 1)
    assert e2["report"][6] == 0 and (got["cell_of"][:len(e2["cell_of"])] < 0).all()


# ---- normals -----------------------------------------------------------------------------------------------------------------------

def every_pixel(depth, views, P, min_agree=0):
    """the filter's list of every pixel with a finite depth (NaN pixels are given a point of their own: the origin's cell)"""
    f = depth_ref.fuse(depth, views, len(P), P, 0.5, min_agree)
    return f["xyz"], f["src"]


@pytest.mark.parametrize("W,H", [(1, 1), (1, 9), (9, 1)])
@pytest.mark.parametrize("k", [1, 8])
def test_normals_on_maps_one_pixel_wide(engine, W, H, k):
    P = np.stack([depth_ref.scene_camera((0.0, 0.0, 0.0), W, H, 9.0).reshape(12)] * 2)
    depth = 3.0 + 0.01 * np.arange(2 * W * H, dtype=np.float64).reshape(2, H, W)
    views = np.array([[0, 1], [1, 0]], np.int32)
    xyz, src = every_pixel(depth, views, P)
    got, e = run_and_check(engine, dict(xyz=xyz, src=src, depth=depth, views=views, P=P), k=k, disc_tol=0.5)
    assert e["report"][1] == 2 * W * H and e["report"][3] == 0           # no direction along one of the two axes: no normal


@pytest.mark.parametrize("k", [1, 8])
def test_normals_at_every_border_and_beside_nonfinite_neighbours(engine, k):
    """20 x 18 maps, every pixel a point: one-sided differences at the four borders (k = 8: the outer eight rows and columns; on
    the 18 rows the two sides overlap), holes of NaN and infinity with a neighbour on each side, a rotated and mirrored camera."""
    W, H = 20, 18
    Rm = depth_ref.look_at((0.3, -0.2, 0.0), (0.0, 0.0, 4.0), 25.0)
    P = np.stack([depth_ref.scene_camera((0.0, 0.0, 0.0), W, H, 22.0).reshape(12),
                  -2.0 * depth_ref.posed_camera(depth_ref.ROT_K * [[0.2], [0.2], [1.0]], Rm, (0.3, -0.2, 0.0)).reshape(12)])
    v, u = np.mgrid[0:H, 0:W]
    depth = np.stack([3.0 + 0.02 * u - 0.01 * v + 0.003 * u * v, 4.0 - 0.01 * u + 0.02 * v]).astype(np.float64)
    depth[0, 5, 5], depth[0, 9, 12], depth[1, 0, 0], depth[1, 17, 19], depth[1, 8, 3] = np.nan, np.inf, np.nan, -np.inf, np.nan
    views = np.array([[0, 1], [1, 0]], np.int32)
    xyz, src = every_pixel(depth, views, P)
    got, e = run_and_check(engine, dict(xyz=xyz, src=src, depth=depth, views=views, P=P), k=k, disc_tol=0.5)
    assert e["report"][1] == 2 * W * H - 5 and e["report"][3] > 0.9 * e["report"][1]
    assert k != 1 or e["report"][3] == e["report"][1]                      # k = 1: every finite pixel has a neighbour along both axes
    # facing the camera: n . (X - C) < 0 for map 0, whose centre is the origin
    m0 = (src[:, 0] == 0) & e["has_normal"]
    assert ((e["pt_normal"][m0].astype(np.float64) * xyz[m0]).sum(1) < 0).all()


def test_disc_tol_at_exact_equality_and_zero(engine):
    """z = 2, neighbours at 2.5: |z' - z| = 0.5 = 0.25 z exactly, so they count at disc_tol 0.25 and not just below; disc_tol 0
    counts equal depths only."""
    W, H = 5, 5
    P = np.stack([depth_ref.scene_camera((0.0, 0.0, 0.0), W, H, 6.0).reshape(12)] * 2)
    depth = np.full((2, H, W), 2.5)
    depth[0, 2, 2] = 2.0
    views = np.array([[0, 1], [1, 0]], np.int32)
    xyz, src = every_pixel(depth, views, P)
    centre = np.flatnonzero((src[:, 0] == 0) & (src[:, 1] == 2 * W + 2))[0]
    c = dict(xyz=xyz, src=src, depth=depth, views=views, P=P)
    for tol, has in ((0.25, True), (np.nextafter(0.25, 0.0), False), (0.0, False)):
        got, e = run_and_check(engine, c, disc_tol=tol)
        assert e["has_normal"][centre] == has, tol
    assert e["report"][3] > 0                  # at 0 the equal depths of map 1 still give normals


def test_a_normal_perpendicular_to_the_ray_is_no_normal(engine):
    """s == 0 by construction: K = diag(f, f, 1), pixel (0, 0), whose ray is (0, 0, f^2); the neighbour at u + 1 has depth 0 (its
    point is the camera centre), so d_u = (0, 0, -z), d_v = (0, z' / f, z' - z), n = (z z' / f, 0, 0), L != 0 and n . e == 0."""
    f = 4.0
    P = np.stack([np.array([[f, 0, 0, 0], [0, f, 0, 0], [0, 0, 1.0, 0]]).reshape(12)] * 2)
    depth = np.full((2, 3, 3), 2.0)
    depth[0, 0, 1] = 0.0
    views = np.array([[0, 1], [1, 0]], np.int32)
    xyz, src = np.array([[0.0, 0.0, 2.0], [0.5, 0.5, 2.0]]), np.array([[0, 0], [0, 4]], np.int32)
    got, e = run_and_check(engine, dict(xyz=xyz, src=src, depth=depth, views=views, P=P), disc_tol=2.0)
    assert not e["has_normal"][0] and e["has_normal"][1] and (got["pt_normal"][0] == 0).all()


@functools.lru_cache(maxsize=None)
def rotated_truth():
    sc = depth_ref.scene_rotated()
    f = depth_ref.fuse(sc["ztrue"], depth_ref.all_views(), 5, sc["P"], 0.05, 1)
    return sc, f


def test_rotated_rig_at_the_true_depths_negated_and_scaled(engine):
    """The CPU test's truth case on the device: 29364 points, 7210 cells, two points without a normal, every normal (0, 0, -1);
    -P for P and the power-of-two scales give the same bits."""
    sc, f = rotated_truth()
    c = dict(xyz=f["xyz"], src=f["src"], depth=sc["ztrue"], views=depth_ref.all_views(), P=sc["P"])
    got, e = run_and_check(engine, c)
    assert tuple(e["report"][[0, 3, 5]]) == (29364, 29362, 7210)
    has = got["pt_normal"].any(1)
    assert ref.angle_to(got["pt_normal"][has], (0, 0, -1)).max() <= 1e-4
    assert ref.angle_to(got["normal"][:7210][got["info"][:7210, 1] > 0], (0, 0, -1)).max() <= 1e-4
    for P in (-sc["P"], depth_ref.scaled_cameras(sc["P"], depth_ref.ROT_SCALES_POW2)):
        other = run_merge(engine, c["xyz"], c["src"], c["depth"], c["views"], P)
        for k in OUT_KEYS + ("pt_normal", "cell_of", "report"):
            assert bits(other[k]) == bits(got[k]), k


# ---- colour -------------------------------------------------------------------------------------------------------------------------

def test_colour_null_one_colour_and_slot_layouts(engine):
    c = synth(900, seed=8, spread=8 * CELL)
    got, e = run_and_check(engine, c)
    assert (e["info"][:, 2] == e["info"][:, 0]).all()
    # the same frames in other slots, a slot that shows no frame in front: the same bits
    again = dict(c, rgba8=np.concatenate([np.full_like(c["rgba8"][:1], 0x55), c["rgba8"][[1, 0]], c["rgba8"][[0]] ^ 0xFFFFFF]),
                 frame_ids=np.array([-1, 1, 0, 0], np.int32))
    got2, _ = run_and_check(engine, again)
    for k in OUT_KEYS:
        assert bits(got2[k]) == bits(got[k]), k
    # NULL colour: nc = 0 and the zero word everywhere
    none = dict(c)
    none.pop("rgba8")
    got3, e3 = run_and_check(engine, none)
    m = int(e3["report"][6])
    assert e3["report"][4] == 0 and (got3["rgba8"][:m] == 0).all() and (got3["info"][:m, 2] == 0).all()
    # one colour: every cell has exactly it, alpha 255
    flat = dict(c, rgba8=np.full_like(c["rgba8"], 0x12C8FF07))
    got4, e4 = run_and_check(engine, flat)
    assert (got4["rgba8"][:m] == 0xFFC8FF07).all()
    # a frame without a slot: its map's points have no colour
    part = dict(c, rgba8=c["rgba8"][[1]], frame_ids=np.array([1], np.int32))
    got5, e5 = run_and_check(engine, part)
    assert 0 < e5["report"][4] < e5["report"][1]


# ---- runs, forms and refusals -------------------------------------------------------------------------------------------------------

def test_repeated_runs_a_used_workspace_and_a_permuted_list(engine):
    c = synth(5000, seed=10, spread=12 * CELL)
    got, e = run_and_check(engine, c, min_support=2)
    run_and_check(engine, synth(70000, seed=11, spread=30 * CELL))           # a larger table in the same workspace
    again, _ = run_and_check(engine, c, min_support=2)
    for k in OUT_KEYS + ("pt_normal", "cell_of", "report"):
        assert bits(again[k]) == bits(got[k]), k
    perm = np.random.default_rng(12).permutation(5000)
    other, eo = run_and_check(engine, dict(c, xyz=c["xyz"][perm], src=c["src"][perm]), min_support=2)
    for k, x in ref.by_key(e).items():
        assert (x == ref.by_key(eo)[k]).all(), k
    m = int(e["report"][6])
    assert m == eo["report"][6] and 0 < m < e["report"][5]
    oa, ob = np.lexsort(got["xyz"][:m].T), np.lexsort(other["xyz"][:m].T)   # the same cells: equal after sorting
    for k in OUT_KEYS:
        x, y = got[k][:m][oa], other[k][:m][ob]
        assert bits(x[:, :3] if k == "info" else x) == bits(y[:, :3] if k == "info" else y), k        # info without `first`


def test_host_form_with_and_without_the_optional_outputs(engine):
    c = ref.boundary_case()
    by_frame = np.zeros((4,) + c["rgba8"].shape[1:], np.uint32)
    by_frame[c["frame_ids"]] = c["rgba8"]                                    # the host form takes colours by frame number
    got = run_merge(engine, c["xyz"], c["src"], c["depth"], c["views"], c["P"], rgba8=by_frame, min_support=2, k=2)
    m = int(got["report"][6])
    h = engine.cloud_merge(c["xyz"], c["src"], c["depth"], c["views"], c["P"], CELL, ORIGIN, rgba8=by_frame, normal_step=2, min_support=2)
    for k in OUT_KEYS:
        assert len(h[k]) == m and bits(h[k]) == bits(got[k][:m]), k
    for k in ("pt_normal", "cell_of", "report"):
        assert bits(h[k]) == bits(got[k]), k
    h0 = engine.cloud_merge(c["xyz"], c["src"], c["depth"], c["views"], c["P"], CELL, ORIGIN, rgba8=by_frame, normal_step=2, min_support=2,
                            pt_normal=False, cell_of=False)
    assert h0["pt_normal"] is None and h0["cell_of"] is None
    for k in OUT_KEYS + ("report",):
        assert bits(h0[k]) == bits(h[k]), k
    with pytest.raises(pg.CapacityError):
        engine.cloud_merge(c["xyz"], c["src"], c["depth"], c["views"], c["P"], CELL, ORIGIN, max_points=m - 1, min_support=2)
    empty = engine.cloud_merge(np.zeros((0, 3)), np.zeros((0, 2), np.int32), c["depth"], c["views"], c["P"], CELL, ORIGIN)
    assert (empty["report"] == 0).all() and len(empty["xyz"]) == 0


def merge_refused(engine, R=2, S=1, W=8, H=8, n_frames=2, max_in=16, max_points=16, cell=0.5, origin=(0.0, 0.0, 0.0), k=1, disc_tol=0.1,
                  min_support=1, F=None, ids=False, alias=None, null=None):
    """pgx_cloud_merge_dev with these arguments over small sentinel-filled buffers: refused, nothing written"""
    i32 = dict(dtype=torch.int32, device=DEV)
    f64 = dict(dtype=torch.float64, device=DEV)
    b = dict(xyz=torch.full((16, 3), 1.0, **f64), src=torch.zeros((16, 2), **i32), count=torch.full((4,), 16, **i32),
             depth=torch.full((2, 8, 8), 3.0, **f64), views=torch.zeros((2, 2), **i32), P=torch.zeros((2, 12), **f64),
             rgba8=torch.zeros((2, 8, 8), **i32), ids=torch.zeros((2,), **i32))
    o = dict(oxyz=torch.full((16, 3), 5.0, **f64), onrm=torch.full((16, 3), 5.0, dtype=torch.float32, device=DEV), orgb=torch.full((16,), 77, **i32),
             oinf=torch.full((16, 4), 77, **i32), ptn=torch.full((16, 3), 77, **i32), cof=torch.full((16,), 77, **i32), rep=torch.full((8,), 77, **i32))
    a = dict(b, **o)
    if alias:
        a[alias[0]] = a[alias[1]]
    if null:
        a[null] = None
    torch.cuda.synchronize()
    with pytest.raises(pg.ArgumentException):
        engine.cloud_merge_dev(a["xyz"], a["src"], a["count"], max_in, a["depth"], a["views"], R, S, W, H, n_frames, a["P"], cell, origin,
                               max_points, a["oxyz"], a["onrm"], a["orgb"], a["oinf"], a["rep"], d_rgba8=a["rgba8"] if F is not None else None,
                               F=F or 0, d_frame_ids=a["ids"] if ids else None, normal_step=k, disc_tol=disc_tol, min_support=min_support,
                               d_pt_normal=a["ptn"], d_cell_of=a["cof"])
    torch.cuda.synchronize()
    engine.check_status()
    assert all((o[x] == 5.0).all() for x in ("oxyz", "onrm")) and all((o[x] == 77).all() for x in ("orgb", "oinf", "ptn", "cof", "rep"))
    assert (b["xyz"] == 1.0).all() and (b["depth"] == 3.0).all()


INF, NAN = float("inf"), float("nan")


@pytest.mark.parametrize("kw", [
    dict(S=0), dict(S=9), dict(R=0), dict(R=65536, W=1, H=1), dict(W=0), dict(H=65536), dict(R=1, W=32768, H=32769), dict(n_frames=0),
    dict(max_in=-1), dict(max_in=2**28 + 1), dict(max_points=-1), dict(max_points=2**28 + 1),
    dict(cell=0.0), dict(cell=-1.0), dict(cell=INF), dict(cell=NAN), dict(origin=(0.0, NAN, 0.0)), dict(origin=(INF, 0.0, 0.0)),
    dict(origin=(0.0, 0.0, -INF)), dict(k=0), dict(k=9), dict(disc_tol=-1e-300), dict(disc_tol=INF), dict(disc_tol=NAN), dict(min_support=0),
    dict(F=0), dict(F=65536), dict(F=3), dict(F=1, W=32768, H=32769, R=1), dict(null="xyz"), dict(null="src"), dict(null="depth"),
    dict(null="views"), dict(null="P"), dict(null="oxyz"), dict(null="onrm"), dict(null="orgb"), dict(null="oinf"), dict(null="rep"),
    dict(alias=("oxyz", "xyz")), dict(alias=("ptn", "src")), dict(alias=("rep", "count")), dict(alias=("cof", "views")),
    dict(alias=("oxyz", "depth"))], ids=lambda kw: ",".join("%s=%s" % i for i in kw.items()))
def test_merge_refusals(engine, kw):
    """cloud_args and the overlap test run before the workspace is sized and a kernel launched."""
    merge_refused(engine, **kw)


# ---- the whole scene ---------------------------------------------------------------------------------------------------------------

def scene_chain(engine, wait):
    """grey -> five maps -> filter -> rgba8 -> merge on one stream; wait: a synchronisation behind every call"""
    sc = depth_ref.scene(0.0)
    W, H, D, S = depth_ref.SCENE_W, depth_ref.SCENE_H, depth_ref.SCENE_D, 4
    rgba = ref.grey_to_rgba16(sc["gray"])
    g = rgba[..., 0]
    rgba[..., 1], rgba[..., 2] = g, g                                        # grey frames: the depth maps see sc["gray"] to 1 / 65535
    rgba[..., 3] = 65535
    i32 = dict(dtype=torch.int32, device=DEV)
    f64 = dict(dtype=torch.float64, device=DEV)
    d_rgba, dP, dv = dev(rgba, np.uint16), dev(sc["P"], np.float64), dev(depth_ref.all_views(), np.int32)
    dr = dev([sc["range"]] * 5, np.float64)
    gray, col = torch.zeros((5, H, W), dtype=torch.float32, device=DEV), torch.zeros((5, H, W), **i32)
    kq8, fl, msum = torch.zeros((5, H, W), **i32), torch.zeros((5, H, W), **i32), torch.zeros((8,), **i32)
    dep = torch.zeros((5, H, W), **f64)
    cap = 5 * W * H
    pts, src, fsum = torch.zeros((cap, 3), **f64), torch.zeros((cap, 2), **i32), torch.zeros((4,), **i32)
    oxyz, onrm = torch.zeros((cap, 3), **f64), torch.zeros((cap, 3), dtype=torch.float32, device=DEV)
    orgb, oinf, ptn, rep = torch.zeros((cap,), **i32), torch.zeros((cap, 4), **i32), torch.zeros((cap, 3), **i32), torch.zeros((8,), **i32)
    torch.cuda.synchronize()
    step = torch.cuda.synchronize if wait else (lambda: None)
    engine.gray_batch_dev(d_rgba, 5, W, H, gray)
    step()
    engine.depth_maps_dev(gray, 5, W, H, 5, dP, dv, 5, S, dr, D, kq8, dep, fl, msum, agg_radius=2, min_views=2)
    step()
    engine.depth_fuse_dev(dep, dv, 5, S, W, H, 5, dP, cap, pts, src, fsum, rel_tol=0.05, min_agree=2)
    step()
    engine.rgba8_batch_dev(d_rgba, 5, W, H, col)
    step()
    engine.cloud_merge_dev(pts, src, fsum, cap, dep, dv, 5, S, W, H, 5, dP, CELL, ORIGIN, cap, oxyz, onrm, orgb, oinf, rep, d_rgba8=col, F=5,
                           normal_step=3, d_pt_normal=ptn)
    engine.check_status()
    out = dict(xyz=oxyz, normal=onrm, rgba8=orgb, info=oinf, pt_normal=ptn, report=rep, depth=dep, pts=pts, src=src, fsum=fsum, col=col)
    return sc, {k: v.cpu().numpy() for k, v in out.items()}


def test_the_scene_as_one_run(engine):
    """One wait at the end and a wait behind every call give the same bits; the merge equals the yardstick on the device's own
    depth maps, list and colours; the entries, the cells and the two fractions of normals within 20 degrees equal what the
    yardstick alone gives on the scene (tests/test_cloud_ref.py's plain case at k = 3: 24124, 9564, 0.98275, 0.99877)."""
    sc, a = scene_chain(engine, wait=False)
    _, b = scene_chain(engine, wait=True)
    for k in a:
        assert bits(a[k]) == bits(b[k]), k
    n = int(a["fsum"][0])
    e = ref.merge(a["pts"], a["src"], a["depth"], depth_ref.all_views(), 5, sc["P"], CELL, ORIGIN, k=3, count=n, rgba8=a["col"].view(np.uint32))
    m = int(e["report"][6])
    assert (a["report"] == e["report"]).all() and 0 < m < n and e["report"][4] == e["report"][1] == n
    assert (a["pt_normal"][:n] == e["pt_normal"]).all() and (a["info"][:m] == e["info"]).all()
    assert (a["rgba8"][:m].view(np.uint32) == e["rgba8"]).all()
    assert bits(a["xyz"][:m]) == bits(e["xyz"]) and bits(a["normal"][:m]) == bits(e["normal"])
    g8 = (np.round(sc["gray"].astype(np.float64) * 65535.0).astype(np.uint16) >> 8).astype(np.uint32)
    assert (a["col"].view(np.uint32) == (g8 | g8 << 8 | g8 << 16 | np.uint32(255) << 24)).all()
    # the CPU test's figures: the yardstick alone on scene(0.0), float32 grey -> depth_ref.depth_maps -> depth_ref.fuse -> merge
    out = depth_ref.depth_maps(sc["gray"], None, 5, sc["P"], depth_ref.all_views(), [sc["range"]] * 5, depth_ref.SCENE_D, 2, 2, 10**6)
    f = depth_ref.fuse(out["depth"], depth_ref.all_views(), 5, sc["P"], 0.05, 2)
    cpu = ref.merge(f["xyz"], f["src"], out["depth"], depth_ref.all_views(), 5, sc["P"], CELL, ORIGIN, k=3)

    def fractions(pt_normal, normal, info):
        lim = np.radians(20.0)
        sel = (info[:, 0] >= 3) & (info[:, 1] > 0)
        return (float((ref.angle_to(pt_normal[pt_normal.any(1)], (0, 0, -1)) <= lim).mean()),
                float((ref.angle_to(normal[sel], (0, 0, -1)) <= lim).mean()))
    pts, cells = fractions(a["pt_normal"][:n], a["normal"][:m], a["info"][:m])
    cpu_pts, cpu_cells = fractions(cpu["pt_normal"], cpu["normal"], cpu["info"])
    print("device chain: %d points, %d cells, %.5f of the points and %.5f of the cells with support >= 3 within 20 degrees; "
          "the yardstick alone: %d, %d, %.5f, %.5f" % (n, a["report"][5], pts, cells, cpu["report"][0], cpu["report"][5], cpu_pts, cpu_cells))
    assert a["report"][0] == cpu["report"][0] and a["report"][5] == cpu["report"][5]
    assert pts == cpu_pts and cells == cpu_cells
    assert pts >= ref.FLOORS[("plain", 3)][0] and cells >= ref.FLOORS[("plain", 3)][1] and cells > pts


# ---- pgx_rgba8_batch_dev ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("fmt", [_lib.PGX_SRC_RGBA64, _lib.PGX_SRC_RGBA8])
@pytest.mark.parametrize("with_map", [False, True])
@pytest.mark.parametrize("W", [36, 37, 38, 39])
def test_rgba8_batch_equals_dewarp_packed(fmt, with_map, W):
    """both source formats, with and without a map, widths 0 .. 3 modulo 4, five frames (a full group of four and one more):
    pgx_dewarp's output, shifted and packed on the CPU; the host form gives the same words"""
    H, F = 11, 5
    rng = np.random.default_rng(31 + W)
    dt = np.uint8 if fmt == _lib.PGX_SRC_RGBA8 else np.uint16
    frames = rng.integers(0, np.iinfo(dt).max + 1, (F, H, W, 4)).astype(dt)
    v, u = np.mgrid[0:H, 0:W]
    eng = pg.Engine(0)
    try:
        eng.set_source_format(fmt)
        if with_map:
            eng.set_dewarp_map(np.stack([rng.integers(0, W, (H, W)), rng.integers(0, H, (H, W))], -1))
        out = torch.full((F, H, W), 77, dtype=torch.int32, device=DEV)
        d_rgba = torch.from_numpy(frames).to(DEV)
        torch.cuda.synchronize()
        eng.rgba8_batch_dev(d_rgba, F, W, H, out)
        eng.check_status()
        got = out.cpu().numpy().view(np.uint32)
        host = eng.rgba8_batch(frames)
        if not with_map:
            eng.set_dewarp_map(np.stack([u, v], -1))                         # pgx_dewarp wants a map: the identity
        for i in range(F):
            want = ref.pack_rgba8(eng.dewarp(frames[i]))                     # 16-bit whatever the source format
            assert (got[i] == want).all() and (host[i] == want).all(), i
        if fmt == _lib.PGX_SRC_RGBA8 and not with_map:
            assert bits(got) == bits(frames)                                 # an RGBA8 source's bytes as they are
    finally:
        eng.close()


@pytest.mark.parametrize("fmt", [_lib.PGX_SRC_RGBA64, _lib.PGX_SRC_RGBA8])
def test_rgba8_batch_map_entries_out_of_range_and_a_wrong_size(fmt):
    W, H, F = 13, 7, 2
    rng = np.random.default_rng(41)
    dt = np.uint8 if fmt == _lib.PGX_SRC_RGBA8 else np.uint16
    frames = rng.integers(1, np.iinfo(dt).max + 1, (F, H, W, 4)).astype(dt)
    m = np.stack([rng.integers(0, W, (H, W)), rng.integers(0, H, (H, W))], -1)
    m[0, 0], m[3, 5], m[6, 12] = (W, 0), (0, H), (70000, 1)                 # three entries outside; 70000 wraps to 4464
    eng = pg.Engine(0)
    try:
        eng.set_source_format(fmt)
        eng.set_dewarp_map(m)
        out = torch.full((F, H, W), 77, dtype=torch.int32, device=DEV)
        d_rgba = torch.from_numpy(frames).to(DEV)
        torch.cuda.synchronize()
        eng.rgba8_batch_dev(d_rgba, F, W, H, out)
        with pytest.raises(pg.IndexOutOfRangeException):
            eng.check_status()
        got = out.cpu().numpy().view(np.uint32)
        src = frames[:, np.clip(m[..., 1], 0, H - 1), np.clip(m[..., 0], 0, W - 1)]
        want = ref.pack_rgba8(src)
        bad = np.zeros((H, W), bool)
        bad[0, 0] = bad[3, 5] = bad[6, 12] = True
        assert (got[:, ~bad] == want[:, ~bad]).all() and (got[:, bad] == 0).all()
        with pytest.raises(pg.ArgumentException):
            eng.rgba8_batch_dev(d_rgba, F, W + 1, H, out)
        with pytest.raises(pg.ArgumentException):
            eng.rgba8_batch_dev(d_rgba, 0, W, H, out)
    finally:
        eng.close()
