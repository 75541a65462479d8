"""GPU tests of the mesh (pgx_mesh_dev and the host form pgx_mesh; k_mesh.hip) against tests/mesh_ref.py: every integer output
and every bit of the float outputs equals the yardstick's.  The shapes are the smallest at which the kernels can go wrong: the
scan block, the grid, the table's size and the hash are read or restated from the kernel source (mesh_ref.kernel_constants,
table_hash)."""
import functools

import numpy as np
import pytest
import torch

import cloud_ref
import depth_ref
import mesh_ref as ref
import photogrammetry_amd as pg
from mesh_gpu import CELL, DEV, ORIGIN, dev, rig, run_mesh, synth
from photogrammetry_amd import _lib

pytestmark = pytest.mark.gpu

K = ref.kernel_constants(_lib.CSRC)
NT, GRID = K["MSH_NT"], K["MSH_GRID_MAX"]
OUT_KEYS = ref.OUT_KEYS
bits = ref.bits


def yardstick(c, cell=CELL, origin=ORIGIN, **kw):
    return ref.mesh(c["xyz"], c["src"], c["depth"], c["views"], len(np.reshape(c["P"], (-1, 12))), c["P"], cell, origin,
                    agree=c.get("agree"), rgba8=c.get("rgba8"), frame_ids=c.get("frame_ids"), **kw)


def check_mesh(got, e, caps):
    """the device's outputs against the yardstick's: the first min(count, capacity) rows, nothing behind them"""
    assert (got["report"] == e["report"]).all(), (got["report"], e["report"])
    mv, mt = min(len(e["xyz"]), caps[1]), min(len(e["tri"]), caps[2])
    assert (got["info"][:mv] == e["info"][:mv]).all(), np.argwhere(got["info"][:mv] != e["info"][:mv])[:5]
    assert (got["rgba8"][:mv] == e["rgba8"][:mv]).all()
    assert bits(got["xyz"][:mv]) == bits(e["xyz"][:mv]), np.argwhere(got["xyz"][:mv] != e["xyz"][:mv])[:5]
    assert bits(got["normal"][:mv]) == bits(e["normal"][:mv]), np.argwhere(got["normal"][:mv] != e["normal"][:mv])[:5]
    assert (got["tri"][:mt] == e["tri"][:mt]).all(), np.argwhere(got["tri"][:mt] != e["tri"][:mt])[:5]
    nothing_behind(got, mv, mt)


def nothing_behind(got, mv, mt):
    assert (got["xyz"][mv:] == 5.0).all() and (got["normal"][mv:] == 5.0).all() and (got["rgba8"][mv:] == 77).all()
    assert (got["info"][mv:] == 77).all() and (got["tri"][mt:] == 77).all()


def run_and_check(engine, c, caps=None, cell=CELL, origin=ORIGIN, **kw):
    """the yardstick and the device on case c, compared; caps default to a few more than the yardstick's counts"""
    e = yardstick(c, cell, origin, **kw)
    if caps is None:
        caps = (int(e["report"][3]) + 5, len(e["xyz"]) + 3, len(e["tri"]) + 3)
    got = run_mesh(engine, c, caps, cell, origin, **kw)
    check_mesh(got, e, caps)
    return got, e


# ---- 1 counts ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", [0, 1, NT - 1, NT, NT + 1, NT * NT + 1, (GRID + 16) * NT])
def test_list_lengths_round_the_scan_block_and_the_grid(engine, n):
    """0, 1 and the scan block's 255, 256, 257 points; 65 537 = more than 256 block counts (a second chunk of the scan); 266 240 =
    more than one pass of the 1024-workgroup grid.  The points fall in a few hundred cells: the voxel count stays small."""
    assert NT * NT + 1 == 65537 and (GRID + 16) * NT == 266240
    c = synth(n + 3, seed=n)
    got, e = run_and_check(engine, c, count=n, band=2)
    assert e["report"][0] == n and e["report"][3] < 20000 and (n < 100 or e["report"][6] > 0)


@pytest.mark.parametrize("kw", [dict(count=10**6), dict(count=57), dict(count=-1), dict()], ids=lambda kw: ",".join("%s=%s" % i for i in kw.items()) or "null")
def test_count_above_below_negative_and_null(engine, kw):
    c = synth(300, seed=5)
    got, e = run_and_check(engine, c, band=2, **kw)
    assert e["report"][0] == {10**6: 300, 57: 57, -1: 0}.get(kw.get("count"), 300)


# ---- 2 the table -------------------------------------------------------------------------------------------------------------------

def colliding_cells(max_voxels, runs, tail):
    """cells (5, g1, g2) found by search whose own node's first probe is the same table entry, in runs of the given lengths, and
    `tail` cells whose node's first probe is one of the table's last two entries (their chain wraps past the end)"""
    lg = ref.table_lg(max_voxels, K)
    T = 1 << lg
    g1, g2 = (x.reshape(-1) for x in np.meshgrid(np.arange(-3, 5), np.arange(-500000, 500000), indexing="ij"))
    keys = np.array([cloud_ref.key_of((5, 0, 0))], dtype=np.uint64) + (g1.astype(np.int64) * (1 << 21) + g2).astype(np.uint64)
    h = (keys * np.uint64(K["MSH_HASH_MUL"])) >> np.uint64(64 - lg)           # uint64 products wrap modulo 2^64
    assert int(h[7]) == ref.table_hash(cloud_ref.key_of((5, int(g1[7]), int(g2[7]))), lg, K)
    cells = []
    full = [b for b in np.argsort(-np.bincount(h.astype(np.int64), minlength=T)) if b < T - 64]
    for L, b in zip(sorted(runs, reverse=True), full):
        hit = np.flatnonzero(h == np.uint64(b))[:L]
        assert len(hit) == L, (L, len(hit))
        cells += [(5, int(g1[x]), int(g2[x])) for x in hit]
    last = [(5, int(g1[x]), int(g2[x])) for x in np.flatnonzero(h >= np.uint64(T - 2))[:tail]]
    assert len(last) == tail
    return cells + last, lg


def test_nodes_that_collide_in_the_first_probe_and_a_chain_that_wraps(engine):
    runs = list(range(2, 41))
    max_voxels = 16384
    cells, lg = colliding_cells(max_voxels, runs, 8)
    hs = [ref.table_hash(cloud_ref.key_of(g), lg, K) for g in cells]
    assert max(np.bincount(hs)) >= 40 and sum(h >= (1 << lg) - 2 for h in hs) == 8
    rng = np.random.default_rng(6)
    c = synth(400, seed=6)                                                    # a surface beside them: the lookups of a real mesh
    g = np.array(cells + cells)[rng.permutation(2 * len(cells))]              # every cell twice, shuffled
    far = np.array(ORIGIN) + (g + rng.uniform(0.05, 0.95, g.shape)) * CELL
    c["xyz"] = np.concatenate([far[:500], c["xyz"], far[500:]])
    c["src"] = np.concatenate([np.zeros((500, 2), np.int32), c["src"], np.zeros((len(far) - 500, 2), np.int32)])
    e = yardstick(c)
    assert 8 * len(cells) <= e["report"][3] <= max_voxels and e["report"][5] > 0
    got = run_mesh(engine, c, (max_voxels, len(e["xyz"]), len(e["tri"])))
    check_mesh(got, e, (max_voxels, len(e["xyz"]), len(e["tri"])))


# ---- 3 capacities --------------------------------------------------------------------------------------------------------------------

def test_max_voxels_at_the_count_and_one_below(engine):
    c = synth(500, seed=7)
    e = yardstick(c, band=2)
    V, A, Tn = int(e["report"][3]), len(e["xyz"]), len(e["tri"])
    assert V > 256 and A > 0 and Tn > 0
    got = run_mesh(engine, c, (V, A, Tn), band=2)
    check_mesh(got, e, (V, A, Tn))
    for mvox in (V - 1, V // 2, 100, 0):                                      # 100 and 0: the table of 256 entries fills
        got = run_mesh(engine, c, (mvox, A, Tn), band=2, check=False)
        assert got["err"] is not None, mvox
        assert got["report"][5] == 0 and got["report"][6] == 0 and got["report"][3] > mvox and got["report"][7] == 0
        assert got["report"][0] == 500 and (mvox != V - 1 or got["report"][3] == V)
        nothing_behind(got, 0, 0)
    with pytest.raises(pg.CapacityError):
        run_mesh(engine, c, (V - 1, A, Tn), band=2)
    again = run_mesh(engine, c, (V, A, Tn), band=2)                           # the error leaves nothing behind in the workspace
    check_mesh(again, e, (V, A, Tn))


def test_max_vertices_and_max_tris_at_the_count_and_to_either_side(engine):
    c = synth(500, seed=7)
    e = yardstick(c, band=2)
    V, A, Tn = int(e["report"][3]) + 9, len(e["xyz"]), len(e["tri"])
    for mv, mt in ((A, Tn), (A - 1, Tn), (A + 1, Tn), (0, Tn), (A, Tn - 1), (A, Tn + 1), (A, 0), (A, Tn - 3), (0, 0)):
        got = run_mesh(engine, c, (V, mv, mt), band=2, check=False)
        assert (got["err"] is not None) == (mv < A or mt < Tn), (mv, mt)
        check_mesh(got, e, (V, mv, mt))                                       # the triangles name full vertex indices


# ---- 4 the rule's parameters ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("band", [1, 2, 3])
@pytest.mark.parametrize("trunc_cells", [1, 3, 8])
def test_band_and_truncation(engine, band, trunc_cells):
    c = dict(rig())
    got, e = run_and_check(engine, c, band=band, trunc_cells=trunc_cells)
    assert e["report"][3] > 0 and (band == 1 or e["report"][6] > 0)


def test_min_weight_at_the_largest_weight_and_one_above(engine):
    c = dict(rig())
    e = yardstick(c, band=2)
    top = int(e["w"].max())
    assert top == 2
    got, e1 = run_and_check(engine, c, band=2, min_weight=top)
    assert 0 < e1["report"][4] < e["report"][4] and e1["report"][5] > 0
    got, e2 = run_and_check(engine, c, band=2, min_weight=top + 1)
    assert e2["report"][4] == 0 and e2["report"][5] == 0 and e2["report"][6] == 0


def flat_rig(za, zb=2.0):
    """Two cameras K [I | 0], K = (4, 4; 4, 4) on 8 x 8 maps, whose constant depths are za and zb.  A node (x, y, z) of the grid of
    0.25 has d = z exactly and u = 4 x / z + 4: at z = 2 every half pixel, so nodes project onto each border of the image
    (u = -0.5: the first pixel; u = 7.5: outside) and half a pixel outside (u = -1).  The list: the filter's, and points out at
    the image's borders on the plane z = 2."""
    W = H = 8
    P = np.stack([np.array([[4.0, 0, 4.0, 0], [0, 4.0, 4.0, 0], [0, 0, 1.0, 0]]).reshape(12)] * 2)
    depth = np.stack([np.full((H, W), za), np.full((H, W), zb)]).astype(np.float64)
    views = np.array([[0, 1], [1, 0]], np.int32)
    f = depth_ref.fuse(depth, views, 2, P, 0.5, 0)
    t = np.array([-2.45, -2.3, -2.2, 1.55, 1.7, 1.8])
    edge = np.array([[x, y, 2.05] for x in t for y in t])
    rgba8 = np.random.default_rng(2).integers(0, 2**32, (2, H, W), dtype=np.uint32)
    return dict(xyz=np.concatenate([f["xyz"], edge]), src=np.concatenate([f["src"], np.zeros((len(edge), 2), np.int32)]), depth=depth,
                views=views, P=P, rgba8=rgba8)


def test_s_exactly_at_the_truncation_and_one_ulp_past_it(engine):
    """trunc_cells 1: trunc = 0.25.  The nodes at z = 2: against a map at 1.75, s = -trunc exactly: the map counts; one ulp below,
    it is passed over.  Against a map at 2.25, s = trunc: the colour counts; one ulp above, the weight counts and the colour does
    not."""
    sums = {}
    for name, za in (("lo", 1.75), ("lo-", np.nextafter(1.75, 0.0)), ("hi", 2.25), ("hi+", np.nextafter(2.25, 3.0))):
        c = flat_rig(za)
        got, e = run_and_check(engine, c, band=2, trunc_cells=1)
        at2 = ref.unpack(e["vox"])[:, 2] == 40                               # z = -8 + 40 / 4 = 2
        assert at2.any()
        sums[name] = (int(e["w"][at2].sum()), int(e["nc"][at2].sum()))
    assert sums["lo"][0] > sums["lo-"][0] and sums["hi"][0] == sums["hi+"][0] and sums["hi"][1] > sums["hi+"][1]


def test_agree_at_min_agree_one_below_and_null(engine):
    c = dict(rig())
    c["agree"] = np.random.default_rng(3).integers(0, 4, c["depth"].shape).astype(np.int32)
    got, e = run_and_check(engine, c, band=2, min_agree=2)
    c0 = dict(rig())
    got0, e0 = run_and_check(engine, c0, band=2, min_agree=2)                 # NULL: min_agree is not read
    assert 0 < e["w"].sum() < e0["w"].sum()
    got1, e1 = run_and_check(engine, c, band=2, min_agree=0)
    for k in OUT_KEYS:
        assert bits(got1[k][:len(e0[k])]) == bits(got0[k][:len(e0[k])]), k


# ---- 5 borders and cameras -------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("W,H", [(1, 1), (1, 9), (9, 1)])
def test_maps_one_pixel_wide(engine, W, H):
    P = np.stack([depth_ref.scene_camera((0.0, 0.0, 0.0), W, H, 9.0).reshape(12)] * 2)
    depth = 3.0 + 0.01 * np.arange(2 * W * H, dtype=np.float64).reshape(2, H, W)
    views = np.array([[0, 1], [1, 0]], np.int32)
    f = depth_ref.fuse(depth, views, 2, P, 0.5, 0)
    got, e = run_and_check(engine, dict(xyz=f["xyz"], src=f["src"], depth=depth, views=views, P=P), band=3, trunc_cells=2)
    assert e["report"][1] == 2 * W * H and e["report"][4] > 0


def test_projections_on_the_image_borders_and_half_a_pixel_outside(engine):
    c = flat_rig(2.0)
    got, e = run_and_check(engine, c, band=2, trunc_cells=2)
    node = ref.unpack(e["vox"])
    at2 = node[:, 2] == 40
    u = 2.0 * (-8.0 + node[at2, 0] / 4.0) + 4.0
    assert {-1.0, -0.5, 7.0, 7.5} <= set(u.tolist())
    assert (e["w"][at2][u == -0.5] > 0).any() and (e["w"][at2][u == -1.0] == 0).all() and (e["w"][at2][u == 7.5] == 0).all()
    assert e["report"][6] > 0


@pytest.mark.parametrize("kw", [dict(), dict(band=2, trunc_cells=1), dict(band=3, trunc_cells=8, min_weight=2), dict(count=57)],
                         ids=lambda kw: ",".join("%s=%s" % i for i in kw.items()) or "plain")
def test_boundary_cells_bad_points_nonfinite_depths_a_skipped_map_and_a_negated_camera(engine, kw):
    """mesh_ref.boundary_case: NaN and infinite coordinates, src out of range, g at the margin and one cell past it, a NaN depth, a
    map whose camera is unknown, -P for a camera, a frame without a slot, slots in another order, agreement counts"""
    c = ref.boundary_case()
    c["depth"] = c["depth"].copy()
    c["depth"][1, 5, 5], c["depth"][0, 1, 1] = np.inf, -np.inf
    got, e = run_and_check(engine, c, cell=ref.CELL, **kw)
    assert e["report"][1] < e["report"][0] and e["report"][3] > 0
    far = dict(c, views=np.array([[0, 1, 2], [7, 0, 2], [-1, 0, 1]], np.int32))   # frames outside [0, n_frames)
    run_and_check(engine, far, cell=ref.CELL, **kw)


def test_rotated_rig_at_the_true_depths_negated_and_scaled(engine):
    """The CPU test's truth case on the device.  The power-of-two scales change no bit.  A negated camera sees nothing by the
    filter's q_2 > 0, so its map is passed over: ROT_SCALES_POW2, whose first scale is negative, is compared with the cameras of
    the same signs at scale 1, and its magnitudes with the plain cameras."""
    sc = depth_ref.scene_rotated()
    f = depth_ref.fuse(sc["ztrue"], depth_ref.all_views(), 5, sc["P"], 0.05, 1)
    c = dict(xyz=f["xyz"], src=f["src"], depth=sc["ztrue"], views=depth_ref.all_views(), P=sc["P"], agree=f["agree"])
    got, e = run_and_check(engine, c, cell=ref.CELL, band=2, trunc_cells=3, min_agree=1)
    assert e["report"][5] > 5000 and e["report"][6] > 10000
    caps = (int(e["report"][3]) + 5, len(e["xyz"]) + 3, len(e["tri"]) + 3)
    pow2 = np.array(depth_ref.ROT_SCALES_POW2)
    other = run_mesh(engine, dict(c, P=depth_ref.scaled_cameras(sc["P"], np.abs(pow2))), caps, cell=ref.CELL, band=2, trunc_cells=3, min_agree=1)
    for k in OUT_KEYS + ("report",):
        assert bits(other[k]) == bits(got[k]), k
    signed, e_s = run_and_check(engine, dict(c, P=depth_ref.scaled_cameras(sc["P"], np.sign(pow2))), cell=ref.CELL, band=2, trunc_cells=3,
                                min_agree=1)
    assert e_s["w"].sum() < e["w"].sum()                                      # map 0, negated, is passed over
    caps_s = (int(e_s["report"][3]) + 5, len(e_s["xyz"]) + 3, len(e_s["tri"]) + 3)
    other = run_mesh(engine, dict(c, P=depth_ref.scaled_cameras(sc["P"], pow2)), caps_s, cell=ref.CELL, band=2, trunc_cells=3, min_agree=1)
    for k in OUT_KEYS + ("report",):
        assert bits(other[k]) == bits(signed[k]), k
    none = run_mesh(engine, dict(c, P=-sc["P"]), caps, cell=ref.CELL, band=2, trunc_cells=3, min_agree=1)   # every camera negated: no weight
    assert none["report"][3] == e["report"][3] and none["report"][4] == 0 and none["report"][5] == 0


# ---- 6 colour --------------------------------------------------------------------------------------------------------------------------

def test_colour_null_one_colour_and_slot_layouts(engine):
    c = dict(rig())
    got, e = run_and_check(engine, c, band=2)
    A = len(e["xyz"])
    assert A > 0 and (e["rgba8"] >> 24 == 255).all()
    # the same frames in other slots, a slot that shows no frame in front: the same bits
    again = dict(c, rgba8=np.concatenate([np.full_like(c["rgba8"][:1], 0x55), c["rgba8"][[1, 0]], c["rgba8"][[0]] ^ 0xFFFFFF]),
                 frame_ids=np.array([-1, 1, 0, 0], np.int32))
    got2, _ = run_and_check(engine, again, band=2)
    for k in OUT_KEYS:
        assert bits(got2[k]) == bits(got[k]), k
    none = dict(c)
    none.pop("rgba8")
    got3, e3 = run_and_check(engine, none, band=2)
    assert (got3["rgba8"][:A] == 0).all() and e3["nc"].sum() == 0
    flat = dict(c, rgba8=np.full_like(c["rgba8"], 0x12C8FF07))
    got4, e4 = run_and_check(engine, flat, band=2)
    assert (got4["rgba8"][:A] == 0xFFC8FF07).all()
    part = dict(c, rgba8=c["rgba8"][[1]], frame_ids=np.array([1], np.int32))   # frame 0 has no slot
    got5, e5 = run_and_check(engine, part, band=2)
    assert 0 < e5["nc"].sum() < e["nc"].sum()


# ---- 7 runs, forms and refusals ----------------------------------------------------------------------------------------------------------

def test_repeated_runs_a_used_workspace_and_a_permuted_list(engine):
    c = synth(3000, seed=10)
    got, e = run_and_check(engine, c, band=2)
    run_and_check(engine, synth(20000, seed=11, jitter=4 * CELL), band=3)    # a larger table in the same workspace
    again, _ = run_and_check(engine, c, band=2)
    for k in OUT_KEYS + ("report",):
        assert bits(again[k]) == bits(got[k]), k
    perm = np.random.default_rng(12).permutation(3000)
    other, eo = run_and_check(engine, dict(c, xyz=c["xyz"][perm], src=c["src"][perm]), band=2)
    A, Tn = len(e["xyz"]), len(e["tri"])
    assert A == len(eo["xyz"]) > 0 and Tn == len(eo["tri"]) > 0 and not (e["info"] == eo["info"]).all()
    a = ref.by_cube({k: got[k][:Tn if k == "tri" else A] for k in OUT_KEYS})
    b = ref.by_cube({k: other[k][:Tn if k == "tri" else A] for k in OUT_KEYS})
    for k in OUT_KEYS:
        assert bits(a[k]) == bits(b[k]), k


def test_host_form_with_and_without_colour_and_agree(engine):
    c = ref.boundary_case()
    c["agree"] = np.random.default_rng(4).integers(0, 4, c["depth"].shape).astype(np.int32)   # a quarter of the pixels below min_agree
    by_frame = np.zeros((4,) + c["rgba8"].shape[1:], np.uint32)
    by_frame[c["frame_ids"]] = c["rgba8"]                                    # the host form takes colours by frame number
    n_used = None
    for col, ag in ((by_frame, c["agree"]), (None, c["agree"]), (by_frame, None), (None, None)):
        case = dict(xyz=c["xyz"], src=c["src"], depth=c["depth"], views=c["views"], P=c["P"])
        if col is not None:
            case["rgba8"] = col
        if ag is not None:
            case["agree"] = ag
        got, e = run_and_check(engine, case, cell=ref.CELL, band=2, min_agree=1)
        h = engine.mesh(c["xyz"], c["src"], c["depth"], c["views"], c["P"], ref.CELL, ref.ORIGIN, agree=ag, min_agree=1, rgba8=col, band=2)
        for k in OUT_KEYS:
            assert len(h[k]) == len(e[k]) and bits(h[k]) == bits(got[k][:len(e[k])]), k
        assert (h["report"] == got["report"]).all() and len(e["tri"]) > 0
        n_used = int(e["report"][1])
    assert n_used > 0
    A = len(e["xyz"])
    with pytest.raises(pg.CapacityError):
        engine.mesh(c["xyz"], c["src"], c["depth"], c["views"], c["P"], ref.CELL, ref.ORIGIN, band=2, max_vertices=A - 1)
    with pytest.raises(pg.CapacityError):
        engine.mesh(c["xyz"], c["src"], c["depth"], c["views"], c["P"], ref.CELL, ref.ORIGIN, band=2, max_voxels=int(e["report"][3]) - 1)
    empty = engine.mesh(np.zeros((0, 3)), np.zeros((0, 2), np.int32), c["depth"], c["views"], c["P"], ref.CELL, ref.ORIGIN)
    assert (empty["report"] == 0).all() and len(empty["xyz"]) == 0 and len(empty["tri"]) == 0


def mesh_refused(engine, R=2, S=1, W=8, H=8, n_frames=2, max_in=16, caps=(64, 16, 16), cell=0.5, origin=(0.0, 0.0, 0.0), band=1,
                 trunc_cells=3, min_weight=1, min_agree=0, F=None, ids=False, alias=None, null=None):
    """pgx_mesh_dev with these arguments over small sentinel-filled buffers: refused, nothing written"""
    i32 = dict(dtype=torch.int32, device=DEV)
    f64 = dict(dtype=torch.float64, device=DEV)
    b = dict(xyz=torch.full((16, 3), 1.0, **f64), src=torch.zeros((16, 2), **i32), count=torch.full((4,), 16, **i32),
             depth=torch.full((2, 8, 8), 3.0, **f64), views=torch.zeros((2, 2), **i32), P=torch.zeros((2, 12), **f64),
             agree=torch.zeros((2, 8, 8), **i32), rgba8=torch.zeros((2, 8, 8), **i32), ids=torch.zeros((2,), **i32))
    o = dict(oxyz=torch.full((16, 3), 5.0, **f64), onrm=torch.full((16, 3), 5.0, dtype=torch.float32, device=DEV), orgb=torch.full((16,), 77, **i32),
             oinf=torch.full((16, 4), 77, **i32), otri=torch.full((16, 3), 77, **i32), rep=torch.full((8,), 77, **i32))
    a = dict(b, **o)
    if alias:
        a[alias[0]] = a[alias[1]]
    if null:
        a[null] = None
    torch.cuda.synchronize()
    with pytest.raises(pg.ArgumentException):
        engine.mesh_dev(a["xyz"], a["src"], a["count"], max_in, a["depth"], a["views"], R, S, W, H, n_frames, a["P"], cell, origin, caps[0],
                        caps[1], caps[2], a["oxyz"], a["onrm"], a["orgb"], a["oinf"], a["otri"], a["rep"], d_agree=a["agree"],
                        min_agree=min_agree, d_rgba8=a["rgba8"] if F is not None else None, F=F or 0, d_frame_ids=a["ids"] if ids else None,
                        band=band, trunc_cells=trunc_cells, min_weight=min_weight)
    torch.cuda.synchronize()
    engine.check_status()
    assert all((o[x] == 5.0).all() for x in ("oxyz", "onrm")) and all((o[x] == 77).all() for x in ("orgb", "oinf", "otri", "rep"))
    assert (b["xyz"] == 1.0).all() and (b["depth"] == 3.0).all()


INF, NAN = float("inf"), float("nan")


@pytest.mark.parametrize("kw", [
    dict(S=0), dict(S=9), dict(R=0), dict(R=65536, W=1, H=1), dict(W=0), dict(H=65536), dict(R=1, W=32768, H=32769), dict(n_frames=0),
    dict(max_in=-1), dict(max_in=2**28 + 1), dict(cell=0.0), dict(cell=-1.0), dict(cell=INF), dict(cell=NAN),
    dict(origin=(0.0, NAN, 0.0)), dict(origin=(INF, 0.0, 0.0)), dict(origin=(0.0, 0.0, -INF)),
    dict(F=0), dict(F=65536), dict(F=3), dict(F=1, W=32768, H=32769, R=1),
    dict(band=0), dict(band=4), dict(trunc_cells=0), dict(trunc_cells=9), dict(min_weight=0), dict(min_agree=-1),
    dict(caps=(-1, 16, 16)), dict(caps=(2**28 + 1, 16, 16)), dict(caps=(64, -1, 16)), dict(caps=(64, 2**28 + 1, 16)),
    dict(caps=(64, 16, -1)), dict(caps=(64, 16, 2**28 + 1)),
    dict(null="xyz"), dict(null="src"), dict(null="depth"), dict(null="views"), dict(null="P"), dict(null="oxyz"), dict(null="onrm"),
    dict(null="orgb"), dict(null="oinf"), dict(null="otri"), dict(null="rep"),
    dict(alias=("oxyz", "xyz")), dict(alias=("otri", "src")), dict(alias=("rep", "count")), dict(alias=("oinf", "views")),
    dict(alias=("oxyz", "depth")), dict(alias=("otri", "agree"))], ids=lambda kw: ",".join("%s=%s" % i for i in kw.items()))
def test_mesh_refusals(engine, kw):
    """mesh_args and the overlap test run before the workspace is sized and a kernel launched."""
    mesh_refused(engine, **kw)


def test_null_outputs_at_capacity_zero(engine):
    c = synth(300, seed=5)
    e = yardstick(c, band=2)
    i32 = dict(dtype=torch.int32, device=DEV)
    rep = torch.full((8,), 77, **i32)
    dx, ds, dd, dv, dP = dev(c["xyz"], np.float64), dev(c["src"], np.int32), dev(c["depth"], np.float64), dev(c["views"], np.int32), dev(c["P"], np.float64)
    torch.cuda.synchronize()
    engine.mesh_dev(dx, ds, None, 300, dd, dv, 2, 1, c["W"], c["H"], 2, dP, CELL, ORIGIN, 4096, 0, 0, None, None, None, None, None, rep, band=2)
    with pytest.raises(pg.CapacityError):
        engine.check_status()
    assert (rep.cpu().numpy() == e["report"]).all() and e["report"][5] > 0


# ---- 8 the whole scene -----------------------------------------------------------------------------------------------------------------

SCENE_CAPS = (1 << 19, 1 << 17, 1 << 18)


def scene_chain(engine, wait):
    """grey -> five maps -> filter -> rgba8 -> mesh on one stream; wait: a synchronisation behind every call"""
    sc = depth_ref.scene(0.0)
    W, H, D, S = depth_ref.SCENE_W, depth_ref.SCENE_H, depth_ref.SCENE_D, 4
    rgba = cloud_ref.grey_to_rgba16(sc["gray"])
    g = rgba[..., 0]
    rgba[..., 1], rgba[..., 2] = g, g                                        # grey frames: the depth maps see sc["gray"] to 1 / 65535
    rgba[..., 3] = 65535
    i32 = dict(dtype=torch.int32, device=DEV)
    f64 = dict(dtype=torch.float64, device=DEV)
    d_rgba, dP, dv = dev(rgba, np.uint16), dev(sc["P"], np.float64), dev(depth_ref.all_views(), np.int32)
    dr = dev([sc["range"]] * 5, np.float64)
    gray, col = torch.zeros((5, H, W), dtype=torch.float32, device=DEV), torch.zeros((5, H, W), **i32)
    kq8, fl, msum = torch.zeros((5, H, W), **i32), torch.zeros((5, H, W), **i32), torch.zeros((8,), **i32)
    dep, agr = torch.zeros((5, H, W), **f64), torch.zeros((5, H, W), **i32)
    cap = 5 * W * H
    pts, src, fsum = torch.zeros((cap, 3), **f64), torch.zeros((cap, 2), **i32), torch.zeros((4,), **i32)
    mvox, mv, mt = SCENE_CAPS
    oxyz, onrm = torch.zeros((mv, 3), **f64), torch.zeros((mv, 3), dtype=torch.float32, device=DEV)
    orgb, oinf, otri, rep = torch.zeros((mv,), **i32), torch.zeros((mv, 4), **i32), torch.zeros((mt, 3), **i32), torch.zeros((8,), **i32)
    torch.cuda.synchronize()
    step = torch.cuda.synchronize if wait else (lambda: None)
    engine.gray_batch_dev(d_rgba, 5, W, H, gray)
    step()
    engine.depth_maps_dev(gray, 5, W, H, 5, dP, dv, 5, S, dr, D, kq8, dep, fl, msum, agg_radius=2, min_views=2)
    step()
    engine.depth_fuse_dev(dep, dv, 5, S, W, H, 5, dP, cap, pts, src, fsum, rel_tol=0.05, min_agree=2, d_agree=agr)
    step()
    engine.rgba8_batch_dev(d_rgba, 5, W, H, col)
    step()
    engine.mesh_dev(pts, src, fsum, cap, dep, dv, 5, S, W, H, 5, dP, ref.CELL, ref.TRUTH_ORIGIN, mvox, mv, mt, oxyz, onrm, orgb, oinf, otri, rep,
                    d_agree=agr, min_agree=2, d_rgba8=col, F=5, band=2, trunc_cells=3)
    engine.check_status()
    out = dict(xyz=oxyz, normal=onrm, rgba8=orgb, info=oinf, tri=otri, report=rep, depth=dep, agree=agr, pts=pts, src=src, fsum=fsum, col=col)
    return sc, {k: v.cpu().numpy() for k, v in out.items()}


def test_the_scene_as_one_run(engine):
    """One wait at the end and a wait behind every call give the same bits; the mesh equals the yardstick on the device's own
    depth maps, agreement counts, list and colours; the counts and the fractions equal what the yardstick alone gives on the scene
    (tests/test_mesh_ref.py's plain case)."""
    sc, a = scene_chain(engine, wait=False)
    _, b = scene_chain(engine, wait=True)
    for k in a:
        assert bits(a[k]) == bits(b[k]), k
    n = int(a["fsum"][0])
    e = ref.mesh(a["pts"], a["src"], a["depth"], depth_ref.all_views(), 5, sc["P"], ref.CELL, ref.TRUTH_ORIGIN, band=2, trunc_cells=3, agree=a["agree"],
                 min_agree=2, rgba8=a["col"].view(np.uint32), count=n)
    A, Tn = len(e["xyz"]), len(e["tri"])
    assert (a["report"] == e["report"]).all() and 0 < A <= SCENE_CAPS[1] and 0 < Tn <= SCENE_CAPS[2] and e["report"][3] <= SCENE_CAPS[0]
    assert (a["info"][:A] == e["info"]).all() and (a["rgba8"][:A].view(np.uint32) == e["rgba8"]).all() and (a["tri"][:Tn] == e["tri"]).all()
    assert bits(a["xyz"][:A]) == bits(e["xyz"]) and bits(a["normal"][:A]) == bits(e["normal"])
    # the CPU test's figures: the yardstick alone on scene(0.0), float32 grey -> depth_ref.depth_maps -> depth_ref.fuse -> mesh
    out = depth_ref.depth_maps(sc["gray"], None, 5, sc["P"], depth_ref.all_views(), [sc["range"]] * 5, depth_ref.SCENE_D, 2, 2, 10**6)
    f = depth_ref.fuse(out["depth"], depth_ref.all_views(), 5, sc["P"], 0.05, 2)
    cpu = ref.mesh(f["xyz"], f["src"], out["depth"], depth_ref.all_views(), 5, sc["P"], ref.CELL, ref.TRUTH_ORIGIN, band=2, trunc_cells=3,
                   agree=f["agree"], min_agree=2)
    trunc = 3 * ref.CELL
    fd = ref.truth_figures(dict(xyz=a["xyz"][:A], normal=a["normal"][:A], tri=a["tri"][:Tn]), ref.CELL, trunc)
    fc = ref.truth_figures(cpu, ref.CELL, trunc)
    print("device chain:", fd, "the yardstick alone:", fc)
    for k in ("vertices", "triangles", "near", "normals"):                   # the counts and the fractions; the grey differs by 1 / 65535
        assert fd[k] == fc[k], k
    want = ref.FLOORS["plain"]
    assert (fd["vertices"], fd["triangles"]) == want[:2] and fd["near"] >= want[2] and fd["normals"] >= want[3] and fd["worst"] <= want[4]
