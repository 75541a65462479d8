"""CPU tests (no GPU) of the yardstick of the mesh's clean stage (tests/mesh_clean_ref.py; include/pgx.h: pgx_mesh_clean_dev): its
two forms agree bit for bit, the exact invariants of the rule, the exact special case (a regular grid plane does not move), the
planted floaters, and the truth table of DESIGN.md section 30."""
import numpy as np
import pytest

import mesh_clean_ref as R
import mesh_ref

ARGS = ("xyz", "normal", "rgba8", "info", "tri")


def both(m, cell=R.CELL, origin=R.ORIGIN, **kw):
    a = R.clean(*(m[k] for k in ARGS), cell, origin, **kw)
    b = R.clean_loop(*(m[k] for k in ARGS), cell, origin, **kw)
    R.assert_same(a, b)
    return a


@pytest.mark.parametrize("kw", [dict(), dict(min_tris=3), dict(min_tris=4, min_frac_pm=200), dict(min_frac_pm=201), dict(min_tris=2, iters=1),
                                dict(iters=3, lam=1.0, mu=0.0), dict(iters=2, lam=0.7, mu=-1.5), dict(min_tris=3, iters=6),
                                dict(iters=2, counts=(60, 70)), dict(counts=(-3, 5)), dict(counts=(10**6, 10**6), iters=1)])
def test_two_forms_agree_on_a_messy_mesh(kw):
    """NaN, infinite and out-of-range vertices, triangles with a repeated, a negative and a too-large index, bare vertices, and
    components of 1, 1, 2, 2, 3, 3, 5, 8 and 40 triangles: on both sides of min_tris = 3 and 4 and of 200 and 201 per mille of 40"""
    xyz, tri = R.messy()
    c = both(R.attrs(xyz, tri), **kw)
    if not kw:
        assert c["report"][3] == 9 and c["report"][7] == 40 and c["report"][2] == 65
    if kw == dict(min_tris=4, min_frac_pm=200):
        assert c["report"][4] == 2                              # 1000 * 5 < 200 * 40 = 1000 * 8: kept are 8 and 40
    if kw == dict(min_frac_pm=201):
        assert c["report"][4] == 1                              # 1000 * 8 < 201 * 40


def test_two_forms_agree_on_the_shapes():
    for xyz, tri in (R.fan(50), R.strip(120, reverse=True), R.grid_plane(7, 5, jitter=0.3), R.islands([1, 2, 3] * 5)):
        both(R.attrs(xyz, tri), iters=2)
        both(R.attrs(xyz, tri), min_tris=2)
    both(R.attrs(np.zeros((0, 3)), np.zeros((0, 3))))
    both(R.attrs(np.ones((4, 3)), np.zeros((0, 3))), iters=1)


def test_identity_parameters_return_the_used_triangles_bit_for_bit():
    xyz, tri = R.messy()
    m = R.attrs(xyz, tri)
    c = both(m)
    used = c["kept_tri"]
    assert c["report"][2] == used.sum() == c["report"][6] == len(c["tri"])
    vm = c["vertex_map"]
    inused = np.zeros(len(xyz), dtype=bool)
    inused[m["tri"][used].reshape(-1)] = True
    assert ((vm >= 0) == inused).all() and (vm[~inused] == -1).all()
    old = np.flatnonzero(vm >= 0)
    assert (vm[old] == np.arange(len(old))).all()               # ascending old index
    for k in ("xyz", "normal"):
        assert R.bits(c[k]) == R.bits(m[k][old])                # every bit copied
    for k in ("rgba8", "info"):
        assert (c[k] == m[k][old]).all()
    # vertex_map composed with the outputs reproduces the inputs: the triangles in order, the winding kept
    assert (c["tri"] == vm[m["tri"][used]]).all()
    assert (old[c["tri"]] == m["tri"][used]).all()
    assert c["tri"].max() < len(c["xyz"]) and c["tri"].min() >= 0


def test_dropped_components_and_indices():
    xyz, tri = R.messy()
    m = R.attrs(xyz, tri)
    c = both(m, min_tris=3, iters=2)
    assert c["tri"].min() >= 0 and c["tri"].max() < c["report"][5] == len(c["xyz"])
    vm, comp = c["vertex_map"], c["comp"]
    assert ((comp == -1) == (vm == -1)).all()
    full = R.clean(*(m[k] for k in ARGS), R.CELL, R.ORIGIN)
    size = np.bincount(full["comp"][m["tri"][full["kept_tri"]][:, 0]], minlength=len(vm))
    named = comp >= 0
    assert (vm[named & (size[comp.clip(0)] >= 3)] >= 0).all() and (vm[named & (size[comp.clip(0)] < 3)] == -2).all()
    for n in np.unique(comp[named]):
        assert n == np.flatnonzero(comp == n).min()             # a component is named by its smallest vertex


@pytest.mark.parametrize("iters,lam,mu", [(1, 1.0, 0.0), (3, 0.5, -0.53), (2, 0.33, -1.5)])
def test_a_regular_grid_plane_does_not_move(iters, lam, mu):
    """vertices on multiples of cell, every quad split along the same diagonal: the umbrella of an inner vertex is symmetric, so
    D = 0 exactly and every vertex at least 2 * iters rings from the rim keeps its q; its normal is exactly the plane's"""
    nx, ny = 4 * iters + 5, 4 * iters + 4
    xyz, tri = R.grid_plane(nx, ny)
    m = R.attrs(xyz, tri)
    c0 = both(m)
    c = both(m, iters=iters, lam=lam, mu=mu)
    j, i = np.mgrid[0:ny, 0:nx]
    inner = ((np.minimum(np.minimum(i, nx - 1 - i), np.minimum(j, ny - 1 - j))) >= 2 * iters).reshape(-1)
    assert inner.sum() >= 4
    assert (c["q"][inner] == c0["q"][inner]).all()
    assert (c["xyz"][inner] == xyz[inner]).all()                # multiples of cell: the fixed-point round trip is exact here
    assert (c["normal"][inner] == np.array([0, 0, -1], dtype=np.float32)).all()


def test_planted_floaters_vanish_and_nothing_else_changes():
    """the blobs round the planted points are components of a few triangles off the planes; with min_tris between their sizes
    and the surfaces' exactly they vanish"""
    t, m = R.planted_case()
    cell, org = mesh_ref.CELL, mesh_ref.TRUTH_ORIGIN
    full = R.clean(*(m[k] for k in ARGS), cell, org)
    comp = full["comp"]
    size = np.bincount(comp[m["tri"][:, 0]], minlength=len(comp))
    names = np.unique(comp[comp >= 0])
    small = [n for n in names if size[n] < 100]
    assert len(small) >= 2 and len(names) - len(small) == 2 and all(size[n] > 1000 for n in names if n not in small)
    for n in small:                                             # off the planes, at a planted point
        ctr = m["xyz"][comp == n].mean(0)
        assert min(np.linalg.norm(ctr - np.array(p)) for p in R.FLOATER_AT) < 3 * cell
        assert min(abs(ctr[2] - 3.0), abs(ctr[2] - 4.0)) > 0.5
    c = R.clean(*(m[k] for k in ARGS), cell, org, min_tris=100)
    blob_v = np.isin(comp, small)
    blob_t = blob_v[m["tri"][:, 0]]
    assert (c["vertex_map"][blob_v] == -2).all() and blob_t.sum() == sum(size[n] for n in small)
    keep_v = (comp >= 0) & ~blob_v
    assert (np.flatnonzero(c["vertex_map"] >= 0) == np.flatnonzero(keep_v)).all()
    for k in ("xyz", "normal"):
        assert R.bits(c[k]) == R.bits(m[k][keep_v])
    assert (c["rgba8"] == m["rgba8"][keep_v]).all() and (c["info"] == m["info"][keep_v]).all()
    assert (np.flatnonzero(keep_v)[c["tri"]] == m["tri"][~blob_t]).all()
    assert c["report"][4] == 2 and c["report"][3] == len(names)


# case -> at 20 iterations (the best row of the table of DESIGN.md section 30 for both scenes): the measured mean distance to the
# nearer plane before / after, the fraction of normals within 20 degrees before / after.  The floors are the measured fractions
# less 0.01, rounded down (mesh_ref.floor2).
TRUTH = {"plain": dict(mean=(0.03558, 0.03544), normals=(0.99760, 1.0)), "rotated": dict(mean=(0.01538, 0.01408), normals=(0.86844, 0.93209))}


@pytest.mark.parametrize("case", ["plain", "rotated"])
def test_truth_table(case):
    t, m = R.truth_mesh(case)
    cell, org = mesh_ref.CELL, mesh_ref.TRUTH_ORIGIN
    before = R.figures(m, cell)
    rows = {}
    for it in (0, 5, 20):
        c = R.clean(*(m[k] for k in ARGS), cell, org, min_tris=100, iters=it, lam=R.LAM, mu=R.MU)
        rows[it] = R.figures(c, cell)
        print(case, it, c["report"].tolist(), {k: (round(v, 5) if isinstance(v, float) else v) for k, v in rows[it].items()})
    print(case, "before", {k: (round(v, 5) if isinstance(v, float) else v) for k, v in before.items()})
    best, want = rows[20], TRUTH[case]
    assert abs(before["mean"] - want["mean"][0]) < 1e-5 and abs(best["mean"] - want["mean"][1]) < 1e-5   # the table's figures
    assert best["mean"] < before["mean"] and best["mean"] < rows[0]["mean"]
    assert best["normals"] >= mesh_ref.floor2(want["normals"][1]) and best["normals"] > before["normals"]
    # no shrinking: the extent of the kept vertices moves by less than a cell under the smoothing
    for it in (5, 20):
        assert (np.abs(rows[it]["extent"] - rows[0]["extent"]) < cell).all()
