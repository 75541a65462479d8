"""CPU tests (no GPU) of the yardstick of the mesh's decimation (tests/mesh_decimate_ref.py; include/pgx.h: pgx_mesh_decimate_dev):
its two forms agree bit for bit, the exact invariants of the rule, the exact special cases (a lattice plane, a nested failure,
negative coordinates, planted duplicates, lmin = lmax = 0), and the truth table of DESIGN.md section 31."""
import numpy as np
import pytest

import mesh_clean_ref as C
import mesh_decimate_ref as R
import mesh_ref

ARGS = R.OUT_KEYS
CELL, ORIGIN = R.CELL, R.ORIGIN


def both(m, cell=CELL, origin=ORIGIN, **kw):
    a = R.decimate(*(m[k] for k in ARGS), cell, origin, **kw)
    b = R.decimate_loop(*(m[k] for k in ARGS), cell, origin, **kw)
    R.assert_same(a, b)
    return a


def invariants(m, d, cell, origin, lmax):
    """what holds exactly for every input"""
    tri, rep, vm, lv = d["tri"], d["report"], d["vertex_map"], d["level"]
    nvo = len(d["xyz"])
    assert rep[5] == nvo and rep[6] == len(tri)
    if len(tri):
        assert tri.min() >= 0 and tri.max() < nvo
        assert (tri[:, 0] != tri[:, 1]).all() and (tri[:, 0] != tri[:, 2]).all() and (tri[:, 1] != tri[:, 2]).all()
        assert len(np.unique(tri, axis=0)) == len(tri)          # no two rows are equal
        assert (np.unique(tri.reshape(-1)) == np.arange(nvo)).all()   # every output vertex is in a triangle
    q, Q, info = d["q"], d["Q"], d["info"].astype(np.int64)
    L = info[:, 1]
    assert (info[:, 3] == 0).all() and (np.diff(info[:, 0]) > 0).all()   # in order of name
    assert ((Q >> (16 + L)[:, None]) == (q[info[:, 0]] >> (16 + L)[:, None])).all()   # Q lies in the block of the cluster's name
    mem = np.flatnonzero(vm >= 0)
    assert (lv[mem] == L[vm[mem]]).all() and ((lv >= 0) == (vm != -1)).all() and (lv <= lmax).all()
    assert (np.abs(q[mem] - Q[vm[mem]]) < (1 << (16 + L[vm[mem]]))[:, None]).all()   # no vertex moves by 2^L cells or more
    assert ((q[mem] >> (16 + lv[mem])[:, None]) == (Q[vm[mem]] >> (16 + lv[mem])[:, None])).all()   # every member in its cluster's block
    assert (np.bincount(vm[mem], minlength=nvo) <= info[:, 2]).all() and (vm[info[:, 0]] == np.arange(nvo)).all()
    o = np.asarray(origin, dtype=np.float64)
    assert R.bits(d["xyz"]) == R.bits(o + (Q.astype(np.float64) / 65536.0) * cell)
    nondeg = rep[4] + rep[6]
    assert 0 <= nondeg <= rep[2] <= rep[1] and rep[4] >= 0 and 0 <= rep[7] <= rep[6]   # used = degenerate + duplicates + kept
    # the kept triangles map through vertex_map onto the output rows, up to the rotation
    src = m["tri"][d["src_tri"]]
    mapped = vm[src]
    assert (np.sort(mapped, 1) == np.sort(tri, 1)).all() and (d["kept_tri"].sum() == len(tri))


SETTINGS = [dict(lmin=0, lmax=0), dict(lmin=1, lmax=1), dict(lmin=0, lmax=3, flat_q=1015), dict(lmin=0, lmax=6, flat_q=900),
            dict(lmin=2, lmax=4, flat_q=0), dict(lmin=6, lmax=6), dict(lmin=0, lmax=2, flat_q=1024)]


@pytest.mark.parametrize("kw", SETTINGS + [dict(lmin=0, lmax=2, counts=(60, 70)), dict(counts=(-3, 5)), dict(counts=(10**6, 10**6))],
                         ids=lambda kw: ",".join("%s=%s" % i for i in kw.items()))
def test_two_forms_agree_on_a_messy_mesh(kw):
    m = C.attrs(*C.messy())
    d = both(m, **kw)
    invariants(m, d, CELL, ORIGIN, kw.get("lmax", 3))
    if "counts" not in kw:
        assert d["report"][2] == 65


@pytest.mark.parametrize("kw", SETTINGS, ids=lambda kw: ",".join("%s=%s" % i for i in kw.items()))
def test_two_forms_agree_on_the_shapes(kw):
    for xyz, tri in (C.fan(50), C.strip(120, reverse=True), C.grid_plane(9, 7, jitter=0.3), C.grid_plane(17, 12, jitter=0.02),
                     C.islands([1, 2, 3] * 5)):
        m = C.attrs(xyz, tri)
        invariants(m, both(m, **kw), CELL, ORIGIN, kw["lmax"])
    both(C.attrs(np.zeros((0, 3)), np.zeros((0, 3))), **kw)
    both(C.attrs(np.ones((4, 3)), np.zeros((0, 3))), **kw)


@pytest.mark.parametrize("case", ["rotated-true", "rotated"])
def test_two_forms_agree_on_the_truth_meshes(case):
    m = R.cleaned_truth(case)
    for kw in (dict(lmin=1, lmax=1), dict(lmin=0, lmax=3, flat_q=1015)):
        d = both(m, mesh_ref.CELL, mesh_ref.TRUTH_ORIGIN, **kw)
        invariants(m, d, mesh_ref.CELL, mesh_ref.TRUTH_ORIGIN, kw["lmax"])


# ---- a lattice plane ----------------------------------------------------------------------------------------------------------------

def test_a_lattice_plane_passes_at_equality_and_keeps_its_coordinate():
    """every normal is exactly (0, 0, -1): m = (0, 0, -1024), S2 = 1024^2 N^2, flat at flat_q = 1024 with equality"""
    xyz, tri = C.grid_plane(33, 25)
    m = C.attrs(xyz, tri)
    for lmax in (1, 3, 6):
        d = both(m, lmin=0, lmax=lmax, flat_q=1024)
        assert (d["level"] == lmax).all()
        assert (d["xyz"][:, 2] == 3.0).all() and (d["normal"] == np.array([0, 0, -1], dtype=np.float32)).all()
        assert d["report"][7] == 0
    assert d["report"][6] == 0                                  # 33 x 25 cells lie in one level-6 block: nothing is left


def test_one_tilted_triangle_fails_exactly_its_ancestors():
    """vertex 0 of the lattice lifted by a quarter cell: the triangles that hold it are no longer axis-aligned; at flat_q = 1024
    exactly the blocks that hold one of those triangles' corners fail, at every level"""
    nx, ny = 33, 25
    xyz, tri = C.grid_plane(nx, ny)
    v = 12 * nx + 16
    xyz[v, 2] += 0.25 * CELL
    m = C.attrs(xyz, tri)
    d = both(m, lmin=0, lmax=3, flat_q=1024)
    q = d["q"]
    touched = np.unique(tri[(tri == v).any(1)].reshape(-1))
    lev = d["level"]
    for u in range(len(xyz)):
        want = 0
        for l in (1, 2, 3):
            if ((q[touched] >> (16 + l)) == (q[u] >> (16 + l))).all(1).any():
                break
            want = l
        assert lev[u] == want, (u, lev[u], want)
    assert (lev == 0).sum() > 0 and (lev == 3).sum() > 0 and (lev == 1).sum() > 0


def test_nested_failure_keeps_a_vertex_at_lmin():
    """a ridge whose two slopes cancel: inside one level-1 block the normals disagree (not flat), but the level-2 block round it
    holds so many flat triangles that it passes: the ridge's vertices stay at lmin all the same"""
    nx, ny = 17, 17
    xyz, tri = C.grid_plane(nx, ny)
    v = 8 * nx + 8
    xyz[v, 2] += 0.45 * CELL
    m = C.attrs(xyz, tri)
    fq = 1000
    d = both(m, lmin=0, lmax=2, flat_q=fq)
    # the flat flags of the blocks of v, from the rule by hand
    q, T = d["q"], tri
    mm = R._tri_m(q[T[:, 0]], q[T[:, 1]], q[T[:, 2]], 1024.0)

    def flat(l):
        inb = ((q[T] >> (16 + l)) == (q[v] >> (16 + l))).all(2)          # [t][3]
        N = int(inb.sum())
        S = (mm * inb.sum(1)[:, None]).sum(0)
        return int((S * S).sum()) >= fq * fq * N * N
    assert not flat(1) and flat(2)
    assert d["level"][v] == 0
    assert (d["level"] == 2).sum() > 0


def test_negative_coordinates_floor_not_truncate():
    """a lattice astride t = 0 on all three axes: the block of q < 0 is the floor; truncation would merge cells -1 and 0"""
    j, i = np.mgrid[0:8, 0:8]
    cell, origin = 0.5, (2.0, 1.0, 0.125)
    xyz = np.stack([origin[0] + (i - 4 + 0.5) * cell, origin[1] + (j - 4 + 0.5) * cell, origin[2] + (i - 4 + 0.5) * cell], -1).reshape(-1, 3)
    _, tri = C.grid_plane(8, 8)
    m = C.attrs(xyz, tri)
    d = both(m, cell, origin, lmin=1, lmax=1)
    assert all((d["q"][:, a] < 0).any() and (d["q"][:, a] > 0).any() for a in range(3))
    # blocks of two cells: (-4, -3), (-2, -1), (0, 1), (2, 3) per axis: 16 clusters of 4 members, none across t = 0
    assert d["report"][3] == 16 and (d["info"][:, 2] == 4).all()
    B = d["Q"] >> 17
    assert sorted(set(B[:, 0].tolist())) == [-2, -1, 0, 1] and (B[:, 2] == B[:, 0]).all()
    invariants(m, d, cell, origin, 1)


def test_planted_duplicates_are_dropped_and_opposite_windings_kept():
    xyz, tri = C.grid_plane(9, 9, jitter=0.2)
    xyz = xyz + 0.5 * CELL                                      # every vertex well inside a cell of its own
    tri = np.concatenate([tri, tri[5:8], tri[20:21][:, [1, 2, 0]], tri[30:32][:, [0, 2, 1]]])
    m = C.attrs(xyz, tri)
    d0 = both(dict(m, tri=tri[:128]), lmin=0, lmax=0)
    d = both(m, lmin=0, lmax=0)
    # one vertex per cell: no merge; the three copies and the rotated copy are duplicates, the two mirrored ones are not
    assert d0["report"][4] == 0 and d["report"][4] == 4 and d["report"][6] == d0["report"][6] + 2
    assert (d["src_tri"][-2:] == [132, 133]).all() and d["report"][7] == 0
    invariants(m, d, CELL, ORIGIN, 0)


def test_lmin_lmax_zero_merges_only_vertices_that_share_a_cell():
    t, mesh = C.truth_mesh("rotated-true")
    d = R.decimate(*(mesh[k] for k in ARGS), mesh_ref.CELL, mesh_ref.TRUTH_ORIGIN, lmin=0, lmax=0)
    vm, q = d["vertex_map"], d["q"]
    mem = np.flatnonzero(vm >= 0)
    cells = q[mem] >> 16
    _, inv = np.unique(cells, axis=0, return_inverse=True)
    inv = inv.reshape(-1)
    # the same cell <=> the same output vertex
    assert len(np.unique(np.stack([inv, vm[mem]], 1), axis=0)) == len(np.unique(inv)) == len(np.unique(vm[mem]))
    assert (d["level"][mem] == 0).all()


# ---- truth ------------------------------------------------------------------------------------------------------------------------
# case -> the cleaned input's triangles and distance, then per setting the triangles and the distance measured on the yardstick
# (the table of DESIGN.md section 31).  The bounds asserted beside the table's own figures: the adaptive setting leaves at most
# the measured ratio of the input's triangles plus 5 %; its distance is at or below the input's plus `margin`, which the table
# shows to be 0 (both settings lie below the input on both scenes); no extent shrinks by more than 2 x 2^lmax cells (rule 5: a
# rim vertex moves by less than a block, on either side).
UNIFORM, ADAPTIVE = dict(lmin=1, lmax=1), dict(lmin=0, lmax=3, flat_q=1015)
TRUTH = {"rotated-true": dict(input=(12692, 0.000516), uniform=(3204, 0.000496), adaptive=(773, 0.000370), margin=0.0),
         "rotated": dict(input=(14368, 0.010759), uniform=(3436, 0.010103), adaptive=(5585, 0.010215), margin=0.0)}


@pytest.mark.parametrize("case", ["rotated-true", "rotated"])
def test_truth_table(case):
    m = R.cleaned_truth(case)
    cell, org = mesh_ref.CELL, mesh_ref.TRUTH_ORIGIN
    d_in, n_in, e_in = R.plane_distance(m), len(m["tri"]), R.extent(m)
    rows = {}
    for name, kw in (("uniform", UNIFORM), ("adaptive", ADAPTIVE)):
        d = R.decimate(*(m[k] for k in ARGS), cell, org, **kw)
        rows[name] = (len(d["tri"]), R.plane_distance(d), R.extent(d), d["report"].tolist())
        print(case, name, len(d["tri"]), round(rows[name][1], 6), rows[name][2].round(4).tolist(), d["report"].tolist())
    print(case, "input", n_in, round(d_in, 6), e_in.round(4).tolist())
    want = TRUTH[case]
    assert want is not None, "the table is not filled in"
    assert n_in == want["input"][0] and abs(d_in - want["input"][1]) < 1e-6
    for name in ("uniform", "adaptive"):
        assert rows[name][0] == want[name][0] and abs(rows[name][1] - want[name][1]) < 1e-6   # the table's figures
    # fewer triangles by the measured ratio, less 5 %
    assert rows["adaptive"][0] <= n_in * min(1.0, want["adaptive"][0] / want["input"][0] * 1.05)
    assert rows["adaptive"][1] <= want["input"][1] + want["margin"]
    for name, lmax in (("uniform", 1), ("adaptive", 3)):
        assert (rows[name][2] >= e_in - 2 * (2**lmax) * cell).all()   # rule 5: a rim vertex moves by less than a block, on either side
