"""GPU tests of the mesh's decimation (pgx_mesh_decimate_dev and the host form pgx_mesh_decimate; k_meshdecimate.hip) against
tests/mesh_decimate_ref.py: every integer output and every bit of the float outputs equals the yardstick's.  The shapes are small
vertex and triangle arrays built directly, the smallest at which the kernels can go wrong: the scan block, the grid, the LDS
table and the hashes are read from the kernel source (mesh_decimate_ref.kernel_constants).  Only the scene cases use mesh_ref's
meshes."""
import numpy as np
import pytest
import torch

import mesh_clean_ref as C
import mesh_decimate_ref as R
import mesh_ref
import photogrammetry_amd as pg
from mesh_gpu import DEV, dev
from photogrammetry_amd import _lib

pytestmark = pytest.mark.gpu

K = R.kernel_constants(_lib.CSRC)
NT, GRID, SLOTS, FLUSH_AT = K["MDC_NT"], K["MDC_GRID_MAX"], K["MDC_SLOTS"], K["MDC_FLUSH_AT"]
ARGS = R.OUT_KEYS
bits = R.bits
PAD = 3                                                        # sentinel rows behind every output
CELL, ORIGIN = R.CELL, R.ORIGIN


def yardstick(m, cell=CELL, origin=ORIGIN, **kw):
    return R.decimate(*(m[k] for k in ARGS), cell, origin, **kw)


def device_inputs(m):
    n, t = len(m["xyz"]), len(m["tri"])
    return (dev(m["xyz"] if n else np.zeros((1, 3)), np.float64), dev(m["normal"] if n else np.zeros((1, 3)), np.float32),
            dev(m["rgba8"].view(np.int32) if n else np.zeros(1), np.int32), dev(m["info"] if n else np.zeros((1, 4)), np.int32),
            dev(m["tri"] if t else np.zeros((1, 3)), np.int32))


def device_outputs(mv, mt, nv, optional=True):
    i32 = dict(dtype=torch.int32, device=DEV)
    o = dict(xyz=torch.full((mv + PAD, 3), 5.0, dtype=torch.float64, device=DEV), normal=torch.full((mv + PAD, 3), 5.0, dtype=torch.float32, device=DEV),
             rgba8=torch.full((mv + PAD,), 77, **i32), info=torch.full((mv + PAD, 4), 77, **i32), tri=torch.full((mt + PAD, 3), 77, **i32),
             report=torch.full((8,), 77, **i32))
    if optional:
        o["vertex_map"], o["level"] = torch.full((nv + PAD,), 77, **i32), torch.full((nv + PAD,), 77, **i32)
    return o


def host(o):
    h = {k: v.cpu().numpy() for k, v in o.items()}
    h["rgba8"] = h["rgba8"].view(np.uint32)
    return h


def run_dec(engine, m, caps, cell=CELL, origin=ORIGIN, counts=None, optional=True, check=True, d_counts=None, **kw):
    """pgx_mesh_decimate_dev on mesh m over sentinel-filled outputs of the capacities caps = (max_out_vertices, max_out_tris), one
    sync -> dict of host arrays (untrimmed) and err.  counts = (vertices, triangles) goes into slots 5 and 6 of a device report."""
    n, t = len(m["xyz"]), len(m["tri"])
    ins = device_inputs(m)
    o = device_outputs(caps[0], caps[1], n, optional)
    if counts is not None:
        d_counts = dev([9, 9, 9, 9, 9, counts[0], counts[1], 9], np.int32)
    torch.cuda.synchronize()
    engine.mesh_decimate_dev(*ins, d_counts, n, t, cell, origin, caps[0], caps[1], o["xyz"], o["normal"], o["rgba8"], o["info"], o["tri"],
                             o["report"], d_vertex_map=o.get("vertex_map"), d_level=o.get("level"), **kw)
    err = None
    try:
        engine.check_status()
    except pg.CapacityError as e:
        if check:
            raise
        err = e
    return dict(host(o), err=err)


def check_dec(got, e, caps):
    """the device's outputs against the yardstick's: the first min(count, capacity) rows, nothing behind them"""
    assert (got["report"] == e["report"]).all(), (got["report"], e["report"])
    mv, mt = min(len(e["xyz"]), caps[0]), min(len(e["tri"]), caps[1])
    assert (got["info"][:mv] == e["info"][:mv]).all(), np.argwhere(got["info"][:mv] != e["info"][:mv])[:5]
    assert (got["rgba8"][:mv] == e["rgba8"][:mv]).all()
    assert bits(got["xyz"][:mv]) == bits(e["xyz"][:mv]), np.argwhere(got["xyz"][:mv] != e["xyz"][:mv])[:5]
    assert bits(got["normal"][:mv]) == bits(e["normal"][:mv]), np.argwhere(got["normal"][:mv] != e["normal"][:mv])[:5]
    assert (got["tri"][:mt] == e["tri"][:mt]).all(), np.argwhere(got["tri"][:mt] != e["tri"][:mt])[:5]
    assert (got["xyz"][mv:] == 5.0).all() and (got["normal"][mv:] == 5.0).all() and (got["rgba8"][mv:] == 77).all()
    assert (got["info"][mv:] == 77).all() and (got["tri"][mt:] == 77).all()
    if "vertex_map" in got:
        nv = int(e["report"][0])
        for k in ("vertex_map", "level"):
            assert (got[k][:nv] == e[k]).all(), (k, np.argwhere(got[k][:nv] != e[k])[:5])
            assert (got[k][nv:] == 77).all()                    # rows >= nv are not written


def run_and_check(engine, m, caps=None, cell=CELL, origin=ORIGIN, counts=None, optional=True, **kw):
    e = yardstick(m, cell, origin, counts=counts, **kw)
    if caps is None:
        caps = (len(e["xyz"]) + 2, len(e["tri"]) + 2)
    got = run_dec(engine, m, caps, cell, origin, counts=counts, optional=optional, **kw)
    check_dec(got, e, caps)
    return got, e


mesh_of = C.attrs
SETTINGS = [dict(lmin=0, lmax=0), dict(lmin=1, lmax=1), dict(lmin=0, lmax=3, flat_q=1015), dict(lmin=0, lmax=6, flat_q=900),
            dict(lmin=2, lmax=4, flat_q=0), dict(lmin=6, lmax=6), dict(lmin=0, lmax=2, flat_q=1024), dict(lmin=5, lmax=6, flat_q=1000)]
IDS = lambda kw: ",".join("%s=%s" % i for i in kw.items())    # noqa: E731


# ---- 1 counts ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", [0, 1, NT - 1, NT, NT + 1])
def test_counts_round_the_scan_block(engine, n):
    """nv = nt = n on a jittered plane: the triangles that name a vertex at or past nv are not used"""
    m = mesh_of(*C.grid_plane(30, 20, jitter=0.3))
    got, e = run_and_check(engine, m, counts=(n, n), lmin=0, lmax=2, flat_q=900)
    assert e["report"][0] == n and e["report"][1] == n
    run_and_check(engine, m, counts=(n, 0), lmin=0, lmax=1)
    got, e = run_and_check(engine, m, counts=(len(m["xyz"]), n), lmin=1, lmax=1)
    assert n < 10 or e["report"][6] > 0


_BIG = []


def big_plane():
    if not _BIG:
        _BIG.append(mesh_of(*C.grid_plane(520, 520, jitter=0.3)))
    return _BIG[0]


@pytest.mark.parametrize("n", [GRID * NT - 1, GRID * NT, GRID * NT + 1])
def test_counts_round_one_pass_of_the_grid(engine, n):
    """one pass of the 1024-workgroup grid over the vertices and the triangles, and one item either side: at 262 145 the first
    workgroup of every kernel takes a second pass, and the one of the incidence pass carries its LDS table into it"""
    assert GRID * NT == 262144
    got, e = run_and_check(engine, big_plane(), counts=(n, n), lmin=0, lmax=1, flat_q=1000)
    assert e["report"][2] > 200000 and 0 < e["report"][6] < e["report"][2]


def test_counts_from_a_report_null_negative_and_above(engine):
    m = mesh_of(*C.islands([1, 2, 3] * 30))
    nv, nt = len(m["xyz"]), len(m["tri"])
    for counts, want in (((57, 33), (57, 33)), ((-1, -5), (0, 0)), ((10**6, 10**6), (nv, nt)), ((nv, -1), (nv, 0)), (None, (nv, nt))):
        got, e = run_and_check(engine, m, counts=counts, lmin=0, lmax=1)
        assert tuple(e["report"][:2]) == want


# ---- 2 the incidence pass and the tables ------------------------------------------------------------------------------------------

def test_a_fan_of_1000_in_one_block(engine):
    """every vertex of the fan lies in one level-5 block: with lmin = 4 every incidence of the 1001 triangles goes to one key of the
    LDS table, from four workgroups, and through their flushes into one entry"""
    m = mesh_of(*C.fan(1000))
    e = yardstick(m, lmin=4, lmax=5, flat_q=300)
    assert len(np.unique(e["q"] >> 21, axis=0)) == 1
    for kw in (dict(lmin=4, lmax=5, flat_q=300), dict(lmin=4, lmax=5, flat_q=1024), dict(lmin=0, lmax=6, flat_q=0), dict(lmin=0, lmax=0)):
        run_and_check(engine, m, **kw)


def test_more_blocks_than_the_lds_table_flushes_at(engine):
    """single triangles whose 3 x 256 corners per pass lie in blocks of their own: the table is flushed inside the pass, before the
    third corner, and goes on; the last workgroup has 7 triangles"""
    n = 5 * NT + 7
    xyz, tri = C.singles(n)
    m = mesh_of(xyz, tri)
    got, e = run_and_check(engine, m, cell=CELL / 4, lmin=0, lmax=1, flat_q=0)
    q = e["q"][tri[:NT].reshape(-1)] >> 17
    assert len(np.unique(q, axis=0)) == 3 * NT and 2 * NT > FLUSH_AT   # two corners of one pass alone pass the flush threshold
    assert e["report"][2] == n
    run_and_check(engine, m, cell=CELL / 4, lmin=0, lmax=3, flat_q=1000)


@pytest.mark.parametrize("l", [0, 1, 2, 3])
def test_probe_chains_that_collide_and_wrap(engine, l):
    """twelve blocks of level l whose keys hash into the last two entries of the table the device uses for these 24 vertices: the
    chains collide and wrap round the table's end.  lmin = lmax = l: the cluster table takes those keys.  lmin = l - 1: the level
    table fed by the incidence pass takes them too.  lmin = l - 2: they are parents, and k_mdc_up inserts them into the other
    level table"""
    lg = R.table_lg(24, K)
    assert lg == K["MDC_LG_TMIN"]
    last = {(1 << lg) - 1, (1 << lg) - 2}
    blocks = R.cells_hashing_to(l, lg, last, 12, K)
    rng = np.random.default_rng(l)
    xyz = []
    for b in blocks:                                            # two vertices a block: a cluster of two where the level is reached
        for _ in range(2):
            xyz.append(np.array(ORIGIN) + (np.array(b) * 2.0**l + rng.uniform(0.1, 0.9, 3) * 2.0**l) * CELL)
    tri = [[2 * i, 2 * ((i + 1) % 12), 2 * ((i + 5) % 12) + 1] for i in range(12)] + [[2 * i + 1, 2 * ((i + 3) % 12), 2 * ((i + 7) % 12)] for i in range(12)]
    m = mesh_of(np.array(xyz), tri)
    got, e = run_and_check(engine, m, lmin=l, lmax=l)
    assert e["report"][3] == 12
    B = np.unique(e["q"] >> (16 + l), axis=0)                   # the blocks the yardstick sees are the chosen ones: 12 keys, 2 homes
    assert len(B) == 12 and {R.table_hash(R.block_key(l, tuple(int(x) for x in b)), lg, K) for b in B} <= last
    for lmin in range(max(l - 2, 0), l):
        got, e = run_and_check(engine, m, lmin=lmin, lmax=l, flat_q=0)
        assert e["report"][3] == 12 and (e["level"] == l).all()


def triple_case():
    """30 vertices, one a cell, in cells whose keys have pairwise distinct home entries in the cluster table: every cluster's
    entry is then its home entry whatever the order of execution, and the yardstick's copy of the triple hash applies.  Of the
    rotated triples of those entries, twelve that hash to the last two entries of the triple table, and a rotated copy of each
    behind them in the list -> (mesh, entries [30], the twelve triples of vertex indices, lg of the triple table)"""
    nv, lgv = 30, R.table_lg(30, K)
    cells, homes = [], set()
    for b0 in range(40):
        for b1 in range(40):
            h = R.table_hash(R.block_key(0, (b0, b1, 0)), lgv, K)
            if h not in homes and len(cells) < nv:
                homes.add(h)
                cells.append((b0, b1, 0))
    assert len(cells) == nv
    entry = [R.table_hash(R.block_key(0, b), lgv, K) for b in cells]
    lgt = R.table_lg(24, K)
    last = {(1 << lgt) - 1, (1 << lgt) - 2}
    picked = []
    for i in range(nv):                                         # a vertex is its cluster's name: the rotated triple leads with the smallest index
        for j in range(i + 1, nv):
            for k in range(i + 1, nv):
                if k != j and len(picked) < 12 and R.triple_hash(entry[i], entry[j], entry[k], lgt, K) in last:
                    picked.append((i, j, k))
    assert len(picked) == 12
    xyz = np.array(ORIGIN) + (np.array(cells) + 0.5) * CELL
    tri = picked + [(j, k, i) for i, j, k in picked]            # the copies: the same triangles, turned
    return mesh_of(xyz, tri), entry, picked, lgt


def test_the_triple_table_collides_and_wraps_on_chosen_triples(engine):
    """twelve distinct triples in two home entries, 510 and 511, of a table of 512: the chain runs through the table's end to entry
    9, every triple but the first of an entry passes owners of other triples, and whatever the order of the claims at least ten of
    the twelve lie behind the wrap; so do the copies that find them there and lose to the smaller index"""
    m, entry, picked, lgt = triple_case()
    assert lgt == 9 and len(set(entry)) == 30
    homes = [R.triple_hash(entry[i], entry[j], entry[k], lgt, K) for i, j, k in picked]
    assert set(homes) <= {510, 511} and len(set(picked)) == 12
    got, e = run_and_check(engine, m, lmin=0, lmax=0)
    assert e["report"][3] == len(set(np.array(picked).reshape(-1).tolist())) >= 12   # a cluster per vertex in use, each at its home entry
    assert e["report"][4] == 12 and e["report"][6] == 12 and (e["src_tri"] == np.arange(12)).all()
    rev = dict(m, tri=np.ascontiguousarray(m["tri"][::-1]))     # the turned copies come first and are kept
    got, e = run_and_check(engine, rev, lmin=0, lmax=0)
    assert e["report"][4] == 12 and (e["src_tri"] == np.arange(12)).all()


# ---- 3 the parameters -------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kw", SETTINGS, ids=IDS)
def test_levels_and_thresholds(engine, kw):
    """a jittered plane of 33 x 21 vertices (more than one workgroup), a nearly flat one, and two islands beside them"""
    x1, t1 = C.grid_plane(33, 21, jitter=0.3)
    x3, t3 = C.grid_plane(40, 30, jitter=0.02, seed=5)
    x2, t2 = C.islands([7, 1])
    m = mesh_of(np.concatenate([x1, x2 + [0, 0, 1.0], x3 + [0, 0, 2.0]]), np.concatenate([t1, t2 + len(x1), t3 + len(x1) + len(x2)]))
    got, e = run_and_check(engine, m, **kw)
    if kw["lmin"] == 0 and kw["lmax"] > 0 and 0 < kw.get("flat_q", 1015) < 1024:
        assert len(np.unique(e["level"])) > 1


def test_a_lattice_plane_at_equality(engine):
    """flat_q = 1024: S2 = 1024^2 N^2 exactly; every vertex reaches lmax, every output vertex has the plane's coordinate"""
    m = mesh_of(*C.grid_plane(70, 45))
    for lmax in (1, 3):
        got, e = run_and_check(engine, m, lmin=0, lmax=lmax, flat_q=1024)
        assert (e["level"] == lmax).all() and (got["xyz"][:len(e["xyz"]), 2] == 3.0).all() and e["report"][6] > 0
    xyz = m["xyz"].copy()
    xyz[20 * 70 + 33, 2] += 0.25 * CELL                         # one tilted fan: its ancestors fail
    got, e = run_and_check(engine, dict(m, xyz=xyz), lmin=0, lmax=3, flat_q=1024)
    assert sorted(np.unique(e["level"]).tolist()) == [0, 1, 2, 3]


def test_every_kind_of_unused_triangle_and_invalid_vertex(engine):
    """NaN and infinite coordinates, t at -2^20 (valid), just below 2^20 (valid: q is clamped to the last cell) and at 2^20 (not); a
    repeated, a negative and a too-large index, a triangle on an invalid vertex, bare vertices"""
    m = mesh_of(*C.messy())
    for kw in SETTINGS:
        got, e = run_and_check(engine, m, **kw)
    assert e["report"][2] == 65 and (e["vertex_map"] == -1).sum() >= 8
    assert e["q"].max() == R.Q_MAX and e["q"].min() == -2**36


def test_all_vertices_in_one_cluster(engine):
    m = mesh_of(*C.grid_plane(20, 20, jitter=0.3))
    got, e = run_and_check(engine, m, lmin=6, lmax=6)
    assert e["report"][3] == 1 and e["report"][5] == 0 and e["report"][6] == 0 and (e["vertex_map"] == -2).all()
    got, e = run_and_check(engine, m, lmin=0, lmax=6, flat_q=0)
    assert e["report"][3] == 1 and e["report"][6] == 0 and (e["level"] == 6).all()


def test_duplicates_in_different_workgroups_and_opposite_windings(engine):
    xyz, tri = C.grid_plane(40, 40, jitter=0.2)
    xyz = xyz + 0.5 * CELL
    n = len(tri)
    assert n > 8 * NT
    tri = np.concatenate([tri, tri[:300][:, [1, 2, 0]], tri[100:130], tri[500:520][:, [0, 2, 1]]])
    m = mesh_of(xyz, tri)
    got, e = run_and_check(engine, m, lmin=0, lmax=0)
    assert e["report"][4] == 330 and e["report"][6] == n + 20
    got, e = run_and_check(engine, m, lmin=0, lmax=2, flat_q=1000)
    assert e["report"][4] >= 1
    rev = dict(m, tri=np.ascontiguousarray(tri[::-1]))          # the kept copy is now the one at the list's far end
    run_and_check(engine, rev, lmin=0, lmax=0)


# ---- 4 capacities, optional outputs, workspace, order ------------------------------------------------------------------------------

def test_each_output_capacity_at_the_count_and_either_side(engine):
    m = mesh_of(*C.grid_plane(30, 22, jitter=0.3))
    kw = dict(lmin=0, lmax=2, flat_q=950)
    e = yardstick(m, **kw)
    kv, kt = len(e["xyz"]), len(e["tri"])
    assert kv > 10 and kt > 10
    for caps in ((kv, kt), (kv + 1, kt + 1), (kv - 1, kt), (kv, kt - 1), (0, 0), (kv, 0), (0, kt)):
        got = run_dec(engine, m, caps, check=False, **kw)
        check_dec(got, e, caps)
        assert (got["err"] is not None) == (caps[0] < kv or caps[1] < kt), caps
    engine.check_status()                                        # the status was cleared by the read


def test_optional_outputs_null(engine):
    m = mesh_of(*C.messy())
    run_and_check(engine, m, optional=False, lmin=0, lmax=2)


def test_a_used_workspace_and_run_to_run(engine):
    small, large = mesh_of(*C.islands([5, 2, 7])), mesh_of(*C.grid_plane(60, 50, jitter=0.3))
    kw = dict(lmin=0, lmax=3, flat_q=980)
    a, e = run_and_check(engine, small, **kw)
    b, _ = run_and_check(engine, large, **kw)
    c, _ = run_and_check(engine, small, **kw)
    d, _ = run_and_check(engine, large, **kw)
    for k in ("xyz", "normal", "tri", "vertex_map", "level", "report"):
        assert bits(a[k]) == bits(c[k]) and bits(b[k]) == bits(d[k])


def test_a_permuted_triangle_list(engine):
    x1, t1 = C.grid_plane(30, 20, jitter=0.3)
    x2, t2 = C.islands([3, 1, 6])
    m = mesh_of(np.concatenate([x1, x2 + [0, 0, 1.0]]), np.concatenate([t1, t2 + len(x1)]))
    kw = dict(lmin=0, lmax=2, flat_q=950)
    a, ea = run_and_check(engine, m, **kw)
    p = np.random.default_rng(8).permutation(len(m["tri"]))
    b, eb = run_and_check(engine, dict(m, tri=np.ascontiguousarray(m["tri"][p])), **kw)
    for k in ("xyz", "normal", "rgba8", "info", "vertex_map", "level"):
        assert bits(a[k]) == bits(b[k])                         # the same vertices
    kt = len(ea["tri"])
    assert len(eb["tri"]) == kt and sorted(map(tuple, a["tri"][:kt])) == sorted(map(tuple, b["tri"][:kt]))   # the same set of rows


def test_host_form(engine):
    m = mesh_of(*C.messy())
    for kw in (dict(), dict(lmin=1, lmax=1), dict(lmin=0, lmax=6, flat_q=0)):
        e = yardstick(m, **kw)
        got = engine.mesh_decimate(*(m[k] for k in ARGS), CELL, ORIGIN, **kw)
        R.assert_same(got, e)
    got = engine.mesh_decimate(*(m[k] for k in ARGS), CELL, ORIGIN, vertex_map=False, level=False, lmin=0, lmax=0)
    assert got["vertex_map"] is None and got["level"] is None
    R.assert_same(got, yardstick(m, lmin=0, lmax=0), keys=R.OUT_KEYS + ("report",))
    with pytest.raises(pg.CapacityError):
        engine.mesh_decimate(*(m[k] for k in ARGS), CELL, ORIGIN, lmin=0, lmax=0, max_out_tris=10)
    empty = mesh_of(np.zeros((0, 3)), np.zeros((0, 3)))
    got = engine.mesh_decimate(*(empty[k] for k in ARGS), CELL, ORIGIN)
    assert (got["report"] == 0).all() and len(got["xyz"]) == 0 and len(got["tri"]) == 0


# ---- 5 refusals --------------------------------------------------------------------------------------------------------------------

def test_every_refusal(engine):
    m = mesh_of(*C.islands([3, 2]))
    n, t = len(m["xyz"]), len(m["tri"])
    ins = device_inputs(m)
    o = device_outputs(n, t, n)
    torch.cuda.synchronize()

    def call(ins=ins, counts=None, nv=n, nt=t, cell=CELL, origin=ORIGIN, mv=n, mt=t, out=None, **kw):
        x = dict(o, **(out or {}))
        engine.mesh_decimate_dev(*ins, counts, nv, nt, cell, origin, mv, mt, x["xyz"], x["normal"], x["rgba8"], x["info"], x["tri"],
                                 x["report"], d_vertex_map=x["vertex_map"], d_level=x["level"], **kw)
    call(lmin=0, lmax=0)                                         # the arguments below differ from a call that passes
    engine.check_status()
    before = host(o)
    bad = [dict(nv=-1), dict(nv=2**28 + 1), dict(nt=-1), dict(nt=2**28 + 1), dict(mv=-1), dict(mv=2**28 + 1), dict(mt=-1), dict(mt=2**28 + 1),
           dict(cell=0.0), dict(cell=-1.0), dict(cell=float("nan")), dict(cell=float("inf")), dict(origin=(0.0, float("nan"), 0.0)),
           dict(origin=(float("inf"), 0.0, 0.0)), dict(origin=(0.0, 0.0, float("-inf"))), dict(lmin=-1), dict(lmin=7, lmax=7),
           dict(lmin=2, lmax=1), dict(lmax=7), dict(flat_q=-1), dict(flat_q=1025)]
    for j in range(5):                                           # null required inputs, unless their capacity is 0
        bad.append(dict(ins=tuple(None if i == j else x for i, x in enumerate(ins))))
    for k in ("xyz", "normal", "rgba8", "info", "tri", "report"):
        bad.append(dict(out={k: None}))
    for j, k in ((0, "xyz"), (1, "normal"), (2, "rgba8"), (3, "info"), (4, "tri"), (4, "vertex_map"), (0, "level"), (3, "report")):
        bad.append(dict(out={k: ins[j]}))                        # an output on an input
    for kw in bad:
        with pytest.raises(pg.ArgumentException):
            call(**kw)
    torch.cuda.synchronize()
    after = host(o)
    for k in before:
        assert bits(before[k]) == bits(after[k]), k             # nothing written
    # what is allowed: null outputs with capacity 0, null inputs with capacity 0
    call(mv=0, out=dict(xyz=None, normal=None, rgba8=None, info=None), lmin=0, lmax=0)
    call(mt=0, out=dict(tri=None), lmin=0, lmax=0)
    call(ins=(None, None, None, None, ins[4]), nv=0)
    call(ins=ins[:4] + (None,), nt=0)
    with pytest.raises(pg.CapacityError):
        engine.check_status()


# ---- 6 behind the mesh and the clean stage, on one stream with one wait ------------------------------------------------------------

def test_behind_the_mesh_and_the_clean_stage_gives_the_tables_figures_and_again_through_the_report(engine):
    """pgx_mesh_dev -> pgx_mesh_clean_dev -> pgx_mesh_decimate_dev -> pgx_mesh_decimate_dev on solved_rotated()'s maps, each on the
    outputs and the report of the one before where they lie, one wait: the figures of the table of DESIGN.md section 31"""
    t, m = C.truth_mesh("rotated")
    cell, org = mesh_ref.CELL, mesh_ref.TRUTH_ORIGIN
    mc = R.cleaned_truth("rotated")
    e = R.decimate(*(mc[k] for k in ARGS), cell, org, lmin=0, lmax=3, flat_q=1015)
    e2 = R.decimate(*(e[k] for k in ARGS), cell, org, lmin=1, lmax=1)
    caps = (int(m["report"][3]) + 5, len(m["xyz"]) + 40, len(m["tri"]) + 40)
    xyz = np.asarray(t["xyz"], dtype=np.float64).reshape(-1, 3)
    R_, H, W = t["depth"].shape
    views = np.asarray(t["views"], dtype=np.int32).reshape(R_, -1)
    stages = [device_outputs(caps[1], caps[2], caps[1]) for _ in range(4)]
    dx, ds, dd, dv, dP = dev(xyz, np.float64), dev(t["src"], np.int32), dev(t["depth"], np.float64), dev(views, np.int32), dev(np.reshape(t["P"], (-1, 12)), np.float64)
    dag = dev(t["agree"], np.int32)
    torch.cuda.synchronize()
    a, b, c, d = stages
    engine.mesh_dev(dx, ds, None, len(xyz), dd, dv, R_, views.shape[1] - 1, W, H, 5, dP, cell, org, caps[0], caps[1], caps[2], a["xyz"],
                    a["normal"], a["rgba8"], a["info"], a["tri"], a["report"], d_agree=dag, min_agree=t["min_agree"], band=mesh_ref.TRUTH_BAND,
                    trunc_cells=mesh_ref.TRUTH_TRUNC)
    engine.mesh_clean_dev(a["xyz"], a["normal"], a["rgba8"], a["info"], a["tri"], a["report"], caps[1], caps[2], cell, org, caps[1], caps[2],
                          b["xyz"], b["normal"], b["rgba8"], b["info"], b["tri"], b["report"], min_tris=100, iters=5, lam=C.LAM, mu=C.MU)
    engine.mesh_decimate_dev(b["xyz"], b["normal"], b["rgba8"], b["info"], b["tri"], b["report"], caps[1], caps[2], cell, org, caps[1], caps[2],
                             c["xyz"], c["normal"], c["rgba8"], c["info"], c["tri"], c["report"], lmin=0, lmax=3, flat_q=1015,
                             d_vertex_map=c["vertex_map"], d_level=c["level"])
    engine.mesh_decimate_dev(c["xyz"], c["normal"], c["rgba8"], c["info"], c["tri"], c["report"], caps[1], caps[2], cell, org, caps[1], caps[2],
                             d["xyz"], d["normal"], d["rgba8"], d["info"], d["tri"], d["report"], lmin=1, lmax=1,
                             d_vertex_map=d["vertex_map"], d_level=d["level"])
    engine.check_status()                                        # the one wait
    got, got2 = host(c), host(d)
    check_dec(got, e, caps[1:])
    check_dec(got2, e2, caps[1:])
    kv, kt = len(e["xyz"]), len(e["tri"])
    dm = dict(xyz=got["xyz"][:kv], tri=got["tri"][:kt])
    assert kt == 5585 and abs(R.plane_distance(dm) - 0.010215) < 1e-6   # the adaptive row of `rotated`
    assert e2["report"][0] == kv and e2["report"][1] == kt and 0 < e2["report"][6] < kt
