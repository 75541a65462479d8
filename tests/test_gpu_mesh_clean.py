"""GPU tests of the mesh's clean stage (pgx_mesh_clean_dev and the host form pgx_mesh_clean; k_meshclean.hip) against
tests/mesh_clean_ref.py: every integer output and every bit of the float outputs equals the yardstick's.  The shapes are small
vertex and triangle arrays built directly, the smallest at which the kernels can go wrong: the scan block and the two grids are
read from the kernel source (mesh_clean_ref.kernel_constants).  Only the scene cases use mesh_ref's meshes."""
import numpy as np
import pytest
import torch

import mesh_clean_ref as R
import mesh_ref
import photogrammetry_amd as pg
from mesh_gpu import DEV, dev
from photogrammetry_amd import _lib

pytestmark = pytest.mark.gpu

K = R.kernel_constants(_lib.CSRC)
NT, GRID, UGRID, LONG = K["MCL_NT"], K["MCL_GRID_MAX"], K["MCL_UNION_GRID"], K["MCL_LONG_ROW"]
ARGS = ("xyz", "normal", "rgba8", "info", "tri")
bits = R.bits
PAD = 3                                                        # sentinel rows behind every output


def yardstick(m, cell=R.CELL, origin=R.ORIGIN, **kw):
    return R.clean(*(m[k] for k in ARGS), cell, origin, **kw)


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
        o["vertex_map"], o["comp"] = torch.full((nv + PAD,), 77, **i32), torch.full((nv + PAD,), 77, **i32)
    return o


def host(o):
    h = {k: v.cpu().numpy() for k, v in o.items()}
    h["rgba8"] = h["rgba8"].view(np.uint32)
    return h


def run_clean(engine, m, caps, cell=R.CELL, origin=R.ORIGIN, counts=None, optional=True, check=True, d_counts=None, **kw):
    """pgx_mesh_clean_dev on mesh m over sentinel-filled outputs of the capacities caps = (max_out_vertices, max_out_tris), one sync
    -> dict of host arrays (untrimmed) and err.  counts = (vertices, triangles) goes into slots 5 and 6 of a device report."""
    n, t = len(m["xyz"]), len(m["tri"])
    ins = device_inputs(m)
    o = device_outputs(caps[0], caps[1], n, optional)
    if counts is not None:
        d_counts = dev([9, 9, 9, 9, 9, counts[0], counts[1], 9], np.int32)
    torch.cuda.synchronize()
    engine.mesh_clean_dev(*ins, d_counts, n, t, cell, origin, caps[0], caps[1], o["xyz"], o["normal"], o["rgba8"], o["info"], o["tri"],
                          o["report"], d_vertex_map=o.get("vertex_map"), d_comp=o.get("comp"), **kw)
    err = None
    try:
        engine.check_status()
    except pg.CapacityError as e:
        if check:
            raise
        err = e
    return dict(host(o), err=err)


def check_clean(got, e, caps):
    """the device's outputs against the yardstick's: the first min(count, capacity) rows, nothing behind them"""
    assert (got["report"] == e["report"]).all(), (got["report"], e["report"])
    mv, mt = min(len(e["xyz"]), caps[0]), min(len(e["tri"]), caps[1])
    assert (got["info"][:mv] == e["info"][:mv]).all() and (got["rgba8"][:mv] == e["rgba8"][:mv]).all()
    assert bits(got["xyz"][:mv]) == bits(e["xyz"][:mv]), np.argwhere(got["xyz"][:mv] != e["xyz"][:mv])[:5]
    assert bits(got["normal"][:mv]) == bits(e["normal"][:mv]), np.argwhere(got["normal"][:mv] != e["normal"][:mv])[:5]
    assert (got["tri"][:mt] == e["tri"][:mt]).all(), np.argwhere(got["tri"][:mt] != e["tri"][:mt])[:5]
    assert (got["xyz"][mv:] == 5.0).all() and (got["normal"][mv:] == 5.0).all() and (got["rgba8"][mv:] == 77).all()
    assert (got["info"][mv:] == 77).all() and (got["tri"][mt:] == 77).all()
    if "vertex_map" in got:
        nv = int(e["report"][0])
        for k in ("vertex_map", "comp"):
            assert (got[k][:nv] == e[k]).all(), (k, np.argwhere(got[k][:nv] != e[k])[:5])
            assert (got[k][nv:] == 77).all()                    # rows >= nv are not written


def run_and_check(engine, m, caps=None, cell=R.CELL, origin=R.ORIGIN, counts=None, optional=True, **kw):
    e = yardstick(m, cell, origin, counts=counts, **kw)
    if caps is None:
        caps = (len(e["xyz"]) + 2, len(e["tri"]) + 2)
    got = run_clean(engine, m, caps, cell, origin, counts=counts, optional=optional, **kw)
    check_clean(got, e, caps)
    return got, e


def mesh_of(xyz, tri, seed=0):
    return R.attrs(xyz, tri, seed)


# ---- 1 counts ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", [0, 1, NT - 1, NT, NT + 1])
def test_counts_round_the_scan_block(engine, n):
    """nv = nt = n on a mesh of 300 small components: the triangles that name a vertex at or past nv are not used"""
    m = mesh_of(*R.islands([1, 2, 3] * 100))
    got, e = run_and_check(engine, m, counts=(n, n), iters=1)
    assert e["report"][0] == n and e["report"][1] == n and (n < 10 or e["report"][6] > 0)
    run_and_check(engine, m, counts=(n, 0))
    run_and_check(engine, m, counts=(len(m["xyz"]), n), min_tris=2)


@pytest.mark.parametrize("n", [UGRID * NT - 1, UGRID * NT, UGRID * NT + 1, GRID * NT - 1, GRID * NT, GRID * NT + 1])
def test_counts_round_one_pass_of_the_grids(engine, n):
    """one pass of the 256-workgroup grid of the union and the count, and of the 1024-workgroup grid of the other kernels, and one
    item either side; the n triangles are ONE component: at 262 145 it spans every workgroup of the count and five of its
    passes, so its sum goes through the LDS table across passes and through one flush per workgroup"""
    assert UGRID * NT == 65536 and GRID * NT == 262144
    got, e = run_and_check(engine, big_plane(), counts=(n, n), iters=1)
    assert e["report"][3] == 1 and e["report"][7] == n and e["report"][6] == n


_BIG = []


def big_plane():
    if not _BIG:
        _BIG.append(mesh_of(*R.grid_plane(520, 520, jitter=0.3)))
    return _BIG[0]


def test_counts_from_a_report_null_negative_and_above(engine):
    m = mesh_of(*R.islands([1, 2, 3] * 30))
    nv, nt = len(m["xyz"]), len(m["tri"])
    for counts, want in (((57, 33), (57, 33)), ((-1, -5), (0, 0)), ((10**6, 10**6), (nv, nt)), ((nv, -1), (nv, 0)), (None, (nv, nt))):
        got, e = run_and_check(engine, m, counts=counts, iters=1)
        assert tuple(e["report"][:2]) == want


# ---- 2 components ----------------------------------------------------------------------------------------------------------------

def test_a_workgroup_of_256_components_and_300_small_ones(engine):
    """512 triangles that are 512 components: every triangle of a workgroup inserts a root of its own into the LDS table, and the
    table of a workgroup that takes a second pass is flushed first; then 300 components of 1 to 3 triangles"""
    m = mesh_of(*R.islands([1] * 512))
    got, e = run_and_check(engine, m, iters=1)
    assert e["report"][3] == 512 and e["report"][7] == 1
    m = mesh_of(*R.islands([1, 2, 3] * 100))
    for kw in (dict(), dict(min_tris=2), dict(min_tris=3, iters=2), dict(min_tris=4)):
        got, e = run_and_check(engine, m, **kw)
    assert e["report"][3] == 300 and e["report"][4] == 0 and e["report"][5] == 0


def test_many_components_across_the_passes_of_the_count(engine):
    """more components than the LDS table has slots in every workgroup: 3 passes of the count's grid over single triangles"""
    n = 2 * UGRID * NT + 5 * NT + 7
    got, e = run_and_check(engine, mesh_of(*R.singles(n)), min_tris=1)
    assert e["report"][3] == n


@pytest.mark.parametrize("kw,kept", [(dict(min_tris=4), 5), (dict(min_tris=5), 4), (dict(min_tris=6), 3), (dict(min_frac_pm=249), 4),
                                    (dict(min_frac_pm=250), 4), (dict(min_frac_pm=251), 3), (dict(min_frac_pm=1000), 2),
                                    (dict(min_tris=21), 0), (dict(min_tris=20, min_frac_pm=1000), 2)])
def test_gates_at_equality_and_either_side_with_a_tie_for_big(engine, kw, kept):
    """components of 10, 20, 20, 5, 4 and 2 triangles: min_tris at 4, 5, 6; 1000 * 5 = 250 * 20; two components are big"""
    m = mesh_of(*R.islands([10, 20, 20, 5, 4, 2]))
    got, e = run_and_check(engine, m, iters=1, **kw)
    assert e["report"][7] == 20 and e["report"][3] == 6 and e["report"][4] == kept


def test_a_fan_of_1000_triangles_and_a_vertex_of_degree_1(engine):
    m = mesh_of(*R.fan(1000))
    deg = np.bincount(m["tri"].reshape(-1))
    assert deg[0] == 1000 and deg[-1] == 1
    for kw in (dict(iters=2), dict(iters=3, lam=1.0, mu=0.0), dict()):
        run_and_check(engine, m, **kw)


@pytest.mark.parametrize("n", [LONG - 1, LONG, LONG + 1, 2 * LONG, 2 * LONG + 1, 3 * LONG + 7])
def test_rows_round_the_long_row_threshold(engine, n):
    """a row of more than 64 entries is summed by its wave, 64 at a time: rows of 63 to 65, of two full rounds and one entry more;
    two hubs that are neighbours in one wave, the second long one way round and short the other"""
    for na, nb in ((n, 3 * LONG), (n, 5), (LONG + 3, n)):
        m = mesh_of(*R.twin_fans(na, nb))
        deg = np.bincount(m["tri"].reshape(-1))
        assert deg[0] == na and deg[1] == nb
        run_and_check(engine, m, iters=2)
    # a vertex capacity of 1: the second hub's long row is not summed for the normals, the first one's is
    e = yardstick(m, iters=1)
    got = run_clean(engine, m, (1, 0), check=False, iters=1)
    check_clean(got, e, (1, 0))
    assert got["err"] is not None


@pytest.mark.parametrize("reverse", [False, True])
def test_long_chains(engine, reverse):
    """a strip of 5000 triangles: the trees of the union-find grow deep; reversed, the smallest index, the component's name, is at
    the far end"""
    m = mesh_of(*R.strip(5000, reverse=reverse))
    got, e = run_and_check(engine, m, iters=2)
    assert e["report"][3] == 1 and e["report"][7] == 5000 and (e["comp"] == 0).all()
    # several strips one behind the other in the list, each numbered from its far end
    xs, ts, at = [], [], 0
    for i in range(6):
        x, t = R.strip(700 + i, reverse=True, seed=i)
        xs.append(x + [0, 0, i * R.CELL])
        ts.append(t + at)
        at += len(x)
    got, e = run_and_check(engine, mesh_of(np.concatenate(xs), np.concatenate(ts)), min_tris=703, iters=1)
    assert e["report"][3] == 6 and e["report"][4] == 3


def test_every_kind_of_unused_triangle_and_invalid_vertex(engine):
    """NaN and infinite coordinates, t at -2^20 (valid), just below 2^20 (valid) and at 2^20 (not); a repeated, a negative and a
    too-large index, a triangle on an invalid vertex, bare vertices"""
    m = mesh_of(*R.messy())
    for kw in (dict(), dict(iters=2), dict(min_tris=3, iters=1), dict(min_tris=2, min_frac_pm=200)):
        got, e = run_and_check(engine, m, **kw)
    e = yardstick(m)
    assert e["report"][2] == 65 and (e["vertex_map"] == -1).sum() >= 8


# ---- 3 smoothing and normals ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kw", [dict(iters=0), dict(iters=1), dict(iters=2), dict(iters=64), dict(iters=3, lam=1.0, mu=0.0),
                                dict(iters=2, lam=0.4, mu=-1.5), dict(iters=5, lam=1e-9, mu=-1e-9)],
                         ids=lambda kw: ",".join("%s=%s" % i for i in kw.items()))
def test_iterations_and_factors(engine, kw):
    """a jittered plane of 33 x 21 vertices (more than one workgroup) and two islands beside it"""
    x1, t1 = R.grid_plane(33, 21, jitter=0.3)
    x2, t2 = R.islands([7, 1])
    m = mesh_of(np.concatenate([x1, x2 + [0, 0, 1.0]]), np.concatenate([t1, t2 + len(x1)]))
    got, e = run_and_check(engine, m, min_tris=2, **kw)
    assert e["report"][4] == 2


def test_a_regular_grid_plane_does_not_move(engine):
    xyz, tri = R.grid_plane(21, 20)
    got, e = run_and_check(engine, mesh_of(xyz, tri), iters=4)
    j, i = np.mgrid[0:20, 0:21]
    inner = (np.minimum(np.minimum(i, 20 - i), np.minimum(j, 19 - j)) >= 8).reshape(-1)
    assert inner.sum() >= 4 and (got["xyz"][:len(xyz)][inner] == xyz[inner]).all()
    assert (got["normal"][:len(xyz)][inner] == np.array([0, 0, -1], dtype=np.float32)).all()


def test_a_tetrahedron_collapses_to_one_point_and_zero_normals(engine):
    """plain Laplacian: every vertex goes to the centroid of the other three; after twelve steps the four positions are one, every
    triangle has no area and contributes nothing, and every normal is zeros"""
    tx = np.array(R.ORIGIN) + np.array([[10, 10, 10], [13, 10, 10], [10, 13, 10], [10, 10, 13]]) * R.CELL
    m = mesh_of(tx, [[0, 2, 1], [0, 1, 3], [1, 2, 3], [0, 3, 2]])
    got, e = run_and_check(engine, m, iters=20, lam=1.0, mu=0.0)
    assert (e["xyz"] == e["xyz"][0]).all() and (e["normal"] == 0).all() and len(e["xyz"]) == 4
    run_and_check(engine, m, iters=3, lam=1.0, mu=0.0)


# ---- 4 capacities, optional outputs, workspace, order ------------------------------------------------------------------------------

def test_each_output_capacity_at_the_count_and_either_side(engine):
    m = mesh_of(*R.islands([3, 1, 40, 2, 9]))
    for kw in (dict(min_tris=2), dict(min_tris=2, iters=2)):
        e = yardstick(m, **kw)
        kv, kt = len(e["xyz"]), len(e["tri"])
        for caps in ((kv, kt), (kv + 1, kt + 1), (kv - 1, kt), (kv, kt - 1), (0, 0), (kv, 0), (0, kt)):
            got = run_clean(engine, m, caps, check=False, **kw)
            check_clean(got, e, caps)
            assert (got["err"] is not None) == (caps[0] < kv or caps[1] < kt), caps
    engine.check_status()                                        # the status was cleared by the read


def test_optional_outputs_null(engine):
    m = mesh_of(*R.messy())
    run_and_check(engine, m, optional=False, min_tris=2, iters=1)


def test_a_used_workspace_and_run_to_run(engine):
    small, large = mesh_of(*R.islands([5, 2, 7])), mesh_of(*R.grid_plane(60, 50, jitter=0.3))
    a, e = run_and_check(engine, small, min_tris=3, iters=2)
    b, _ = run_and_check(engine, large, iters=2)
    c, _ = run_and_check(engine, small, min_tris=3, iters=2)
    d, _ = run_and_check(engine, large, iters=2)
    for k in ("xyz", "normal", "tri", "vertex_map", "comp", "report"):
        assert bits(a[k]) == bits(c[k]) and bits(b[k]) == bits(d[k])


def test_a_permuted_triangle_list(engine):
    x1, t1 = R.grid_plane(30, 20, jitter=0.3)
    x2, t2 = R.islands([3, 1, 6])
    m = mesh_of(np.concatenate([x1, x2 + [0, 0, 1.0]]), np.concatenate([t1, t2 + len(x1)]))
    a, ea = run_and_check(engine, m, min_tris=2, iters=3)
    p = np.random.default_rng(8).permutation(len(m["tri"]))
    mp = dict(m, tri=np.ascontiguousarray(m["tri"][p]))
    b, eb = run_and_check(engine, mp, min_tris=2, iters=3)
    for k in ("xyz", "normal", "rgba8", "info", "vertex_map", "comp"):
        assert bits(a[k]) == bits(b[k])                         # the same vertices
    assert (eb["tri"] == ea["vertex_map"][m["tri"][p][ea["kept_tri"][p]]]).all()   # the same triangles in the new order


def test_host_form(engine):
    m = mesh_of(*R.messy())
    for kw in (dict(), dict(min_tris=3, iters=2), dict(min_tris=2, min_frac_pm=200, iters=1, lam=1.0, mu=0.0)):
        e = yardstick(m, **kw)
        got = engine.mesh_clean(*(m[k] for k in ARGS), R.CELL, R.ORIGIN, **kw)
        R.assert_same(got, e)
    got = engine.mesh_clean(*(m[k] for k in ARGS), R.CELL, R.ORIGIN, vertex_map=False, comp=False, iters=1)
    assert got["vertex_map"] is None and got["comp"] is None
    R.assert_same(got, yardstick(m, iters=1), keys=R.OUT_KEYS + ("report",))
    with pytest.raises(pg.CapacityError):
        engine.mesh_clean(*(m[k] for k in ARGS), R.CELL, R.ORIGIN, max_out_tris=10)
    empty = mesh_of(np.zeros((0, 3)), np.zeros((0, 3)))
    got = engine.mesh_clean(*(empty[k] for k in ARGS), R.CELL, R.ORIGIN, iters=1)
    assert (got["report"] == 0).all() and len(got["xyz"]) == 0 and len(got["tri"]) == 0


# ---- 5 refusals --------------------------------------------------------------------------------------------------------------------

def test_every_refusal(engine):
    m = mesh_of(*R.islands([3, 2]))
    n, t = len(m["xyz"]), len(m["tri"])
    ins = device_inputs(m)
    o = device_outputs(n, t, n)
    torch.cuda.synchronize()

    def call(ins=ins, counts=None, nv=n, nt=t, cell=R.CELL, origin=R.ORIGIN, mv=n, mt=t, out=None, **kw):
        x = dict(o, **(out or {}))
        engine.mesh_clean_dev(*ins, counts, nv, nt, cell, origin, mv, mt, x["xyz"], x["normal"], x["rgba8"], x["info"], x["tri"], x["report"],
                              d_vertex_map=x["vertex_map"], d_comp=x["comp"], **kw)
    call(iters=1)                                                # the arguments below differ from a call that passes
    engine.check_status()
    before = host(o)
    bad = [dict(nv=-1), dict(nv=2**28 + 1), dict(nt=-1), dict(nt=2**28 + 1), dict(mv=-1), dict(mv=2**28 + 1), dict(mt=-1), dict(mt=2**28 + 1),
           dict(cell=0.0), dict(cell=-1.0), dict(cell=float("nan")), dict(cell=float("inf")), dict(origin=(0.0, float("nan"), 0.0)),
           dict(origin=(float("inf"), 0.0, 0.0)), dict(origin=(0.0, 0.0, float("-inf"))), dict(min_tris=0), dict(min_frac_pm=-1),
           dict(min_frac_pm=1001), dict(iters=-1), dict(iters=65), dict(lam=0.0), dict(lam=1.0000001), dict(lam=float("nan")),
           dict(lam=-0.5), dict(mu=-1.5000001), dict(mu=1e-9), dict(mu=float("nan")), dict(mu=float("-inf")), dict(lam=float("inf"))]
    for j in range(5):                                           # null required inputs, unless their capacity is 0
        bad.append(dict(ins=tuple(None if i == j else x for i, x in enumerate(ins))))
    for k in ("xyz", "normal", "rgba8", "info", "tri", "report"):
        bad.append(dict(out={k: None}))
    for j, k in ((0, "xyz"), (1, "normal"), (2, "rgba8"), (3, "info"), (4, "tri"), (4, "vertex_map"), (0, "comp"), (3, "report")):
        bad.append(dict(out={k: ins[j]}))                        # an output on an input
    for kw in bad:
        with pytest.raises(pg.ArgumentException):
            call(**kw)
    torch.cuda.synchronize()
    after = host(o)
    for k in before:
        assert bits(before[k]) == bits(after[k]), k             # nothing written
    # what is allowed: null outputs with capacity 0, null inputs with capacity 0
    call(mv=0, out=dict(xyz=None, normal=None, rgba8=None, info=None))
    call(mt=0, out=dict(tri=None))
    call(ins=(None, None, None, None, ins[4]), nv=0)
    call(ins=ins[:4] + (None,), nt=0)
    with pytest.raises(pg.CapacityError):
        engine.check_status()


# ---- 6 behind the mesh, on one stream with one wait -------------------------------------------------------------------------------

def chain(engine, t, kw_mesh, kw_clean):
    """pgx_mesh_dev -> pgx_mesh_clean_dev on the mesh's own outputs and report, no host round trip between them"""
    cell, org = mesh_ref.CELL, mesh_ref.TRUTH_ORIGIN
    c = dict(xyz=t["xyz"], src=t["src"], depth=t["depth"], views=t["views"], P=t["P"])
    if "agree" in kw_mesh:
        c["agree"] = kw_mesh.pop("agree")
    e_mesh = mesh_ref.mesh(c["xyz"], c["src"], c["depth"], c["views"], 5, c["P"], cell, org, agree=c.get("agree"), **kw_mesh)
    caps = (int(e_mesh["report"][3]) + 5, len(e_mesh["xyz"]) + 40, len(e_mesh["tri"]) + 40)
    xyz = np.asarray(c["xyz"], dtype=np.float64).reshape(-1, 3)
    R_, H, W = c["depth"].shape
    views = np.asarray(c["views"], dtype=np.int32).reshape(R_, -1)
    i32 = dict(dtype=torch.int32, device=DEV)
    mo = dict(xyz=torch.full((caps[1], 3), 5.0, dtype=torch.float64, device=DEV), normal=torch.full((caps[1], 3), 5.0, dtype=torch.float32, device=DEV),
              rgba8=torch.full((caps[1],), 77, **i32), info=torch.full((caps[1], 4), 77, **i32), tri=torch.full((caps[2], 3), 77, **i32),
              report=torch.full((8,), 77, **i32))
    o = device_outputs(caps[1], caps[2], caps[1])
    dx, ds, dd, dv, dP = dev(xyz, np.float64), dev(c["src"], np.int32), dev(c["depth"], np.float64), dev(views, np.int32), dev(np.reshape(c["P"], (-1, 12)), np.float64)
    dag = None if c.get("agree") is None else dev(c["agree"], np.int32)
    torch.cuda.synchronize()
    engine.mesh_dev(dx, ds, None, len(xyz), dd, dv, R_, views.shape[1] - 1, W, H, 5, dP, cell, org, caps[0], caps[1], caps[2], mo["xyz"],
                    mo["normal"], mo["rgba8"], mo["info"], mo["tri"], mo["report"], d_agree=dag, **kw_mesh)
    engine.mesh_clean_dev(mo["xyz"], mo["normal"], mo["rgba8"], mo["info"], mo["tri"], mo["report"], caps[1], caps[2], cell, org, caps[1],
                          caps[2], o["xyz"], o["normal"], o["rgba8"], o["info"], o["tri"], o["report"], d_vertex_map=o["vertex_map"],
                          d_comp=o["comp"], **kw_clean)
    engine.check_status()                                        # the one wait
    got = host(o)
    e = R.clean(*(e_mesh[k] for k in ARGS), cell, org, **kw_clean)
    check_clean(got, e, caps[1:])
    kv, kt = len(e["xyz"]), len(e["tri"])
    return {k: got[k][:kv] for k in ("xyz", "normal", "rgba8", "info")} | dict(tri=got["tri"][:kt]), e, e_mesh


def test_behind_the_mesh_on_the_planted_floaters(engine):
    t, m = R.planted_case()
    got, e, e_mesh = chain(engine, t, dict(band=mesh_ref.TRUTH_BAND, trunc_cells=mesh_ref.TRUTH_TRUNC), dict(min_tris=100))
    assert e["report"][3] >= 4 and e["report"][4] == 2 and (e_mesh["report"] == m["report"]).all()
    assert (np.minimum(np.abs(got["xyz"][:, 2] - 3.0), np.abs(got["xyz"][:, 2] - 4.0)) < 0.5).all()   # what is left is on the planes


def test_behind_the_mesh_on_the_sweeps_maps_gives_the_tables_figures(engine):
    """solved_rotated()'s maps: the figures of the table of DESIGN.md section 30 at 20 iterations, from the device's mesh"""
    t, m = R.truth_mesh("rotated")
    got, e, e_mesh = chain(engine, t, dict(band=mesh_ref.TRUTH_BAND, trunc_cells=mesh_ref.TRUTH_TRUNC, agree=t["agree"], min_agree=t["min_agree"]),
                           dict(min_tris=100, iters=20, lam=R.LAM, mu=R.MU))
    f, before = R.figures(got, mesh_ref.CELL), R.figures(m, mesh_ref.CELL)
    print(f, before)
    assert abs(f["mean"] - 0.01408) < 1e-5 and abs(f["normals"] - 0.93209) < 1e-5 and f["vertices"] == 7633 and f["triangles"] == 14368
    assert f["mean"] < before["mean"] and f["normals"] >= mesh_ref.floor2(0.93209) and f["normals"] > before["normals"]
