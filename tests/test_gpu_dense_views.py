"""GPU tests of the dense stage's plan (pgx_dense_views_dev / pgx_dense_views; include/pgx.h, k_denseviews.hip).  Every integer
output and every bit of d_range is held to the numpy yardstick of tests/dense_views_ref.py, at the smallest shapes that reach
each path of the kernels: the lane classes by track length and one past each boundary, more tracks than one sweep of each
grid, the LDS and the global form of the per-frame counts and of the pair counts, every frame and reference count, the source
choice and its ties, exact equality of the angle test, the radix select at every pass, every PGX_DVW_* bit, every report slot,
every refusal, and the chain triangulate -> dense views -> grey -> depth maps -> filter on one stream."""

import numpy as np
import pytest
import torch

import dense_views_ref as ref
import depth_ref
import photogrammetry_amd as pg
from dense_views_gpu import KEYS, buffers, call, dev, outputs, run
from geom_gpu import DEV, F64, I32, bits
from photogrammetry_amd import synth

pytestmark = pytest.mark.gpu

CONST = ref.kernel_constants()
NT, GRID, PGRID = CONST["DVW_NT"], CONST["DVW_GRID_MAX"], CONST["DVW_PAIR_GRID_MAX"]
LDS_FRAMES, LDS_CELLS = CONST["DVW_LDS_FRAMES"], CONST["DVW_LDS_CELLS"]
BIG = 2**30
PLANNED_FLOOR = 0.98      # tests/test_dense_views_ref.py measures 0.9924 and argues the margin


def check(engine, off, nd, xyz, flags, P, refs, S, max_tracks=None, max_nodes=None, **kw):
    """the device against plan(): every integer, every bit, and the status (the capacity is reported before a bad node)"""
    got = run(engine, off, nd, xyz, flags, P, refs, S, max_tracks, max_nodes, **kw)
    e = ref.plan(off, nd, xyz, flags, P, refs, S, max_tracks=max_tracks, max_nodes=max_nodes, **kw)
    ref.assert_equal(got, e, KEYS)
    assert got["status"] == ({"cap"} if "cap" in e["status"] else e["status"]), (got["status"], e["status"])
    return got, e


def graph_of_lengths(rng, nf, lens, spread=0.5):
    """tracks of exactly these lengths, frames drawn with repeats only where a track is longer than nf, points around the
    origin -> (offsets, nodes, xyz)"""
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    nd = np.zeros((off[-1], 2), dtype=np.int32)
    for t, L in enumerate(lens):
        nd[off[t]:off[t + 1], 0] = rng.permutation(nf)[:L] if L <= nf else rng.integers(0, nf, L)
    return off, nd, spread * rng.standard_normal((len(lens), 3))


def ring(nf, rng=None, radius=6.0, span=40.0):
    ang = np.linspace(-span, span, nf)
    return ref.arc_cameras(ang + (0 if rng is None else rng.uniform(-1, 1, nf)), radius=radius)


# ---- track lengths and grids ----------------------------------------------------------------------------------------------

def test_every_lane_class_and_its_boundaries(engine):
    """2 nodes; 8 | 9 and 32 | 33, the boundaries of the three lane classes; 64 | 65, one wave's lanes; 300 nodes (frames
    named many times: pairs in one frame are passed over); a track of one node and an empty one"""
    rng = np.random.default_rng(1)
    lens = [2, 8, 9, 32, 33, 64, 65, 300, 1, 0, 3, 16, 17, 31, 63]
    P = ring(40, rng)
    off, nd, xyz = graph_of_lengths(rng, 40, lens)
    got, e = check(engine, off, nd, xyz, None, P, None, 4, min_shared=1, min_points=1)
    assert e["report"][1] == len(lens) and e["report"][3] > 300 * 299 // 4
    assert 40 * 40 <= LDS_CELLS


def test_more_tracks_than_one_sweep_of_each_grid(engine):
    """each class has more tracks than the node kernels' grid (and so the pair kernel's smaller one) takes in one sweep"""
    rng = np.random.default_rng(2)
    n0, n1, n2 = GRID * NT // 4 + 300, GRID * NT // 16 + 100, GRID * NT // 64 + 50
    assert PGRID <= GRID
    lens = np.concatenate([rng.integers(2, 4, n0), rng.integers(9, 11, n1), rng.integers(33, 35, n2)])
    rng.shuffle(lens)
    P = ring(48, rng)
    off, nd, xyz = graph_of_lengths(rng, 48, lens)
    flags = (rng.random(len(lens)) < 0.05).astype(np.int32)
    got, e = check(engine, off, nd, xyz, flags, P, None, 8)
    assert (e["ref_stats"][:, 3] == 0).all() and e["report"][5] == 48


# ---- frame and reference counts ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("nf", [1, 2])
def test_one_and_two_frames(engine, nf):
    rng = np.random.default_rng(3)
    P = ring(nf) if nf > 1 else ring(2)[:1]
    off, nd, xyz = graph_of_lengths(rng, nf, [nf] * 20)
    got, e = check(engine, off, nd, xyz, None, P, None, 2, min_shared=1)
    assert (e["ref_stats"][:, 3] & ref.FEWVIEWS).all() and e["report"][6] == (0 if nf == 1 else 2)


@pytest.mark.parametrize("refs", [[3], None, [8, 2, 5, 0, 7, 1, 4, 3, 6], [4, 4, 1, 4], [6, 2], [9, -1, 100000, 2]],
                         ids=["one", "null", "permuted", "twice", "unknown", "outside"])
def test_reference_lists(engine, refs):
    off, nd, xyz, flags, P = ref.mixed_graph()        # frame 6 is unknown, frame 3 negated
    got, e = check(engine, off, nd, xyz, flags, P, refs, 3, min_shared=1, min_points=1)
    if refs == [4, 4, 1, 4]:
        for k in KEYS[:4]:
            assert bits(got[k][0]) == bits(got[k][1]) == bits(got[k][3])
    if refs in ([6, 2], [9, -1, 100000, 2]):
        bad = [r for r, f in enumerate(refs) if f != 2]
        assert (got["ref_stats"][bad] == [0, 0, 0, ref.NOCAMERA]).all() and np.isnan(got["range"][bad]).all()
        assert (got["views"][bad, 1:] == -1).all() and (got["pair_counts"][bad] == 0).all()
        assert (got["views"][:, 0] == refs).all()


# ---- capacity, bad nodes, and the two forms of both count tables ------------------------------------------------------------

@pytest.mark.parametrize("delta", [0, 7, -1])
def test_capacity(engine, delta):
    off, nd, xyz, flags, P = ref.mixed_graph()
    n = len(off) - 1
    got, e = check(engine, off, nd, xyz, flags, P, None, 3, max_tracks=n + delta)
    assert got["status"] == ({"cap"} if delta < 0 else set()) and got["report"][0] == min(n, n + delta)
    if delta > 0:
        ref.assert_equal(got, ref.plan(off, nd, xyz, flags, P, None, 3), KEYS)


def test_bad_nodes_and_malformed_offsets(engine):
    """a node in frame n_frames and one in frame -1 are skipped and reported; a last track whose end lies beyond max_nodes counts
    as empty and is reported"""
    off, nd, xyz, flags, P = ref.mixed_graph()
    nd = nd.copy()
    t = np.flatnonzero((flags == 0) & np.isfinite(xyz).all(1))
    nd[off[t[3]], 0], nd[off[t[5]] + 1, 0] = 9, -1
    got, e = check(engine, off, nd, xyz, flags, P, None, 3)
    assert got["status"] == {"node"}
    off2 = off.copy()
    off2[-1] += 5
    flags2 = flags.copy()
    flags2[-1] = 0
    xyz2 = xyz.copy()
    xyz2[-1] = 0.1
    got, e = check(engine, off2, ref.mixed_graph()[1], xyz2, flags2, P, None, 3, max_nodes=len(nd))
    assert got["status"] == {"node"}


@pytest.mark.parametrize("extra", [0, 1])
def test_pair_counts_in_lds_and_in_global_memory(engine, extra):
    """R n_frames at DVW_LDS_CELLS (the last size counted in LDS) and one row above it"""
    rng = np.random.default_rng(4)
    nf = int(np.sqrt(LDS_CELLS))
    assert nf * nf == LDS_CELLS
    P = ring(nf, rng, span=60.0)
    off, nd, xyz = graph_of_lengths(rng, nf, rng.integers(2, 40, 300))
    refs = list(rng.permutation(nf)) + [5] * extra
    got, e = check(engine, off, nd, xyz, None, P, refs, 8)
    assert len(refs) * nf == LDS_CELLS + extra * nf and e["report"][3] > 30000


@pytest.mark.parametrize("nf", [LDS_FRAMES, LDS_FRAMES + 1])
def test_frame_counts_in_lds_and_in_global_memory(engine, nf):
    """n_frames at DVW_LDS_FRAMES (per-frame counts and scatter cursors in LDS) and one above (global atomics), with a few
    references; the scan of the per-frame counts takes more than one round of the workgroup either way"""
    rng = np.random.default_rng(5)
    base = ring(32, rng)
    P = base[rng.integers(0, 32, nf)]
    off, nd, xyz = graph_of_lengths(rng, nf, rng.integers(2, 12, 2000))
    nd[:, 0] = np.where(rng.random(len(nd)) < 0.5, nd[:, 0] % 64, nd[:, 0])          # some frames with many nodes
    nd[:8, 0] = nf - 1
    refs = [0, 5, nf - 1, 63, 17]
    got, e = check(engine, off, nd, xyz, None, P, refs, 4, min_shared=2, min_points=4)
    assert (e["ref_stats"][:, 0] > 0).all()


# ---- the choice of the sources ----------------------------------------------------------------------------------------------

def tie_case():
    """frame 0 shares exactly 6 tracks with each of frames 1 .. 5, all at good angles but frame 5 (behind a too-wide angle:
    good 0), and 3 with frame 6"""
    P = ref.arc_cameras([0.0, 10.0, -10.0, 20.0, -20.0, 80.0, 15.0], radius=6.0)
    tracks = [[0, b] for b in (1, 2, 3, 4, 5) for _ in range(6)] + [[0, 6]] * 3
    off = np.concatenate([[0], np.cumsum([len(t) for t in tracks])]).astype(np.int32)
    nd = np.array([(f, 0) for t in tracks for f in t], dtype=np.int32)
    xyz = 0.05 * np.random.default_rng(6).standard_normal((len(tracks), 3))
    return off, nd, xyz, P


@pytest.mark.parametrize("S,min_shared", [(2, 1), (4, 1), (8, 1), (8, 6), (8, 7), (3, 0), (8, 0)])
def test_source_choice(engine, S, min_shared):
    off, nd, xyz, P = tie_case()
    got, e = check(engine, off, nd, xyz, None, P, [0, 6, 5], S, min_shared=min_shared, min_points=1)
    v = got["views"][0, 1:].tolist()
    order = [1, 2, 3, 4, 6, 5]                            # good 6 x 4 (ties to the smaller frame), good 3, good 0 shared 6
    if min_shared == 1:
        assert v == (order + [-1, -1])[:S]
    if min_shared == 6:
        assert v == [1, 2, 3, 4, 5, -1, -1, -1] and got["ref_stats"][0].tolist() == [33, 5, 5, ref.FEWVIEWS]
    if min_shared == 7:
        assert v == [-1] * 8 and got["ref_stats"][0, 1:].tolist() == [0, 0, ref.FEWVIEWS]
    if min_shared == 0:                                  # every other known frame is a candidate, shared or not
        assert got["ref_stats"][1, 1] == 6 and got["views"][1, 1] == 0


# ---- the angle test -----------------------------------------------------------------------------------------------------------

def exact_camera(R, C):
    """K [R | -R C] with K = [[512, 0, 256], [0, 512, 256], [0, 0, 1]], a signed permutation R and power-of-two centres: every
    entry, every cofactor and C = -(Minv p4) are exact"""
    K = np.array([[512.0, 0, 256.0], [0, 512.0, 256.0], [0, 0, 1.0]])
    R, C = np.asarray(R, dtype=np.float64), np.asarray(C, dtype=np.float64)
    return (K @ np.hstack([R, -(R @ C)[:, None]])).reshape(12)


def test_angle_equalities(engine):
    """X at the origin.  Frames 0 and 1 on one line through it (centres (0, 0, -2) and (0, 0, -4)): d d == na nb exactly, a good
    pair at min_angle_deg = 0 and not at any larger angle.  Frame 2 at (2, 0, 0), 90 degrees from frame 0: d == 0, not good.
    Frame 3 at (2, 0, 1), beyond 90 degrees: d < 0."""
    I3 = np.eye(3)
    Ry = [[0, 0, 1.0], [0, 1.0, 0], [-1.0, 0, 0]]          # looks along -x
    P = np.stack([exact_camera(I3, [0, 0, -2.0]), exact_camera(I3, [0, 0, -4.0]), exact_camera(Ry, [2.0, 0, 0]),
                  exact_camera(Ry, [2.0, 0, 1.0])])
    off, nd = np.array([0, 4], np.int32), np.array([(0, 0), (1, 0), (2, 0), (3, 0)], np.int32)
    xyz = np.zeros((1, 3))
    e0 = ref.plan(off, nd, xyz, None, P, None, 3, min_angle_deg=0.0, max_angle_deg=89.0, min_shared=1, min_points=1)
    assert e0["report"][2] == 4 and e0["pair_counts"][0].tolist() == [[0, 0], [1, 1], [1, 0], [1, 0]]
    got, _ = check(engine, off, nd, xyz, None, P, None, 3, min_angle_deg=0.0, max_angle_deg=89.0, min_shared=1, min_points=1)
    assert got["pair_counts"][0].tolist() == [[0, 0], [1, 1], [1, 0], [1, 0]]
    got, _ = check(engine, off, nd, xyz, None, P, None, 3, min_angle_deg=1e-3, max_angle_deg=89.0, min_shared=1, min_points=1)
    assert got["pair_counts"][0].tolist() == [[0, 0], [1, 0], [1, 0], [1, 0]]
    assert got["pair_counts"][2].tolist() == [[1, 0], [1, 0], [0, 0], [1, 1]]      # frames 2 and 3: 26.6 degrees


# ---- the order statistics -------------------------------------------------------------------------------------------------------

def depth_lists():
    """one list of depths per frame; frame f is [I | 0], so that z = X_z exactly"""
    rng = np.random.default_rng(7)
    one = np.float64(1.0).view(np.uint64)
    lists = [[2.0], [5.0, 3.0]]
    lists += [np.exp(rng.uniform(-3, 3, n)) for n in (255, 256, 257, 1001)]
    lists.append(np.full(300, 3.0))                                                     # equal depths
    lists.append((one + rng.permutation(400).astype(np.uint64)).view(np.float64))      # the lowest mantissa bits only
    for b in range(8):                                                                  # patterns that differ in byte b only
        base = np.uint64(0x3FF0000000000000) if b < 7 else np.uint64(0x00F0000000000000)
        lists.append((base ^ (rng.permutation(100 if b < 7 else 0x60).astype(np.uint64) << np.uint64(8 * b))).view(np.float64))
    lists.append(np.array([1e-300, 1e300, 1.0, 1e-300, 1e300]))
    lists.append(np.concatenate([np.full(700, 4.0), rng.uniform(1, 2, 30), rng.uniform(8, 9, 30)]))   # many equal, few apart
    return [np.asarray(z, dtype=np.float64) for z in lists]


@pytest.mark.parametrize("q", [(0, 1000), (500, 500), (1, 999)])
@pytest.mark.parametrize("grow", [1.0, 1.25, 1e10])
def test_order_statistics(engine, q, grow):
    lists = depth_lists()
    nf = len(lists)
    P = np.tile(np.hstack([np.eye(3), np.zeros((3, 1))]).reshape(12), (nf, 1))
    lens = np.concatenate([np.ones(len(z), int) for z in lists])
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    nd = np.array([(f, 0) for f, z in enumerate(lists) for _ in z], dtype=np.int32)
    xyz = np.zeros((len(nd), 3))
    xyz[:, 2] = np.concatenate(lists)
    order = np.random.default_rng(8).permutation(len(nd))                  # the lists interleaved
    nd, xyz = nd[order], xyz[order]
    assert all(np.isfinite(z).all() and (z > 0).all() for z in lists)
    got, e = check(engine, off, nd, xyz, None, P, None, 1, q_near_pm=q[0], q_far_pm=q[1], grow=grow, min_points=1)
    assert (e["ref_stats"][:, 0] == [len(z) for z in lists]).all()
    if grow == 1.0:
        assert e["ref_stats"][0, 3] & ref.NARROW and e["ref_stats"][6, 3] & ref.NARROW      # one depth; equal depths
        if q == (0, 1000):
            assert all(bits(e["range"][f]) == bits(np.array([z.min(), z.max()])) for f, z in enumerate(lists))
    if grow == 1e10 and q == (0, 1000):
        assert np.isinf(e["range"][-2, 1]) and not e["ref_stats"][-2, 3] & ref.NARROW and e["report"][4] == nf - 1


@pytest.mark.parametrize("delta", [0, 1])
def test_min_points_at_and_above_the_count(engine, delta):
    off, nd, xyz, flags, P = ref.mixed_graph()
    e0 = ref.plan(off, nd, xyz, flags, P, [2], 3)
    na = int(e0["ref_stats"][0, 0])
    got, e = check(engine, off, nd, xyz, flags, P, [2], 3, min_points=na + delta)
    assert bool(got["ref_stats"][0, 3] & ref.FEWPOINTS) == bool(delta) and np.isnan(got["range"][0]).all() == bool(delta)
    assert got["report"][4] == 1 - delta


# ---- outputs, refusals, repeatability, the host form -------------------------------------------------------------------------

def test_every_bit_and_every_report_slot(engine):
    """one call that shows NOCAMERA, FEWPOINTS, FEWVIEWS and NARROW and has every report slot different from the others"""
    off, nd, xyz, flags, P = ref.mixed_graph()
    n = len(off) - 1
    off = np.concatenate([off, [off[-1] + 1]]).astype(np.int32)            # one more track: the only node of a tenth frame
    nd = np.concatenate([nd, [(9, 0)]]).astype(np.int32)
    xyz, flags = np.concatenate([xyz, [[0.0, 0.0, 0.0]]]), np.concatenate([flags, [0]])
    P = np.concatenate([P, P[:1]])
    got, e = check(engine, off, nd, xyz, flags, P, [0, 6, 9, 1, 2], 3, min_points=1, grow=1.0, min_shared=30)
    st = e["ref_stats"][:, 3]
    assert st[1] == ref.NOCAMERA and st[2] == ref.FEWVIEWS | ref.NARROW and np.bitwise_or.reduce(st) & ref.FEWVIEWS
    got, e = check(engine, off, nd, xyz, flags, P, [0, 6, 9, 1, 2], 3, min_points=2, min_shared=1)
    assert e["ref_stats"][2, 3] == ref.FEWPOINTS | ref.FEWVIEWS
    r = e["report"]
    assert r[0] == n + 1 and r[0] > r[1] > 0 and r[2] > r[1] and r[3] > r[2] and r[4] == 3 and r[5] == 3 and r[6] == 3 and r[7] == 0


REFUSALS = [dict(S=0), dict(S=9), dict(R=0), dict(R=65536), dict(nf=0), dict(nf=65536), dict(max_tracks=-1), dict(max_nodes=-1),
            dict(min_angle_deg=-1.0), dict(min_angle_deg=10.0, max_angle_deg=10.0), dict(max_angle_deg=90.0),
            dict(min_angle_deg=float("nan")), dict(max_angle_deg=float("inf")), dict(min_shared=-1), dict(min_points=0),
            dict(q_near_pm=-1), dict(q_far_pm=1001), dict(q_near_pm=600, q_far_pm=500), dict(grow=0.99), dict(grow=float("inf")),
            dict(grow=float("nan")), dict(off=None), dict(nodes=None), dict(tsum=None), dict(xyz=None), dict(P=None), dict(views=None),
            dict(range=None), dict(ref_stats=None), dict(report=None), dict(refs=None, R=3), dict(alias=("report", "tsum")),
            dict(alias=("views", "nodes")), dict(alias=("range", "xyz")), dict(alias=("ref_stats", "off")),
            dict(alias=("pair_counts", "refs"))]


@pytest.mark.parametrize("how", REFUSALS, ids=lambda h: ",".join("%s=%s" % kv for kv in h.items()))
def test_refusals_write_nothing(engine, how):
    off, nd, xyz, flags, P = ref.mixed_graph()
    b = buffers(off, nd, xyz, flags, P, [1, 2, 3, 4], 3)
    before = outputs(b)
    kw = {}
    for k, v in how.items():
        if k == "alias":
            b[v[0]] = b[v[1]]
        elif k in b:
            b[k] = v
        else:
            kw[k] = v
    torch.cuda.synchronize()
    with pytest.raises(pg.ArgumentException):
        call(engine, b, **kw)
    engine.check_status()
    torch.cuda.synchronize()
    if "alias" not in how:      # an aliased output is an input: the inputs are the caller's
        after = outputs(b)
        for k in KEYS:
            assert after[k] is None or bits(before[k]) == bits(after[k]), k


def test_r_times_frames_above_the_limit_is_refused(engine):
    off, nd, xyz, flags, P = ref.mixed_graph()
    b = buffers(off, nd, xyz, flags, P, [1], 3)
    b.update(R=4097, nf=4096, refs=b["off"])            # 4097 * 4096 > 2^24: refused before anything is read
    with pytest.raises(pg.ArgumentException):
        call(engine, b)
    assert (b["report"].cpu().numpy() == 77).all()


def test_repeated_runs_and_a_used_workspace(engine):
    rng = np.random.default_rng(9)
    P = ring(20, rng)
    off, nd, xyz = graph_of_lengths(rng, 20, rng.integers(2, 21, 500))
    small = ref.mixed_graph()
    a = run(engine, off, nd, xyz, None, P, None, 4)
    run(engine, *small, None, 3)                                            # another graph through the same workspace
    b = run(engine, off, nd, xyz, None, P, None, 4)
    c = run(engine, off, nd, xyz, None, P, None, 4, pair_counts=False)
    for k in KEYS:
        assert bits(a[k]) == bits(b[k]), k
        assert c[k] is None or bits(a[k]) == bits(c[k]), k
    ref.assert_equal(a, ref.plan(off, nd, xyz, None, P, None, 4), KEYS)


def test_host_form(engine):
    off, nd, xyz, flags, P = ref.mixed_graph()
    refs = [4, 0, 6, 4]
    e = ref.plan(off, nd, xyz, flags, P, refs, 3, min_shared=1)
    h = engine.dense_views(off, nd, xyz, P, 3, refs=refs, track_flags=flags, **dict(ref.DEFAULTS, min_shared=1))
    ref.assert_equal(h, e, KEYS)
    d = run(engine, off, nd, xyz, flags, P, refs, 3, min_shared=1)
    for k in KEYS:
        assert bits(h[k]) == bits(d[k]), k
    h2 = engine.dense_views(off, nd, xyz, P, 3, refs=refs, track_flags=flags, pair_counts=False, ref_stats=False,
                            **dict(ref.DEFAULTS, min_shared=1))
    assert h2["pair_counts"] is None and h2["ref_stats"] is None
    for k in ("views", "range", "report"):
        assert bits(h2[k]) == bits(e[k]), k
    ref.assert_equal(engine.dense_views(off, nd, xyz, P, 2, **ref.DEFAULTS), ref.plan(off, nd, xyz, None, P, None, 2), KEYS)
    h0 = engine.dense_views(off, nd, xyz, P, 3, refs=[], **ref.DEFAULTS)
    assert (h0["report"] == 0).all() and len(h0["views"]) == 0
    with pytest.raises(pg.ArgumentException):                               # a node outside the frames: before any GPU work
        engine.dense_views(off, np.concatenate([[(99, 0)], nd[1:]]), xyz, P, 3, **ref.DEFAULTS)


# ---- the chain on the two-plane scene -------------------------------------------------------------------------------------------

def chain_run(engine, sync):
    """triangulate -> dense views -> grey -> depth maps -> filter on the scene's sparse model; sync: a check_status (a wait for
    the stream) behind every call instead of behind the last one only"""
    sc = depth_ref.scene()
    W, H, D, S = depth_ref.SCENE_W, depth_ref.SCENE_H, depth_ref.SCENE_D, 4
    X = ref.scene_points(sc, depth_ref.SCENE_CENTRES, W, H, depth_ref.SCENE_F)
    off, nd, _, kxy = ref.sparse_from_scene(sc, X)
    kps = []
    for k in kxy:
        a = np.zeros(len(k), dtype=pg.api.KEYPOINT_DTYPE)
        a["x"], a["y"] = k[:, 0], k[:, 1]
        kps.append(a)
    d = synth.device_tracks(kps, off, nd)
    n, nf, N = d["n_tracks"], 5, 5 * d["stride"]
    dP = dev(sc["P"], np.float64)
    g16 = np.round(sc["gray"].astype(np.float64) * 65535.0).astype(np.uint16)
    d_rgba = dev(np.stack([g16, g16, g16, np.full_like(g16, 65535)], -1), np.uint16)
    xyz, qual, tfl, tsum = torch.full((n, 3), 5.0, **F64), torch.full((n, 3), 5.0, **F64), torch.full((n,), 77, **I32), torch.full((8,), 77, **I32)
    views, rng, st, rep = torch.full((5, 1 + S), 77, **I32), torch.full((5, 2), 5.0, **F64), torch.full((5, 4), 77, **I32), torch.full((8,), 77, **I32)
    gray = torch.zeros((5, H, W), dtype=torch.float32, device=DEV)
    kq8, fl, msum = torch.full((5, H, W), 77, **I32), torch.full((5, H, W), 77, **I32), torch.full((8,), 77, **I32)
    dep = torch.full((5, H, W), 5.0, **F64)
    cap = 5 * H * W
    pts, src, fsum = torch.full((cap, 3), 5.0, **F64), torch.full((cap, 2), 77, **I32), torch.full((4,), 77, **I32)
    torch.cuda.synchronize()
    step = engine.check_status if sync else (lambda: None)
    engine.triangulate_tracks_dev(d["kp"], d["F"], d["stride"], nf, dP, d["off"], d["nodes"], d["tsum"], n, xyz, qual, tfl, tsum)
    step()
    engine.dense_views_dev(d["off"], d["nodes"], d["tsum"], n, N, xyz, nf, dP, 5, S, views, rng, st, rep, d_track_flags=tfl,
                           q_near_pm=0, q_far_pm=1000, grow=1.1)
    step()
    engine.gray_batch_dev(d_rgba, 5, W, H, gray)
    step()
    engine.depth_maps_dev(gray, 5, W, H, nf, dP, views, 5, S, rng, D, kq8, dep, fl, msum, agg_radius=2, min_views=2, max_cost=BIG)
    step()
    engine.depth_fuse_dev(dep, views, 5, S, W, H, nf, dP, cap, pts, src, fsum)
    engine.check_status()
    out = dict(xyz=xyz, tflags=tfl, views=views, range=rng, ref_stats=st, report=rep, kq8=kq8, flags=fl, depth=dep, points=pts,
               src=src, fsum=fsum, msum=msum)
    return sc, (off, nd), {k: v.cpu().numpy() for k, v in out.items()}


def test_chain_on_one_stream(engine):
    sc, (off, nd), a = chain_run(engine, sync=False)
    _, _, b = chain_run(engine, sync=True)
    for k in a:
        assert bits(a[k]) == bits(b[k]), k
    # the plan is the yardstick's of the device's own points
    e = ref.plan(off, nd, a["xyz"], a["tflags"], sc["P"], None, 4, q_near_pm=0, q_far_pm=1000, grow=1.1)
    ref.assert_equal(a, e, ("views", "range", "ref_stats", "report"))
    assert (a["ref_stats"][:, 3] == 0).all() and a["report"][4] == a["report"][5] == 5
    z = sc["ztrue"].reshape(5, -1)
    assert (a["range"][:, 0] <= z.min(1)).all() and (z.max(1) <= a["range"][:, 1]).all()
    ktrue = ref.planes_of(sc["ztrue"][0], a["range"][0, 0], a["range"][0, 1], depth_ref.SCENE_D)
    frac = depth_ref.within_one_plane(a["kq8"][:1], a["flags"][:1], ktrue[None])[0]
    print("chain: range %s, %.4f of the origin's pixels within one plane, %d points kept" % (a["range"][0], frac, a["fsum"][0]))
    assert frac >= PLANNED_FLOOR
    assert a["fsum"][0] > 0.5 * a["fsum"][1] > 0
