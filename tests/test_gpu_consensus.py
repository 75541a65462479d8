"""GPU tests of track consensus (pgx_track_consensus_dev / pgx_track_consensus; include/pgx.h).  Every integer output --
offsets, nodes, summary, map, stats, flags, report, track_of -- is held to the numpy yardstick of tests/consensus_ref.py
exactly; the points to 1e-9 of the distance to the mean camera centre, and the keep set is derived again in numpy from the
device's own point.  Tracks the yardstick marks as near a threshold may be left out of the equality (at most 1 %; the scenes
here have none, the purpose-built exact cases are compared in full).  The cases: the planted scene as one chain on one
stream, every lane class and its boundaries, the exhaustive / sampled switch, late and tied winners, exact equality of the
predicate, mirrored and unknown cameras, every PGX_CNS_* outcome, the scan's limits, and bit-identical results across
layouts, capacities, runs and the host form."""
import os
import re

import numpy as np
import pytest
import torch

import consensus_ref as ref
import photogrammetry_amd as pg
from consensus_gpu import DEFAULTS, IN_SUMMARY, run
from geom_gpu import DEV, F64, I32, bits
from photogrammetry_amd import synth
from photogrammetry_amd._lib import PGX_DIST_NONE

pytestmark = pytest.mark.gpu

INT_KEYS = ("offsets", "nodes", "summary", "map", "flags", "stats", "report")
ALL_KEYS = INT_KEYS + ("xyz",)


def kernel_constant(name):
    src = open(os.path.join(os.path.dirname(pg.__file__), "csrc", "k_consensus.hip")).read()
    return int(re.search(r"constexpr int %s = (\d+);" % name, src).group(1))


def yardstick(kps, P, off, nodes, stride=None, track_of=None, in_summary=IN_SUMMARY, **kw):
    kw = dict(DEFAULTS, **kw)
    s = np.zeros(8, np.int32)
    s[2:8] = in_summary
    return ref.consensus(kps, P, off, nodes, in_summary=s, track_of=track_of, stride=stride, **kw)


def check(got, e, P, off, nodes, kps, inlier_px=4.0, exact_cases=False):
    """every integer output exact; xyz to 1e-9 of the distance to the mean camera centre; the keep set again from the
    device's own point.  Tracks near a threshold: at most 1 % (none in a purpose-built exact case, where all are compared)."""
    near = np.zeros(len(e["near"]), bool) if exact_cases else e["near"]
    assert near.mean() <= 0.01 if len(near) else True
    if not near.any():
        for k in INT_KEYS:
            assert np.array_equal(got[k], e[k]), (k, got[k], e[k])
        if e["track_of"] is not None:
            assert np.array_equal(got["track_of"], e["track_of"])
    else:
        assert np.array_equal(got["stats"][~near], e["stats"][~near])
    assert np.array_equal(np.isnan(got["xyz"]), np.isnan(e["xyz"]))
    known, M, _, C, sgn = ref.frames(P)
    P3 = np.asarray(P, np.float64).reshape(-1, 3, 4)
    old = np.flatnonzero(e["map"] >= 0)
    xy = [np.stack([k["x"], k["y"]], 1).astype(np.float64) if k.dtype.names else np.asarray(k, np.float64).reshape(-1, 2) for k in kps]
    for tn, t in enumerate(old):
        if near[t] or np.isnan(e["xyz"][tn]).any():
            continue
        nd = np.asarray(nodes)[off[t]:off[t + 1]]
        kn = np.array([0 <= f < len(known) and known[f] for f, _ in nd], bool)
        centre = C[nd[kn, 0]].mean(0)
        assert np.linalg.norm(got["xyz"][tn] - e["xyz"][tn]) <= 1e-9 * np.linalg.norm(e["xyz"][tn] - centre), t
        if exact_cases:
            continue      # a point on a threshold by construction: the yardstick's equality above is the check
        keep = np.ones(len(nd), bool)
        for i in np.flatnonzero(kn):
            f, k = nd[i]
            h = P3[f][:, :3] @ (got["xyz"][tn] - C[f])
            keep[i] = sgn[f] * h[2] > 0 and (h[0] - xy[f][k][0] * h[2]) ** 2 + (h[1] - xy[f][k][1] * h[2]) ** 2 <= (inlier_px * h[2]) ** 2
        assert np.array_equal(keep, e["keep"][off[t]:off[t + 1]]), t
    return e


def run_and_check(engine, kps, P, off, nodes, exact_cases=False, slots=None, n_slots=None, max_tracks=None, raises=None, **kw):
    d = synth.device_tracks(kps, off, nodes, slots=slots, n_slots=n_slots)
    got = run(engine, d, P, max_tracks=max_tracks, raises=raises, **kw)
    e = yardstick(kps, P, off, nodes, stride=d["stride"], **kw)
    check(got, e, P, np.asarray(off), nodes, kps, kw.get("inlier_px", 4.0), exact_cases)
    return got, e


# ---- the planted scene ------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def planted():
    s = synth.make_scene(1500, 12, seed=11)
    off, nodes, _ = synth.scene_tracks(s)
    bad, mask = ref.plant_swaps(s, off, nodes, 0.1, 11)
    return dict(s=s, off=off, nodes=bad, planted=mask, e=yardstick(s["kps"], s["P"], off, bad, track_of=None))


def graph_inputs(s, off, nodes):
    """match lists that link every track's consecutive nodes: pgx_tracks_dev rebuilds exactly these tracks"""
    stride = int(max(s["counts"]))
    rows = {}
    for t in range(len(off) - 1):
        nd = nodes[off[t]:off[t + 1]]
        for (a, ka), (b, kb) in zip(nd[:-1], nd[1:]):
            rows.setdefault((int(a), int(b)), []).append((int(ka), int(kb)))
    pairs = sorted(rows)
    m = np.zeros((len(pairs), stride, 3), np.int32)
    m[:, :, 2] = PGX_DIST_NONE
    for i, p in enumerate(pairs):
        for ka, kb in rows[p]:
            m[i, ka] = (ka, kb, 0)
    return pairs, m, stride


@pytest.mark.parametrize("follow", ["triangulate_ba", "register"])
def test_planted_scene_as_one_chain(engine, planted, follow):
    s, nf = planted["s"], 12
    pairs, m, stride = graph_inputs(s, planted["off"], planted["nodes"])
    lay = synth.slot_layout(s["kps"])
    N = nf * stride
    kp = torch.from_numpy(lay["kp"].view(np.int32).reshape(nf, stride, 4)).to(DEV)
    d_m, d_c = torch.from_numpy(m).to(DEV), torch.from_numpy(lay["counts"]).to(DEV)
    d_pl = torch.tensor(np.array(pairs, np.int32), **I32)
    track_of, off, nodes, tsum = torch.full((nf, stride), 7, **I32), torch.full((N + 1,), 7, **I32), torch.full((N, 2), 7, **I32), \
        torch.full((8,), 7, **I32)
    off2, nodes2, tsum2, report = torch.full((N + 1,), 7, **I32), torch.full((N, 2), 7, **I32), torch.full((8,), 7, **I32), \
        torch.full((8,), 7, **I32)
    tmap, stats = torch.full((N,), 7, **I32), torch.full((N, 4), 7, **I32)
    xyz, flags = torch.full((N, 3), 5.0, **F64), torch.full((N,), 7, **I32)
    dP, dK, dRt = (torch.from_numpy(np.ascontiguousarray(s[k])).to(DEV) for k in ("P", "K", "Rt"))
    q, tflags, tsumm = torch.zeros((N, 3), **F64), torch.zeros((N,), **I32), torch.zeros((8,), **I32)
    Rt_out, P_out, X_out = torch.zeros((nf, 12), **F64), torch.zeros((nf, 12), **F64), torch.zeros((N, 3), **F64)
    trace, rep2 = torch.zeros((6, 2), **F64), torch.zeros((8,), **I32)
    txyz = torch.zeros((N, 3), **F64)
    torch.cuda.synchronize()
    engine.tracks_dev(d_m, d_c, d_pl, len(pairs), nf, stride, nf, 0, 2, track_of, off, nodes, tsum)
    before = track_of.clone()
    engine.track_consensus_dev(kp, nf, stride, nf, dP, off, nodes, tsum, N, off2, nodes2, tsum2, tmap, xyz, flags, stats, report,
                               d_track_of=track_of, **DEFAULTS)
    if follow == "triangulate_ba":
        engine.triangulate_tracks_dev(kp, nf, stride, nf, dP, off2, nodes2, tsum2, N, txyz, q, tflags, tsumm, 0.0, 2.0, 10)
        fixed = torch.tensor([1, 1] + [0] * (nf - 2), **I32)
        engine.bundle_adjust_dev(kp, nf, stride, nf, dK, dRt, fixed, off2, nodes2, tsum2, N, txyz, Rt_out, P_out, X_out, trace, rep2,
                                 max_iters=5, d_track_flags=tflags)
    else:
        # registration directly on the consensus points: frame 6 is placed again from the other frames' tracks
        reg = torch.tensor([int(f == 6) for f in range(nf)], **I32)
        fstats, ferr = torch.zeros((nf, 4), **I32), torch.zeros((nf, 2), **F64)
        engine.register_frames_dev(kp, nf, stride, nf, dK, dRt, reg, off2, nodes2, tsum2, N, xyz, Rt_out, P_out, fstats, ferr, rep2,
                                   n_samples=128, inlier_px=4.0, min_inliers=12, refine_iters=10, seed=7, d_track_flags=flags)
    engine.check_status()                      # the one sync
    ts, ts2 = tsum.cpu().numpy(), tsum2.cpu().numpy()
    assert ts[0] == 1500 and ts2[0] == 1500 and ts[1] - ts2[1] == 150
    g_off, g_nodes = off.cpu().numpy()[:1501], nodes.cpu().numpy()[:ts[1]]
    e = ref.consensus(s["kps"], s["P"], g_off, g_nodes, in_summary=ts, track_of=before.cpu().numpy(), stride=stride, **DEFAULTS)
    got = dict(offsets=off2.cpu().numpy()[:1501], nodes=nodes2.cpu().numpy()[:ts2[1]], summary=ts2, map=tmap.cpu().numpy()[:1500],
               xyz=xyz.cpu().numpy()[:1500], flags=flags.cpu().numpy()[:1500], stats=stats.cpu().numpy()[:1500],
               report=report.cpu().numpy(), track_of=track_of.cpu().numpy())
    check(got, e, s["P"], g_off, g_nodes, s["kps"])
    assert list(got["report"][:7]) == [1500, 1500, ts[1], ts[1] - 150, 150, 0, 0]
    # exactly the planted observations went: as (frame, keypoint) sets, whatever the graph's order of tracks
    gone = set(map(tuple, g_nodes)) - set(map(tuple, got["nodes"]))
    assert gone == set(map(tuple, planted["nodes"][planted["planted"]]))
    assert (got["track_of"][tuple(np.array(sorted(gone)).T)] == -3).all() and (got["track_of"] == -3).sum() == 150
    if follow == "triangulate_ba":
        assert (tflags.cpu().numpy()[:1500] == 0).all()          # 1350 of 1500 without the stage
        r = rep2.cpu().numpy()
        assert r[4] == 1500 and r[2] in (1, 2, 3)
    else:
        assert fstats.cpu().numpy()[6, 3] == 0 and fstats.cpu().numpy()[6, 1] >= 100
        assert np.abs(Rt_out.cpu().numpy()[6] - s["Rt"][6]).max() < 1e-2


def test_bit_identical_across_layouts_capacity_runs_and_host_form(engine, planted):
    s, off, nodes = planted["s"], planted["off"], planted["nodes"]
    zero = (0,) * 6                             # the host form has no input summary
    d = synth.device_tracks(s["kps"], off, nodes)
    base = run(engine, d, s["P"], in_summary=zero)
    e = yardstick(s["kps"], s["P"], off, nodes, stride=d["stride"], in_summary=zero)
    check(base, e, s["P"], off, nodes, s["kps"])

    def same(x):
        for k in ALL_KEYS:
            assert bits(base[k]) == bits(x[k]), k
    same(run(engine, d, s["P"], in_summary=zero))                                   # a second run on the used workspace
    same(run(engine, d, s["P"], in_summary=zero, max_tracks=len(off) - 1 + 1000))  # a larger capacity
    slots = np.random.default_rng(0).permutation(15)[:12]
    same(run(engine, synth.device_tracks(s["kps"], off, nodes, slots=slots, n_slots=15), s["P"], in_summary=zero))
    same(run(engine, d, s["P"], in_summary=zero))                                   # ... and after other shapes used the workspace
    h = engine.track_consensus(s["kps"], s["P"], off, nodes, **DEFAULTS)
    same(h)
    # the rewritten track_of of a graph whose nodes are distinct
    to = np.full((12, d["stride"]), -1, np.int32)
    to[nodes[:, 0], nodes[:, 1]] = np.repeat(np.arange(len(off) - 1), np.diff(off))
    got = run(engine, d, s["P"], track_of=to)
    check(got, yardstick(s["kps"], s["P"], off, nodes, stride=d["stride"], track_of=to), s["P"], off, nodes, s["kps"])


# ---- lane classes -----------------------------------------------------------------------------------------------------

LENGTHS = (2, 3, 4, 5, 8, 9, 16, 17, 32, 33, 64, 65, 130, 300)


def lane_class_graph():
    """one clean track and one track per outlier position (first, last, and around every lane-group multiple 4, 8, 16, 32,
    64, 128) for every length, from a 300-frame scene"""
    s = synth.make_scene(40, 300, seed=3, arc_deg=120.0)
    off, nodes, pts = synth.scene_tracks(s)
    full = [t for t in range(len(off) - 1) if off[t + 1] - off[t] == 300]
    assert len(full) >= 4
    kp_of = [dict(zip(s["point_id"][f].tolist(), range(len(s["point_id"][f])))) for f in range(300)]
    tracks = []
    for L in LENGTHS:
        frames = np.unique(np.linspace(0, 299, L).round().astype(int))
        assert len(frames) == L
        cuts = sorted({p for g in (4, 16, 64) for b in (g, 2 * g) for p in (b - 1, b) if p < L} | {0, L - 1})
        for n, pos in enumerate([None] + cuts):
            p, q = pts[full[n % 3]], pts[full[3]]
            tr = [(int(f), kp_of[f][int(p)]) for f in frames]
            if pos is not None:
                tr[pos] = (tr[pos][0], kp_of[tr[pos][0]][int(q)])
            tracks.append(tr)
    o = np.cumsum([0] + [len(t) for t in tracks]).astype(np.int32)
    return s, o, np.array([n for t in tracks for n in t], np.int32)


@pytest.fixture(scope="module")
def lanes():
    return lane_class_graph()


@pytest.mark.parametrize("max_hyp", [512, 64])      # 512: exhaustive up to 32 nodes (496 pairs), sampled above
def test_every_lane_class_and_outlier_position(engine, lanes, max_hyp):
    s, off, nodes = lanes
    got, e = run_and_check(engine, s["kps"], s["P"], off, nodes, max_hyp=max_hyp, seed=5)
    n_k = e["stats"][:, 0]
    assert set(n_k.tolist()) == set(LENGTHS) and not e["near"].any()
    assert e["report"][4] > 50 and (e["stats"][n_k >= 4, 3] == 0).all()


def test_exhaustive_sampled_switch_and_sampled_winner(engine, lanes):
    s, off, nodes = lanes
    f12, f13 = np.arange(0, 300, 25)[:12], np.arange(0, 300, 23)[:13]
    scene_off, scene_nodes, pts = synth.scene_tracks(s)
    t0 = next(t for t in range(len(scene_off) - 1) if scene_off[t + 1] - scene_off[t] == 300)
    nd = scene_nodes[scene_off[t0]:scene_off[t0 + 1]]
    other = scene_nodes[scene_off[t0 + 1]:scene_off[t0 + 2]]
    tracks = []
    for fr in (f12, f13):
        tr = [tuple(nd[f]) for f in fr]
        wrong = dict(map(tuple, other)).get(int(fr[5]))
        assert wrong is not None
        bad = list(tr)
        bad[5] = (int(fr[5]), wrong)
        tracks += [tr, bad] * 4                 # the same tracks at several indices: the sampler depends on the index
    o = np.cumsum([0] + [len(t) for t in tracks]).astype(np.int32)
    n = np.array([x for t in tracks for x in t], np.int32)
    for seed in (1, 2):
        got, e = run_and_check(engine, s["kps"], s["P"], o, n, max_hyp=66, seed=seed)
        st = e["stats"]
        assert (st[:8, 0] == 12).all() and (st[8:, 0] == 13).all()
        assert len(set(st[0:8:2, 2].tolist())) == 1                # 66 pairs: exhaustive, the index does not matter
        if seed == 1:
            first = st.copy()
    assert (first[:8] == st[:8]).all() and (first[8:, 2] != st[8:, 2]).any()      # the seed matters only when sampled
    run_and_check(engine, s["kps"], s["P"], o, n, max_hyp=1, seed=3)
    run_and_check(engine, s["kps"], s["P"], off[:40], nodes[:off[39]], max_hyp=1, seed=3)


# ---- purpose-built cameras: exactly representable numbers -----------------------------------------------------------

def cam(C, f=128.0, back=False):
    """P [12] of an axis-aligned camera at the integer centre C with focal f and the principal point at 0; back: turned half
    a turn about x, looking along -z (R = diag(1, -1, -1))"""
    R = np.diag([1.0, -1.0, -1.0]) if back else np.eye(3)
    M = np.diag([f, f, 1.0]) @ R
    return np.concatenate([M, (-M @ np.asarray(C, float))[:, None]], 1).reshape(12)


def problem(cams, tracks):
    """tracks: lists of (frame, (u, v)) -> (kps per frame, P, offsets, nodes); every observation gets a keypoint of its own"""
    kps = [[] for _ in cams]
    nodes = []
    for tr in tracks:
        for f, uv in tr:
            nodes.append((f, len(kps[f])))
            kps[f].append(uv)
    kps = [np.array(k, np.int64).reshape(-1, 2) for k in kps]
    return kps, np.array(cams), np.cumsum([0] + [len(t) for t in tracks]).astype(np.int32), np.array(nodes, np.int32).reshape(-1, 2)


def test_exact_equality_of_the_predicate(engine):
    # cameras 0 and 1 see X = (2, 0, 8) exactly: a = c = 1.0625, b = 0.9375, den = 0.25, s = tt = 8, X' = (2, 0, 8).  Camera 2
    # at (2, 0, 0) sees it at (0, 0); its observation (3, 4) gives a' = -24, b' = -32, e' = 5 * 8: 576 + 1024 == 1600.
    # Camera 3 at (0, 0, 8) has the point in its principal plane: w == 0.  At 20 degrees only the pair (0, 1) is a hypothesis.
    cams = [cam((0, 0, 0)), cam((4, 0, 0)), cam((2, 0, 0)), cam((0, 0, 8))]
    tr = [(0, (32, 0)), (1, (-32, 0)), (2, (3, 4)), (3, (0, 0))]
    kps, P, off, nodes = problem(cams, [tr])
    got, e = run_and_check(engine, kps, P, off, nodes, exact_cases=True, inlier_px=5.0, min_parallax_deg=20.0)
    assert list(e["stats"][0]) == [4, 3, 0, 0] and e["near"][0]
    assert e["keep"].tolist() == [True, True, True, False] and (got["xyz"][0] == (2.0, 0.0, 8.0)).all()
    got, e = run_and_check(engine, kps, P, off, nodes, exact_cases=True, inlier_px=float(np.nextafter(5.0, 0.0)), min_parallax_deg=20.0)
    assert list(e["stats"][0]) == [4, 2, 0, 0] and e["keep"].tolist() == [True, True, False, False]
    # s == 0: ray j meets ray i in camera i's centre (b e == c dd == 10): no hypothesis, the track passes through
    kps, P, off, nodes = problem([cam((0, 0, 0)), cam((-4, 0, -8))], [[(0, (0, 0)), (1, (64, 0))]])
    got, e = run_and_check(engine, kps, P, off, nodes, exact_cases=True)
    assert list(e["stats"][0]) == [2, 0, -1, ref.LOWPARALLAX] and np.isnan(got["xyz"]).all() and got["flags"][0] == 1


def test_late_winner_and_tie(engine):
    # frames 0 .. 5 look along -z with parallel rays (den == 0 among them, s < 0 against the two good rays): only the last
    # pair (6, 7) is a hypothesis.  A second track of three consistent views: all three hypotheses tie at 3, h = 0 wins.
    cams = [cam((x, 0, 0), back=True) for x in (0, 1, -3, 1, 0, -3)] + [cam((-2, 0, 0)), cam((-1, 0, 0)), cam((5, 0, 0))]
    late = [(f, (0, 0)) for f in range(6)] + [(6, (64, 0)), (7, (48, 0))]
    tie = [(6, (64, 0)), (7, (48, 0)), (8, (-48, 0))]
    kps, P, off, nodes = problem(cams, [late, tie])
    got, e = run_and_check(engine, kps, P, off, nodes, exact_cases=True)
    assert list(e["stats"][0]) == [8, 2, 27, 0] and list(e["stats"][1]) == [3, 3, 0, 0]
    assert (got["xyz"] == (2.0, 0.0, 8.0)).all() and got["offsets"].tolist() == [0, 2, 5]


def test_every_outcome(engine):
    nan = np.full(12, np.nan)
    cams = [cam((0, 0, 0)), cam((4, 0, 0)), cam((8, 0, 0)), nan, cam((1, 0, 0), f=1024.0), nan]
    good = [(0, (32, 0)), (1, (-32, 0)), (2, (-96, 0))]                    # X = (2, 0, 8)
    fewviews = [(0, (32, 0)), (3, (5, 5)), (5, (6, 6))]                     # one known view
    lowpar = [(0, (32, 0)), (4, (128, 0))]                                  # 1 unit apart at depth 8, nearly parallel: gated at 10 deg
    nocons = [(0, (32, 0)), (1, (-32, 40)), (2, (-96, -90))]                # three rays that pass each other 2.5 units apart
    short = [(0, (32, 0)), (1, (-32, 0)), (2, (-96, 60))]                   # one outlier of three at min_len 3
    unknown = [(0, (32, 0)), (1, (-32, 0)), (2, (-96, 60)), (3, (1, 1)), (5, (2, 2))]   # ... kept by its unknown-frame nodes
    kps, P, off, nodes = problem(cams, [good, fewviews, lowpar, nocons, short, unknown])
    got, e = run_and_check(engine, kps, P, off, nodes, exact_cases=True, min_parallax_deg=10.0, min_inliers=2, min_len=3)
    assert e["stats"][:, 3].tolist() == [0, ref.FEWVIEWS, ref.LOWPARALLAX | ref.SHORT, ref.NOCONSENSUS, ref.SHORT, 0]
    assert got["map"].tolist() == [0, 1, -1, -1, -1, 2] and got["report"].tolist() == [6, 3, 19, 10, 2, 1, 2, 2]
    got, e = run_and_check(engine, kps, P, off, nodes, exact_cases=True, min_parallax_deg=10.0, min_inliers=3, min_len=2)
    assert e["stats"][:, 3].tolist() == [0, ref.FEWVIEWS, ref.LOWPARALLAX, ref.NOCONSENSUS, ref.NOCONSENSUS, ref.NOCONSENSUS]
    got, e = run_and_check(engine, kps, P, off, nodes, exact_cases=True, min_parallax_deg=10.0, min_inliers=2, min_len=2)
    assert e["stats"][:, 3].tolist() == [0, ref.FEWVIEWS, ref.LOWPARALLAX, ref.NOCONSENSUS, 0, 0]
    assert got["map"].tolist() == [0, 1, 2, -1, 3, 4] and got["flags"].tolist() == [0, 1, 1, 0, 0]
    assert np.diff(got["offsets"]).tolist() == [3, 3, 2, 2, 4] and got["report"].tolist() == [6, 5, 19, 14, 2, 1, 0, 2]
    got, e = run_and_check(engine, kps, P, off, nodes, exact_cases=True, min_parallax_deg=10.0, min_inliers=2, min_len=4)
    assert got["map"].tolist() == [-1, -1, -1, -1, -1, 0] and got["nodes"].tolist() == [[0, 5], [1, 3], [3, 1], [5, 1]]
    got, e = run_and_check(engine, kps, P, off, nodes, exact_cases=True, min_parallax_deg=10.0, min_inliers=2, min_len=0)
    assert (got["map"] >= 0).tolist() == [True, True, True, False, True, True]      # min_len < 1 counts as 1


def test_mirrored_and_unknown_cameras(engine, planted):
    s, off, nodes = planted["s"], planted["off"], planted["nodes"]
    # det M < 0 is read as the negative of a proper camera (the triangulation's depth rule): -P decides like P ...
    P = s["P"].copy()
    P[[2, 7]] = -P[[2, 7]]
    got, e = run_and_check(engine, s["kps"], P, off, nodes)
    assert (ref.frames(P)[4][[2, 7]] == -1).all()
    assert np.array_equal(e["stats"], planted["e"]["stats"]) and np.array_equal(e["keep"], planted["e"]["keep"])
    # ... and a mirrored K (fx < 0, u -> 1920 - u) has its points behind it: its observations go, the tracks stay
    P = s["P"].copy().reshape(12, 3, 4)
    kps = [k.copy() for k in s["kps"]]
    for f in (2, 7):
        P[f, 0] = 2.0 * 960.0 * P[f, 2] - P[f, 0]
        kps[f]["x"] = 1920 - kps[f]["x"]
    got, e = run_and_check(engine, kps, P.reshape(12, 12), off, nodes)
    assert (ref.frames(P.reshape(12, 12))[4][[2, 7]] == -1).all()
    assert not e["keep"][np.isin(nodes[:, 0], [2, 7])].any() and (e["map"] >= 0).all()
    # unknown cameras: NaN rows and det M == 0
    P = s["P"].copy()
    P[[1, 4, 5, 9, 10]] = np.nan
    P[7, :3] = 0.0
    got, e = run_and_check(engine, s["kps"], P, off, nodes, min_len=3)
    unknown = np.isin(nodes[:, 0], [1, 4, 5, 7, 9, 10])
    surv = np.repeat(e["map"] >= 0, np.diff(off))
    assert e["keep"][unknown].all() and set(map(tuple, nodes[unknown & surv])) <= set(map(tuple, got["nodes"]))
    assert (e["stats"][:, 3] == 0).sum() > 1000 and e["report"][4] > 20


# ---- the scan, capacity, empty and full removal -------------------------------------------------------------------------

def two_frame_graph(n):
    """n 2-node tracks over two frames; track t is pattern t % 7: consistent (kept) or 2.5 units apart (removed at 4 px).
    Every track has keypoints of its own (the slots behind the 7 patterns' keypoints repeat them)."""
    cams = [cam((0, 0, 0)), cam((4, 0, 0))]
    pat = np.array([1, 0, 1, 1, 0, 0, 1], bool)
    kp0 = np.tile([[32, 0]], (n, 1))
    kp1 = np.where(pat[np.arange(n) % 7][:, None], [[-32, 0]], [[-32, 40]])
    nodes = np.stack([np.tile([0, 1], n), np.repeat(np.arange(n), 2)], 1).astype(np.int32)
    return [kp0, kp1], np.array(cams), (2 * np.arange(n + 1)).astype(np.int32), nodes, pat[np.arange(n) % 7]


def expected_two_frame(n, keep, e7):
    """the yardstick's result for the first 7 tracks, tiled over n tracks"""
    tmap = np.where(keep, np.cumsum(keep) - 1, -1).astype(np.int32)
    nodes = np.stack([np.tile([0, 1], n), np.repeat(np.arange(n), 2)], 1).astype(np.int32)[np.repeat(keep, 2)]
    stats = e7["stats"][np.arange(n) % 7]
    k = int(keep.sum())
    return dict(offsets=(2 * np.arange(k + 1)).astype(np.int32), nodes=nodes, map=tmap, stats=stats,
                summary=np.array([k, 2 * k, 21, 22, 23, 2 if k else 0, 24, 0], np.int32), flags=np.zeros(k, np.int32),
                report=np.array([n, k, 2 * n, 2 * k, 0, n - k, 0, 0], np.int32), xyz=np.tile(e7["xyz"][0], (k, 1)))


def scan_sizes():
    items, nt = kernel_constant("CNS_SCAN_ITEMS"), kernel_constant("CNS_NT")
    assert items == nt * kernel_constant("CNS_SCAN_PER_THREAD")
    return [items - 1, items, items + 1, 2 * items + 1, nt * items + 1]     # the last: one more than a full block of block sums


@pytest.mark.parametrize("which", range(5))
def test_scan_limits(engine, which):
    n = scan_sizes()[which]
    kps, P, off, nodes, keep = two_frame_graph(n)
    e7 = yardstick(kps, P, off[:8], nodes[:14])
    assert (e7["map"] >= 0).tolist() == keep[:7].tolist() and (e7["stats"][~keep[:7], 3] == ref.NOCONSENSUS).all()
    got = run(engine, synth.device_tracks(kps, off, nodes), P)
    want = expected_two_frame(n, keep, e7)
    for k in INT_KEYS:
        assert np.array_equal(got[k], want[k]), k
    assert bits(got["xyz"]) == bits(want["xyz"])


def test_all_removed_nothing_removed_empty_and_capacity(engine, planted):
    kps, P, off, nodes, keep = two_frame_graph(700)
    bad = np.flatnonzero(~keep)
    o_bad = (2 * np.arange(len(bad) + 1)).astype(np.int32)
    n_bad = nodes.reshape(-1, 2, 2)[bad].reshape(-1, 2)
    got, e = run_and_check(engine, kps, P, o_bad, n_bad, exact_cases=True)          # every track removed
    assert got["summary"][:2].tolist() == [0, 0] and got["offsets"].tolist() == [0] and (got["map"] == -1).all()
    assert got["report"].tolist() == [len(bad), 0, 2 * len(bad), 0, 0, len(bad), 0, 0]
    good = np.flatnonzero(keep)
    o_good = (2 * np.arange(len(good) + 1)).astype(np.int32)
    n_good = nodes.reshape(-1, 2, 2)[good].reshape(-1, 2)
    got, e = run_and_check(engine, kps, P, o_good, n_good, exact_cases=True)        # nothing removed: the graph bit for bit
    assert bits(got["offsets"]) == bits(o_good) and bits(got["nodes"]) == bits(n_good)
    assert got["summary"].tolist() == [len(good), 2 * len(good), 21, 22, 23, 2, 24, 0]
    got = run(engine, synth.device_tracks(kps, off[:1], nodes), P)                  # n_tracks == 0
    e = yardstick(kps, P, off[:1], nodes[:0])
    for k in INT_KEYS:
        assert np.array_equal(got[k], e[k]), k
    assert got["offsets"].tolist() == [0] and got["report"].tolist() == [0] * 8 and got["summary"].tolist() == [0, 0, 21, 22, 23, 0, 24, 0]
    # max_tracks < n_tracks: PGX_E_CAPACITY from the status, the first max_tracks tracks processed
    d = synth.device_tracks(kps, off, nodes)
    got = run(engine, d, P, max_tracks=300, raises=pg.CapacityError)
    e = yardstick(kps, P, off[:301], nodes[:600])
    for k in INT_KEYS:
        assert np.array_equal(got[k], e[k]), k


# ---- errors ----------------------------------------------------------------------------------------------------------------

def test_bad_nodes_and_offsets_on_the_device(engine):
    cams = [cam((0, 0, 0)), cam((4, 0, 0)), cam((8, 0, 0))]
    good = [(0, (32, 0)), (1, (-32, 0)), (2, (-96, 0))]
    kps, P, off, nodes = problem(cams, [good, good, good])
    bad = nodes.copy()
    bad[4] = (1, 7)                              # keypoint outside [0, stride)
    bad[6] = (3, 0)                              # frame outside [0, n_frames)
    d = synth.device_tracks(kps, off, bad)
    got = run(engine, d, P, raises=pg.ArgumentException)
    e = yardstick(kps, P, off, bad, stride=d["stride"])
    for k in INT_KEYS:
        assert np.array_equal(got[k], e[k]), k
    assert got["nodes"].tolist() == [[0, 0], [1, 0], [2, 0], [0, 1], [2, 1], [1, 2], [2, 2]]
    # malformed offsets: the last track ends before it starts and counts as empty
    d = synth.device_tracks(kps, np.array([0, 3, 6, 5], np.int32), nodes)
    got = run(engine, d, P, raises=pg.ArgumentException)
    e = yardstick(kps, P, np.array([0, 3, 6, 6]), nodes[:6], stride=d["stride"])
    for k in INT_KEYS:
        assert np.array_equal(got[k], e[k]), k
    # two slots naming one frame
    d = synth.device_tracks(kps, off, nodes)
    d.update(identity=False, ids=torch.tensor([0, 1, 1], **I32))
    run(engine, d, P, raises=pg.ArgumentException)
    run(engine, synth.device_tracks(kps, off, nodes), P)      # the status word is clean again


def test_argument_checks(engine, planted):
    s, off, nodes = planted["s"], planted["off"][:11], planted["nodes"][:planted["off"][10]]
    d = synth.device_tracks(s["kps"], off, nodes)
    for kw in (dict(inlier_px=0.0), dict(inlier_px=-1.0), dict(inlier_px=float("inf")), dict(inlier_px=float("nan")),
               dict(min_parallax_deg=-0.5), dict(min_parallax_deg=90.0), dict(min_parallax_deg=float("nan")), dict(min_inliers=1),
               dict(max_hyp=0), dict(max_hyp=4097), dict(max_tracks=-1)):
        with pytest.raises(pg.ArgumentException):
            run(engine, d, s["P"], **kw)
    nf, stride = d["nf"], d["stride"]
    N = nf * stride
    dP = torch.from_numpy(s["P"]).to(DEV)
    o2, n2, s2 = torch.zeros(N + 1, **I32), torch.zeros((N, 2), **I32), torch.zeros(8, **I32)
    rest = (torch.zeros(N, **I32), torch.zeros((N, 3), **F64), torch.zeros(N, **I32), torch.zeros((N, 4), **I32), torch.zeros(8, **I32))
    torch.cuda.synchronize()
    for outs in ((d["off"], n2, s2), (o2, d["nodes"], s2), (o2, n2, d["tsum"])):          # aliased outputs
        with pytest.raises(pg.ArgumentException):
            engine.track_consensus_dev(d["kp"], nf, stride, nf, dP, d["off"], d["nodes"], d["tsum"], 10, *outs, *rest)
    with pytest.raises(pg.ArgumentException):
        engine.track_consensus_dev(d["kp"], nf, stride, nf + 1, dP, d["off"], d["nodes"], d["tsum"], 10, o2, n2, s2, *rest)
    # the host form: nodes and offsets are checked before any GPU work; optional outputs may be NULL; empty input
    bad = nodes.copy()
    bad[0, 1] = s["counts"][bad[0, 0]]
    with pytest.raises(pg.ArgumentException):
        engine.track_consensus(s["kps"], s["P"], off, bad)
    with pytest.raises(pg.ArgumentException):
        engine.track_consensus(s["kps"], s["P"], np.array([0, 3, 2]), nodes[:3])
    h = engine.track_consensus(s["kps"], s["P"], np.zeros(1, np.int32), np.zeros((0, 2), np.int32))
    assert h["offsets"].tolist() == [0] and h["report"].tolist() == [0] * 8 and len(h["nodes"]) == 0
    import ctypes as C
    full = engine.track_consensus(s["kps"], s["P"], off, nodes)
    flat = np.ascontiguousarray(np.concatenate(s["kps"]))
    o_out, n_out, s_out, rep = np.zeros(11, np.int32), np.zeros((len(nodes), 2), np.int32), np.zeros(8, np.int32), np.zeros(8, np.int32)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    rc = engine._L.pgx_track_consensus(engine._h, p(flat), p(s["counts"]), 12, p(np.ascontiguousarray(s["P"])), p(off), p(nodes), 10,
                                       4.0, 1.0, 2, 2, 256, 0, p(o_out), p(n_out), p(s_out), None, None, None, None, p(rep))
    assert rc == 0 and np.array_equal(o_out[:s_out[0] + 1], full["offsets"]) and np.array_equal(rep, full["report"])
    engine.check_status()
