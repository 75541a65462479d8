"""GPU tests of the float64 geometry stages (triangulation, bundle adjustment, registration) at the sizes where their index
arithmetic changes: the wave-per-track phase and several nodes per lane, second grid-stride passes, the largest reduced camera
system, sample chunks and the scoring tile's edges.  The tracks are cut to exact lengths on the host (synth.cut_tracks) and go
straight to the *_dev calls with a hand-made track summary, so that their lengths do not depend on the track graph.  Every
case is held to its stage's numpy yardstick with the comparison helpers and tolerances that tests/test_gpu_{triangulate,
bundle,register}.py use (tests/geom_gpu.py), and to itself bit for bit where only the grid, the slot layout or the chunking changes.  Each test asserts on the
host that its shape reaches the path it names, so that a later change to synth cannot quietly shrink it."""
import numpy as np
import pytest
import torch

import bundle_ref
import register_ref
import geom_gpu as g
import triangulate_ref as tref
from geom_gpu import DEV, F64, I32
from photogrammetry_amd import synth

pytestmark = pytest.mark.gpu

# the kernels' launch shapes (k_triangulate.hip, k_bundle.hip, k_register.hip)
TRI_GROUPS_G64 = 1024 * 256 // 64       # TRI_GRID_MAX workgroups x TRI_NT threads / 64 lanes: wave groups of one pass
BA_GROUPS = 1024 * 256 // 16            # BA_GRID_MAX x BA_NT / BA_G: track groups of one pass of a per-track kernel
BA_G, REG_G = 16, 16                    # lanes per track of the per-track kernels of k_bundle.hip and k_reg_count
REG_CHUNK_CELLS = 1 << 17


def reg_chunk(n_frames, n_samples):
    ch = max(64, (REG_CHUNK_CELLS // n_frames) & ~63)
    return min(ch, (n_samples + 63) & ~63)


def tri_run(engine, d, P, min_par=1.0, max_e=2.0, iters=10, max_tracks=None):
    """pgx_triangulate_tracks_dev on g.device_problem's buffers, one sync -> the dict g.tri_check_against_yardstick reads"""
    nf, n = d["nf"], d["n_tracks"]
    mt = n if max_tracks is None else max_tracks
    xyz, q = torch.full((max(mt, 1), 3), 5.0, **F64), torch.full((max(mt, 1), 3), 5.0, **F64)
    fl, summ = torch.full((max(mt, 1),), 7, **I32), torch.full((8,), 7, **I32)
    err = torch.full((max(d["F"], nf) * d["stride"],), 5.0, **F64)
    dP = torch.from_numpy(np.ascontiguousarray(P, dtype=np.float64).reshape(nf, 12)).to(DEV)
    torch.cuda.synchronize()
    engine.triangulate_tracks_dev(d["kp"], d["F"], d["stride"], nf, dP, d["off"], d["nodes"], d["tsum"], mt, xyz, q, fl, summ,
                                  min_par, max_e, iters, d_node_err=err, d_frame_ids=None if d["identity"] else d["ids"])
    engine.check_status()
    return dict(offsets=d["off"].cpu().numpy(), nodes=d["nodes"].cpu().numpy(), xyz=xyz.cpu().numpy()[:n],
                quality=q.cpu().numpy()[:n], flags=fl.cpu().numpy()[:n], summary=summ.cpu().numpy(), n_tracks=n,
                node_err=err.cpu().numpy()[:d["n_nodes"]])


def tri_grid(max_tracks):
    return min(max((max_tracks + 3) // 4, 1), 1024)       # k_triangulate.hip's grid


def assert_points_within_1e9(got, e, P, mask):
    """the refined points of the tracks in mask to 1e-9 of the distance to their mean camera centre (check_against_yardstick's
    bound without the stop band)"""
    known, C, _, _ = tref.cameras(P)
    off, nodes = got["offsets"], got["nodes"]
    ok = mask & np.isfinite(e["xyz"]).all(1) & (e["parallax"] >= 1.0)
    S = np.array([C[[f for f, _ in nodes[off[t]:off[t + 1]] if known[f]]].mean(0) for t in np.flatnonzero(ok)])
    dist = np.linalg.norm(e["xyz"][ok] - S, axis=1)
    dx = np.linalg.norm(got["xyz"][ok] - e["xyz"][ok], axis=1)
    assert ok.any() and (dx <= 1e-9 * dist).all(), (dx / dist).max()


def padded_slots(nf, pad, seed):
    return list(np.random.default_rng(seed).permutation(nf + pad)[:nf]), nf + pad


# ---------------------------------------------------------------------------------------------------------------- triangulation

TRI_EDGES = (2, 8, 9, 16, 32, 33, 64, 65, 100, 130)


def test_triangulate_every_length_class_in_one_call(engine):
    """130 frames, track lengths on every class edge (2, 8, 9, 16, 32, 33, 64, 65, 100, 130) mixed in one call, against the
    yardstick with 10 refinement steps and with none.  The short tracks' baselines are narrow here, so the refined points are
    held to max(1e-9 dist, triangulate_ref.stop_band).  The tracks of more than 64 nodes are held to 1e-9 dist as well.  Those
    of 33..64 nodes are not: on this 60-degree arc they reach 1.1e-9, as do the yardstick's own SVD and Gram-matrix starts
    (1.1e-9 on 33-node tracks); test_triangulate_long_tracks_second_grid_pass holds 33..64 nodes to 1e-9 on 64 frames.
    Rows reached: 'tri_phase<64, 2>: a whole wave per track' (tracks of more than 32 nodes) and 'more than one observation per
    lane in the G = 64 phase; O(n^2) parallax loop over long tracks' (tracks of more than 64 nodes)."""
    nf, n_points = 130, 2000
    s = synth.make_scene(n_points, nf, seed=31)
    lengths = np.array(TRI_EDGES)[np.arange(n_points) % len(TRI_EDGES)]
    off, nodes, _ = synth.cut_tracks(s, lengths, seed=1)
    L = np.diff(off)
    for e in TRI_EDGES:
        assert (L == e).sum() >= 150, (e, (L == e).sum())
    assert ((L > 32) & (L <= 64)).any()        # G = 64: one node per lane at most
    assert (L > 64).any() and L.max() == nf    # G = 64: two or three nodes per lane
    d = g.device_problem(s["kps"], off, nodes)
    for iters in (10, 0):
        got = tri_run(engine, d, s["P"], 1.0, 2.0, iters)
        e, excluded = g.tri_check_against_yardstick(got, s["kps"], s["P"], 1.0, 2.0, iters, stop_band=True)
        if iters > 0:
            assert_points_within_1e9(got, e, s["P"], L > 64)
        assert (got["flags"][L > 32] == 0).mean() > 0.9       # the long tracks are valid points, not flagged away
        print("iters", iters, "excluded from flag equality:", excluded.tolist())


def test_triangulate_long_tracks_second_grid_pass(engine):
    """More than 4096 tracks of 33..64 nodes: the G = 64 phase strides over the grid a second time.  Against the yardstick at
    1e-9, and bit for bit across max_tracks = n_tracks, n_tracks + 5000 and the node count (these all launch the capped grid
    of 1024 workgroups: with more than 4096 tracks max_tracks cannot change it).  The grid does change for the first 1000
    tracks alone: 250 workgroups (one pass, a wave per track) at max_tracks = 1000 and 1024 at 6000; their points keep the
    bits they have in the full call.
    Row reached: 'a second grid-stride pass of the G = 64 phase' (more than TRI_GRID_MAX x 4 waves = 4096 long tracks)."""
    nf, n_points = 64, 5000
    s = synth.make_scene(n_points, nf, seed=32)
    lengths = 33 + np.arange(n_points) % 32
    off, nodes, _ = synth.cut_tracks(s, lengths, seed=2)
    L = np.diff(off)
    assert ((L > 32) & (L <= 64)).sum() > TRI_GROUPS_G64, (L > 32).sum()
    d = g.device_problem(s["kps"], off, nodes)
    base = tri_run(engine, d, s["P"], 1.0, 2.0, 10, max_tracks=len(nodes))
    g.tri_check_against_yardstick(base, s["kps"], s["P"], 1.0, 2.0, 10)
    for mt in (d["n_tracks"], d["n_tracks"] + 5000):
        other = tri_run(engine, d, s["P"], 1.0, 2.0, 10, max_tracks=mt)
        g.same_bits(base, other, g.TRI_KEYS)
        assert g.bits(base["node_err"]) == g.bits(other["node_err"])
    n1 = 1000
    assert tri_grid(n1) == 250 and tri_grid(n1 + 5000) == 1024 == tri_grid(len(nodes))
    d1 = g.device_problem(s["kps"], off[:n1 + 1], nodes[:off[n1]])
    for mt in (n1, n1 + 5000):
        sub = tri_run(engine, d1, s["P"], 1.0, 2.0, 10, max_tracks=mt)
        for k in ("xyz", "quality", "flags"):
            assert g.bits(sub[k]) == g.bits(base[k][:n1]), (mt, k)
        assert g.bits(sub["node_err"]) == g.bits(base["node_err"][:off[n1]]), mt


def test_triangulate_bench_shape(engine):
    """tools/bench_triangulate.py's shape (a): 64 frames on a 120-degree arc, 8000 points cut to 2..64 nodes.  The yardstick on
    every track (refined points to max(1e-9 dist, triangulate_ref.stop_band): narrow baselines; the tracks of more than 32
    nodes to 1e-9 dist), and bit equality with the frames in permuted slots among 5 padding slots.
    Rows reached: all three phases (G = 4, 16, 64) in one call, 'tri_phase<64, 2>' among them."""
    rng = np.random.default_rng(0)
    nf = 64
    s = synth.make_scene(8000, nf, seed=1, arc_deg=120.0)
    off, nodes, _ = synth.cut_tracks(s, rng.integers(2, 65, size=8000), seed=3)
    L = np.diff(off)
    assert len(L) > 7500 and (L <= 8).any() and ((L > 8) & (L <= 32)).any() and (L > 32).any() and L.max() == 64
    d = g.device_problem(s["kps"], off, nodes)
    base = tri_run(engine, d, s["P"], 1.0, 2.0, 10)
    e, _ = g.tri_check_against_yardstick(base, s["kps"], s["P"], 1.0, 2.0, 10, stop_band=True)
    assert_points_within_1e9(base, e, s["P"], L > 32)
    slots, F = padded_slots(nf, 5, 4)
    perm = tri_run(engine, g.device_problem(s["kps"], off, nodes, slots=slots, n_slots=F), s["P"], 1.0, 2.0, 10)
    g.same_bits(base, perm, g.TRI_KEYS)
    assert g.bits(base["node_err"]) == g.bits(perm["node_err"])


# ------------------------------------------------------------------------------------------------------------ bundle adjustment

def ba_problem(n_points, nf, lengths, seed, perturb_seed=7):
    s = synth.make_scene(n_points, nf, seed=seed)
    off, nodes, pid = synth.cut_tracks(s, lengths, seed=seed)
    fixed = np.zeros(nf, np.int32)
    fixed[[0, nf - 1]] = 1
    Rt, X = synth.perturb(s["Rt"], s["points"][pid], seed=perturb_seed, fixed=fixed)
    return s, off, nodes, fixed, Rt, X


def ba_check(engine, s, off, nodes, fixed, Rt, X, d=None):
    d = d or g.device_problem(s["kps"], off, nodes)
    got = g.ba_run(engine, d, s["K"], Rt, fixed, X)
    e = bundle_ref.bundle_adjust(s["kps"], s["K"], Rt, fixed, off, nodes, X, max_iters=20)
    dg, de = g.ba_check_against_yardstick(got, e, 5.0)
    print("gpu", dg, got["report"].tolist(), "yardstick", de, e["report"].tolist())
    assert got["report"][1] >= 2         # steps were taken and accepted
    return d, got


def test_bundle_62_free_cameras_layouts_and_capacity(engine):
    """64 frames, 2 fixed and 62 free (the bench's count), tracks of 2..64 nodes; against the yardstick step for step, then
    bit for bit with the frames in permuted slots among 7 padding slots and with a larger max_tracks.
    Rows reached: 'lanes that handle more than one node (i += BA_G)' (tracks of more than 16 nodes) and 'reduced system of 62
    free cameras' (k_ba_schur with 62 owner threads, k_ba_solve on 372 x 372)."""
    nf = 64
    lengths = np.array([2, 16, 17, 32, 33, 48, 64])[np.arange(1500) % 7]
    s, off, nodes, fixed, Rt, X = ba_problem(1500, nf, lengths, seed=41)
    L = np.diff(off)
    assert (L > BA_G).any() and (L > 2 * BA_G).any() and L.max() == nf
    d, got = ba_check(engine, s, off, nodes, fixed, Rt, X)
    assert got["report"][3] == 62
    g.same_bits(got, g.ba_run(engine, d, s["K"], Rt, fixed, X, max_tracks=d["n_tracks"] + 3000), g.BA_KEYS)
    slots, F = padded_slots(nf, 7, 5)
    g.same_bits(got, g.ba_run(engine, g.device_problem(s["kps"], off, nodes, slots=slots, n_slots=F), s["K"], Rt, fixed, X),
                g.BA_KEYS)


def test_bundle_128_free_cameras(engine):
    """130 frames, 2 fixed and 128 free (BA_MAX_FREE: the largest reduced system that solves), tracks of up to 130 nodes;
    against the yardstick step for step.  No 2-node tracks: on this arc two neighbouring views are about 2 degrees apart, and
    such a point's depth turns the 2e-10 by which the cameras of the two solvers differ into up to 8e-8 (above 1e-8 x 5).
    Rows reached: 'reduced system of 128 free cameras' (k_ba_schur with 128 owner threads, k_ba_solve's blocked Cholesky on
    768 x 768), 'lanes that handle more than one node' (up to 9 nodes per lane at BA_G = 16) and the one-wave-per-track s_tab
    fill of k_ba_schur with a second wave pass (tracks of more than 64 nodes)."""
    nf = 130
    lengths = np.array([9, 16, 17, 64, 65, 100, 130])[np.arange(1400) % 7]
    s, off, nodes, fixed, Rt, X = ba_problem(1400, nf, lengths, seed=42)
    L = np.diff(off)
    assert (L > BA_G).any() and (L > 64).any() and L.max() == nf
    _, got = ba_check(engine, s, off, nodes, fixed, Rt, X)
    assert got["report"][3] == bundle_ref.MAX_FREE == 128


def test_bundle_second_grid_pass_over_tracks(engine):
    """More than 16384 tracks of 2..4 nodes over 6 frames (2 fixed): the per-track kernels stride over the grid a second time.
    Against the yardstick step for step.
    Row reached: 'grid-stride over tracks in the per-track kernels' (more than BA_GRID_MAX x BA_NT / BA_G = 16384 tracks)."""
    nf, n_points = 6, 20000
    lengths = 2 + np.arange(n_points) % 3
    s, off, nodes, fixed, Rt, X = ba_problem(n_points, nf, lengths, seed=43)
    L = np.diff(off)
    assert len(L) > BA_GROUPS + 2000 and L.min() == 2 and L.max() == 4
    ba_check(engine, s, off, nodes, fixed, Rt, X)


# ----------------------------------------------------------------------------------------------------------------- registration

def check_register(got, e, scale=5.0):
    """tests/test_gpu_register.py's rules: correspondence counts, winning samples and flags equal; final inlier sets equal
    outside the rounding band (margin > 1e-9); poses to 1e-9 of the scene scale, NaN where the yardstick's are"""
    assert (got["frame_stats"][:, 0] == e["frame_stats"][:, 0]).all()
    win, win_e = got["frame_stats"][:, 2], e["frame_stats"][:, 2]
    assert (win == win_e).all(), np.flatnonzero(win != win_e)
    assert (got["frame_stats"][:, 3] == e["frame_stats"][:, 3]).all()
    for f, x in e["extra"].items():
        nd = x["nodes"]
        resolved = x["margin"] > 1e-9
        assert (got["node_inlier"][nd][resolved] == e["node_inlier"][nd][resolved]).all(), f
    assert (got["node_inlier"][e["node_inlier"] == -1] == -1).all()
    assert (np.isnan(got["Rt"]) == np.isnan(e["Rt"])).all()
    assert np.nanmax(np.abs(got["Rt"] - e["Rt"])) <= 1e-9 * scale
    assert (got["report"][:6] == e["report"][:6]).all()


def reg_scene(n_points, nf, seed, outlier_frame=None):
    """make_scene's true tracks and true points, 20 % of one target's keypoints moved to random pixels; frames 0, 1 known"""
    s = synth.make_scene(n_points, nf, seed=seed)
    kps = [k.copy() for k in s["kps"]]
    if outlier_frame is not None:
        rng = np.random.default_rng(9)
        k = kps[outlier_frame]
        mv = rng.choice(len(k), size=len(k) // 5, replace=False)
        k["x"][mv] = rng.integers(0, 1920, len(mv))
        k["y"][mv] = rng.integers(0, 1080, len(mv))
    reg = np.ones(nf, np.int32)
    reg[:2] = 0
    return s, kps, reg


@pytest.mark.parametrize("n_samples", [100, 128, 3000])
def test_register_sample_chunks_change_no_result(engine, n_samples):
    """The same 4-frame problem (2 known, 2 targets) as 4 frames and as 2048 frames, the 2044 extra frames known, without
    keypoints or nodes: 2048 frames shrink the sample chunk to 64, so 100 samples run in two chunks (the last partial), 128 in
    exactly two and 3000 in 47.  Every output is bit-equal to the compact problem's (a single chunk) and matches the yardstick.
    inlier_px = 0.8 spreads the hypotheses' inlier counts, so that both targets' winning samples lie past the first chunk
    (asserted from the yardstick): a chunk that scored the wrong samples, or keyed them with the wrong hypothesis number,
    would change the winner.
    Row reached: 'more than one sample chunk' (k_reg_hyp / k_reg_score per s0, best-key slot (4 s0) / REG_NT + blockIdx.x, a
    last chunk reaching past n_samples)."""
    nf, big, ip = 4, 2048, 0.8
    s, kps, reg = reg_scene(600, nf, seed=51, outlier_frame=3)
    off, nodes, pid = synth.scene_tracks(s)
    xyz = s["points"][pid]
    assert reg_chunk(nf, n_samples) >= n_samples                        # compact: one chunk
    ch = reg_chunk(big, n_samples)
    n_chunks = -(-n_samples // ch)
    assert ch == 64 and n_chunks == {100: 2, 128: 2, 3000: 47}[n_samples]
    e = register_ref.register(kps, s["K"], s["Rt"], reg, off, nodes, xyz, None, n_samples, ip, g.MIN_IN, g.ITERS, g.SEED)
    assert (e["frame_stats"][2:, 2] >= ch).all(), e["frame_stats"][2:, 2]       # every winner lies past the first chunk
    a = g.reg_run(engine, g.device_problem(kps, off, nodes), s["K"], s["Rt"], reg, xyz, n_samples=n_samples, inlier_px=ip)
    check_register(a, e)
    assert a["report"][1] == 2
    K2 = np.concatenate([s["K"], np.tile(s["K"][:1], (big - nf, 1))])
    Rt2 = np.concatenate([s["Rt"], np.tile(s["Rt"][:1], (big - nf, 1))])
    reg2 = np.concatenate([reg, np.zeros(big - nf, np.int32)])
    kps2 = kps + [kps[0][:0]] * (big - nf)
    b = g.reg_run(engine, g.device_problem(kps2, off, nodes), K2, Rt2, reg2, xyz, n_samples=n_samples, inlier_px=ip)
    for k in ("Rt", "P", "frame_stats", "frame_err"):
        assert g.bits(a[k]) == g.bits(b[k][:nf]), k
    assert g.bits(a["node_inlier"]) == g.bits(b["node_inlier"]) and g.bits(a["report"]) == g.bits(b["report"])
    assert (b["frame_stats"][nf:] == -1).all() and g.bits(b["Rt"][nf:]) == g.bits(Rt2[nf:])
    print("winning samples", a["frame_stats"][2:, 2].tolist(), "chunk", ch)


def test_register_bench_like_scene(engine):
    """64 frames, 2 known and 62 targets, tracks cut to 2..64 nodes, one target with 20 % of its keypoints moved; against the
    yardstick (winning samples, inlier sets, poses).
    Row reached: 'k_reg_count lanes with more than one node' (tracks of more than REG_G = 16 nodes, up to 4 per lane)."""
    nf, n_points = 64, 3000
    s, kps, reg = reg_scene(n_points, nf, seed=52, outlier_frame=30)
    off, nodes, pid = synth.cut_tracks(s, np.random.default_rng(5).integers(2, 65, size=n_points), seed=6)
    xyz = s["points"][pid]
    L = np.diff(off)
    assert (L > REG_G).any() and (L > 3 * REG_G).any()
    got = g.reg_run(engine, g.device_problem(kps, off, nodes), s["K"], s["Rt"], reg, xyz)
    e = register_ref.register(kps, s["K"], s["Rt"], reg, off, nodes, xyz, None, g.NS, g.IP, g.MIN_IN, g.ITERS, g.SEED)
    check_register(got, e)
    assert got["report"][0] == 62 and got["report"][1] == 62, got["report"]


TILE_COUNTS = {2: 3, 3: 255, 4: 256, 5: 257, 6: 513}        # target frame -> correspondences
TILE_EDGES = {3: (254,), 4: (255,), 5: (255, 256), 6: (255, 256, 511, 512)}   # the last / first element of a 256-tile
TILE_SEEDS = {2: 0, 3: 1, 4: 2, 5: 1, 6: 6}      # found by search; the test asserts what they give


def tile_scene(seeds=TILE_SEEDS):
    """7 frames (0, 1 known) and five targets with exactly TILE_COUNTS correspondences, one 2-node track (frame 0, target) per
    correspondence, in the target's order.  A target's correspondences are two consistent groups: P, seen by the true camera,
    and Q, one fewer, whose keypoints are the projections through that camera turned by 4 degrees (an even count adds one
    random pixel).  Every element at a tile edge (TILE_EDGES) belongs to P.  So a correct count picks a P hypothesis, and a
    count that misses any one P element ties P with Q -- the seeds place a clean Q sample before the first clean P sample, so
    the tie goes to Q.  -> (scene, kps, offsets, nodes, xyz, reg)"""
    nf = 7
    s = synth.make_scene(700, nf, seed=53)
    where = np.full((nf, 700), -1, np.int64)
    for f, pid in enumerate(s["point_id"]):
        where[f, pid] = np.arange(len(pid))
    every = np.flatnonzero((where >= 0).all(0))
    kps, tracks, xyz = [s["kps"][0], s["kps"][1]], [], []
    for f, n in TILE_COUNTS.items():
        rng = np.random.default_rng(1000 * f + seeds[f])
        pts = rng.choice(every, size=n, replace=False)
        n_p = (n + 1) // 2 if n > 3 else n
        n_q = n_p - 1 if n > 3 else 0
        role = np.full(n, 2)                               # 0: P, 1: Q, 2: a random pixel
        edges = list(TILE_EDGES.get(f, ()))
        rest = rng.permutation([j for j in range(n) if j not in edges])
        role[edges + list(rest[:n_p - len(edges)])] = 0
        role[rest[n_p - len(edges):n_p - len(edges) + n_q]] = 1
        R, tv = s["Rt"][f, :9].reshape(3, 3), s["Rt"][f, 9:]
        w = np.radians(4.0) * np.array([0.3, 1.0, 0.2]) / np.linalg.norm([0.3, 1.0, 0.2])
        RB = bundle_ref.exp_so3(w) @ R
        C = -R.T @ tv
        k = np.zeros(n, dtype=s["kps"][0].dtype)
        for j, p in enumerate(pts):
            X = s["points"][p]
            q = (R @ X + tv) if role[j] != 1 else RB @ (X - C)
            uv = s["K"][f, :2] * q[:2] / q[2] + s["K"][f, 2:]
            if role[j] == 2:
                uv = rng.integers(0, [1920, 1080])
            k["x"][j], k["y"][j] = np.round(uv)
            tracks.append([(0, where[0, p]), (f, j)])
            xyz.append(X)
        kps.append(k)
    off = np.concatenate([[0], np.cumsum([len(tr) for tr in tracks])]).astype(np.int32)
    nodes = np.array([nd for tr in tracks for nd in tr], np.int32)
    reg = np.ones(nf, np.int32)
    reg[:2] = 0
    return s, kps, off, nodes, np.array(xyz), reg


def hypothesis_inliers(kps, K, reg, off, nodes, xyz, n_samples, ip, seed):
    """register_ref's RANSAC stage laid open: per target with >= 3 correspondences, (inlier matrix [4 n_samples][n] of every
    hypothesis h = 4 s + rank, valid [4 n_samples])"""
    corr, _ = register_ref.correspondences(kps, reg, K, off, nodes, xyz)
    out = {}
    for f, (nd, _, X, u, v) in corr.items():
        if len(nd) < 3:
            continue
        fx, fy, cx, cy = (float(x) for x in K[f])
        Xs, cu, cv = X - X.mean(axis=0), cx - u, cy - v
        M, valid = np.zeros((4 * n_samples, len(nd)), bool), np.zeros(4 * n_samples, bool)
        for smp in range(n_samples):
            for rank, (Rh, th) in enumerate(register_ref.hypotheses(Xs, cu, cv, fx, fy, seed, f, smp)):
                M[4 * smp + rank] = register_ref.inliers(Rh, th, Xs, cu, cv, fx, fy, ip)
                valid[4 * smp + rank] = True
        out[f] = (M, valid)
    return out


def winning_hypothesis(M, valid, keep):
    c = np.where(valid, M[:, keep].sum(1), -1)
    return int(np.argmax(c)) if c.max() >= 0 else -1       # the largest count, ties to the lowest h (k_reg_score's key)


def miscounts(n):
    """scoring counts that lose elements at tile edges -> {name: correspondences kept}"""
    j = np.arange(n)
    out = {"last element of each tile": ~((j % 256 == 255) | (j == n - 1))}
    if n % 256:
        out["partial last tile"] = j < (n // 256) * 256
    if n > 256:
        out["first element of each later tile"] = ~((j % 256 == 0) & (j > 0))
        out["first tile only"] = j < 256
    return out


def test_register_scoring_tile_edges(engine):
    """Targets with exactly 3, 255, 256, 257 and 513 correspondences: k_reg_score stages them through LDS in tiles of
    REG_NT = 256, so these are one short tile, one tile less one, one full tile, one tile and one, and two tiles and one.
    tile_scene makes the exact counts decide the winner; the host asserts, on the yardstick's hypotheses, that a count which
    misses a tile's last element, its first, or the partial last tile picks another winner for every target it touches.
    Against the yardstick; the 3-correspondence target ends FEWINLIERS in both.
    Row reached: 'k_reg_score LDS tile edges'."""
    s, kps, off, nodes, xyz, reg = tile_scene()
    corr, _ = register_ref.correspondences(kps, reg, s["K"], off, nodes, xyz)
    assert {f: len(corr[f][0]) for f in corr} == TILE_COUNTS
    H = hypothesis_inliers(kps, s["K"], reg, off, nodes, xyz, g.NS, g.IP, g.SEED)
    for f, (M, valid) in H.items():
        n = M.shape[1]
        w = winning_hypothesis(M, valid, np.ones(n, bool))
        if n == 3:
            continue
        assert M[w].sum() == (n + 1) // 2, (f, M[w].sum())                 # the winner is a P hypothesis
        for name, keep in miscounts(n).items():
            assert winning_hypothesis(M, valid, keep) != w, (n, name)
    got = g.reg_run(engine, g.device_problem(kps, off, nodes), s["K"], s["Rt"], reg, xyz)
    e = register_ref.register(kps, s["K"], s["Rt"], reg, off, nodes, xyz, None, g.NS, g.IP, g.MIN_IN, g.ITERS, g.SEED)
    check_register(got, e)
    win = [winning_hypothesis(*H[f], np.ones(TILE_COUNTS[f], bool)) // 4 for f in range(3, 7)]
    assert (e["frame_stats"][3:, 2] == win).all()
    assert got["frame_stats"][2, 3] == register_ref.FEWINLIERS and (got["frame_stats"][3:, 3] == 0).all()
