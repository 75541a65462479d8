"""GPU tests of epipolar-guided exact matching (pgx_knn_guided_batch_dev, pgx_match_guided_batch_dev, pgx_knn_guided).

Every result is exact, so every check is == against the numpy yardstick of tests/guided_ref.py (the header's predicate in
float64, a brute-force top-2 and column nearest over the admissible pairs), which tests/test_guided_codegen.py ties to a
literal Python loop.  Two checks tie the mode to paths that already exist: with a band that admits everything it equals the
unguided nearest-neighbour mode, and its NN lists go through the track graph like the oracle's.
"""
import numpy as np
import pytest
import torch

from geom_gpu import run_tracks
from guided_ref import admissible, ref_guided
from knn_ref import NONE, ref_select
from match_gpu import DEV, run_knn, run_nn, upload
from oracle import pose_np, tracks_np
import photogrammetry_amd as pg
from photogrammetry_amd import synth

pytestmark = pytest.mark.gpu
ENGINE = None


@pytest.fixture(scope="module", autouse=True)
def _engine():
    global ENGINE
    ENGINE = pg.Engine(0)
    yield
    ENGINE.close()
    ENGINE = None


# ---- scenes -----------------------------------------------------------------------------------------------------------------
K = pose_np.K.astype(np.float64)
F_AXIS = np.array([[0, 0, 0], [0, 0, -1], [0, 1, 0]], dtype=np.float32)   # the line of row (x, y) is v = y


def two_views(n, n_out, seed, words, flip=0.12, a=0.07, t=(0.6, 0.05, 0.1)):
    """The pose tests' scene (synth.two_view_pixels) with descriptors: n points drawn, those seen in both views kept, and n_out
    distractors per frame.  Column j < n_true of frame b is the view of row perm[j] of frame a.
    -> (da, kpa, db, kpb, F, truth) with truth[j] = true row of column j or -1."""
    rng = np.random.default_rng(seed)
    R, tt = synth.rot_y(a), np.asarray(t, dtype=np.float64)
    p1, p2 = synth.two_view_pixels(rng, n, K, R, tt)
    nt = len(p1)
    d1, d2, perm = synth.true_match_descriptors(nt, words, seed + 1000, flip=flip)
    pts = lambda m: np.stack([rng.integers(0, 3000, m), rng.integers(0, 4000, m)], 1).astype(np.int32)   # noqa: E731
    rnd = lambda m: rng.integers(0, 2**32, size=(m, words), dtype=np.uint32)                            # noqa: E731
    kpa, da = np.concatenate([p1, pts(n_out)]), np.concatenate([d1, rnd(n_out)])
    kpb, db = np.concatenate([p2[perm], pts(n_out)]), np.concatenate([d2, rnd(n_out)])
    truth = np.concatenate([perm, np.full(n_out, -1)]).astype(np.int64)
    return da, kpa, db, kpb, synth.fundamental_from_pose(K, R, tt), truth


def check_knn(frames, stride, words, pl, Fs, band, refs=None):
    """Every k and column-side combination of one batch against the yardstick; returns the refs."""
    dev = upload(stride, words, *zip(*frames))
    counts = dev[3]
    if refs is None:
        refs = [ref_guided(frames[a][0], frames[b][0], frames[a][1], frames[b][1], Fs[m], band) for m, (a, b) in enumerate(pl)]
    for k in (1, 2):
        for col in (False, True):
            idx, dist, cnn = run_knn(ENGINE, dev, stride, words, pl, k, col, guide=(Fs, band))
            for m, (a, b) in enumerate(pl):
                r_idx, r_dist, r_col = refs[m]
                n1, n2 = counts[a], counts[b]
                assert (idx[m, :n1] == r_idx[:, :k]).all(), (m, band, k, col, "idx")
                assert (dist[m, :n1] == r_dist[:, :k]).all(), (m, band, k, col, "dist")
                assert (idx[m, n1:] == 77).all() and (dist[m, n1:] == 77).all(), "rows >= counts[a] written"
                if col:
                    assert (cnn[m, :n2] == r_col).all(), (m, band, k, "col")
                    assert (cnn[m, n2:] == 77).all(), "columns >= counts[b] written"
    return refs


# ---- 1. the two-view scene ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("words", [8, 5])
def test_two_view_scene(words):
    s0 = two_views(700, 150, 1, words)
    s1 = two_views(400, 300, 2, words, a=-0.05, t=(-0.3, 0.4, 0.05))
    frames = [(s0[0], s0[1]), (s0[2], s0[3]), (s1[0], s1[1]), (s1[2], s1[3])]
    pl = [(0, 1), (1, 0), (2, 3), (0, 1), (3, 2)]
    Fs = [s0[4], s0[4].T, s1[4], s0[4], s1[4].T]
    stride = max(len(f[0]) for f in frames) + 13
    for band in (0.0, 0.5, 2.0, 8.0):
        refs = check_knn(frames, stride, words, pl, Fs, band)
        if band == 8:   # the scene is what it claims: true matches lie inside the band
            adm = admissible(s0[1], s0[3], s0[4], band)
            truth = s0[5]
            j = np.nonzero(truth >= 0)[0]
            assert adm[truth[j], j].mean() > 0.99
            assert (refs[0][0][:, 0] >= 0).mean() > 0.5


# ---- 2. a band that admits everything is the unguided mode -------------------------------------------------------------------
@pytest.mark.parametrize("words", [8, 5])
def test_huge_band_equals_knn(words):
    rng = np.random.default_rng(40 + words)
    n = [4096, 4096, 1500]
    frames = [(rng.integers(0, 2**32, size=(c, words), dtype=np.uint32),
               np.stack([rng.integers(0, 1920, c), rng.integers(0, 1080, c)], 1).astype(np.int32)) for c in n]
    Fr = rng.normal(size=9).astype(np.float32)
    pl = [(0, 1), (1, 2), (2, 0)]
    Fs = [F_AXIS, Fr, Fr]
    for m, (a, b) in enumerate(pl):   # well conditioned: every row has a line
        assert admissible(frames[a][1], frames[b][1], Fs[m], 1e30).all()
    stride = 4096
    dev = upload(stride, words, *zip(*frames))
    u = run_knn(ENGINE, dev, stride, words, pl, 2, True, sentinel=5)
    g = run_knn(ENGINE, dev, stride, words, pl, 2, True, sentinel=5, guide=(Fs, 1e30))
    assert (g[0] == u[0]).all() and (g[1] == u[1]).all() and (g[2] == u[2]).all()
    for ratio, cross in ((0.8, True), (0.0, False)):
        nn = run_nn(ENGINE, dev, stride, words, pl, 32 * words // 3, ratio, cross, sentinel=5)
        gm = run_nn(ENGINE, dev, stride, words, pl, 32 * words // 3, ratio, cross, sentinel=5, guide=(Fs, 1e30))
        assert (gm == nn).all(), (ratio, cross)


# ---- 3. boundary cases --------------------------------------------------------------------------------------------------------
def test_band_edge_is_inclusive():
    """Lines v = y_i: columns at exactly `band` rows away are taken at band, and not at nextafter(band, 0)."""
    rng = np.random.default_rng(3)
    words = 8
    ya = np.arange(20, 620, 30)
    kpa = np.stack([rng.integers(0, 1000, len(ya)), ya], 1).astype(np.int32)
    offs = np.array([-4, -3, -2, 0, 2, 3, 4])
    kpb = np.array([(int(rng.integers(0, 1000)), y + o) for y in ya for o in offs], dtype=np.int32)
    da = rng.integers(0, 2**32, size=(len(kpa), words), dtype=np.uint32)
    db = rng.integers(0, 2**32, size=(len(kpb), words), dtype=np.uint32)
    frames = [(da, kpa), (db, kpb)]
    for band in (3.0, float(np.nextafter(np.float32(3), np.float32(0)))):
        refs = check_knn(frames, 160, words, [(0, 1)], [F_AXIS], band)
        adm = admissible(kpa, kpb, F_AXIS, band)
        edge = np.abs(kpb[None, :, 1] - kpa[:, None, 1]) == 3
        if band == 3.0:
            assert adm[edge].all()
        else:
            assert not adm[edge].any()
        assert adm.sum(1).min() == (5 if band == 3.0 else 3)
        assert (refs[0][0][:, 1] >= 0).all()


def test_degenerate_and_non_finite_F():
    rng = np.random.default_rng(4)
    words = 8
    x0, y0 = 500, 300
    kpa = np.concatenate([[[x0, y0]], np.stack([rng.integers(0, 1000, 99), rng.integers(0, 600, 99)], 1)]).astype(np.int32)
    kpb = np.stack([rng.integers(0, 1000, 300), rng.integers(0, 600, 300)], 1).astype(np.int32)
    da = rng.integers(0, 2**32, size=(100, words), dtype=np.uint32)
    db = rng.integers(0, 2**32, size=(300, words), dtype=np.uint32)
    F_pt = np.array([[1, 0, 0], [0, 1, 0], [-x0, -y0, 1]], dtype=np.float32)   # columns (1, 0, -x0), (0, 1, -y0), (0, 0, 1)
    bad = [np.zeros((3, 3), np.float32), F_AXIS.copy(), F_AXIS.copy(), F_AXIS.copy()]
    bad[1][2, 2] = np.nan
    bad[2][0, 0] = np.inf
    bad[3][1, 2] = -np.inf
    pl = [(0, 1)] * 5
    Fs = [F_pt] + bad
    refs = check_knn([(da, kpa), (db, kpb)], 304, words, pl, Fs, 40.0)
    assert (refs[0][0][0] == -1).all() and (refs[0][0][1:, 0] >= 0).any()   # n2 = 0 at (x0, y0) only
    for r in refs[1:]:
        assert (r[0] == -1).all() and (r[1] == NONE).all() and (r[2] == -1).all()


# ---- 4. shapes, chunks, repeatability, errors -----------------------------------------------------------------------------
def random_frames(rng, sizes, words, W=2000, H=1500):
    return [(rng.integers(0, 2**32, size=(n, words), dtype=np.uint32),
             np.stack([rng.integers(0, W, n), rng.integers(0, H, n)], 1).astype(np.int32).reshape(n, 2)) for n in sizes]


@pytest.mark.parametrize("words", [8, 3])
def test_shapes_padded_repeated_swapped_untouched(words):
    rng = np.random.default_rng(11 + words)
    frames = random_frames(rng, [300, 0, 1000, 77, 2, 5000], words)
    frames[3][1][:] = frames[3][1][0]     # every keypoint of a frame at one place: a one-cell grid
    stride = 5056
    pl = [(0, 2), (2, 0), (0, 2), (3, 5), (5, 3), (2, 1), (1, 2), (4, 0), (0, 4), (5, 5), (2, 5), (5, 2)]
    Fs = [rng.normal(size=9).astype(np.float32) for _ in pl]
    Fs[2] = Fs[0]
    refs = check_knn(frames, stride, words, pl, Fs, 12.0)
    assert sum(int((r[0][:, 0] >= 0).sum()) for r in refs) > 500
    # max_count below the stride, the host form, the NN lists
    dev = upload(stride, words, *zip(*frames))
    idx, dist, _ = run_knn(ENGINE, dev, stride, words, pl, 2, False, max_count=5000, guide=(Fs, 12.0))
    for m, (a, b) in enumerate(pl):
        assert (idx[m, :len(frames[a][0])] == refs[m][0]).all()
    for m in (0, 3, 4, 10):
        a, b = pl[m]
        h = ENGINE.knn_guided(frames[a][0], kp_array(frames[a][1]), frames[b][0], kp_array(frames[b][1]), Fs[m], 12.0, k=2, col=True)
        assert (h[0] == refs[m][0]).all() and (h[1] == refs[m][1]).all() and (h[2] == refs[m][2]).all()
        h1 = ENGINE.knn_guided(frames[a][0], kp_array(frames[a][1]), frames[b][0], kp_array(frames[b][1]), Fs[m], 12.0, k=1)
        assert (h1[0] == refs[m][0][:, :1]).all() and (h1[1] == refs[m][1][:, :1]).all()
    for max_dist, ratio, cross in ((32 * words, 0.0, False), (32 * words // 3, 0.8, True), (0, 1.0, False)):
        out = run_nn(ENGINE, dev, stride, words, pl, max_dist, ratio, cross, guide=(Fs, 12.0))
        for m, (a, b) in enumerate(pl):
            n1 = len(frames[a][0])
            assert (out[m, :n1] == ref_select(*refs[m], max_dist, ratio, cross)).all(), (m, max_dist, ratio, cross)
            assert (out[m, n1:] == 77).all()


def kp_array(p):
    kp = np.zeros(len(p), dtype=pg.KEYPOINT_DTYPE)
    kp["x"], kp["y"] = p[:, 0], p[:, 1]
    return kp


def test_chunk_size_and_repeatability():
    rng = np.random.default_rng(12)
    words, Fn = 8, 12
    frames = random_frames(rng, [int(rng.integers(200, 900)) for _ in range(Fn)], words)
    pl = [(i, j) for i in range(Fn) for j in range(Fn) if i != j][:40]
    Fs = [rng.normal(size=9).astype(np.float32) for _ in pl]
    stride = 900
    dev = upload(stride, words, *zip(*frames))
    base = run_knn(ENGINE, dev, stride, words, pl, 2, True, guide=(Fs, 6.0))
    again = run_knn(ENGINE, dev, stride, words, pl, 2, True, guide=(Fs, 6.0))
    m0 = run_nn(ENGINE, dev, stride, words, pl, 80, 0.8, True, guide=(Fs, 6.0))
    try:
        ENGINE.set_match_chunk(16)
        small = run_knn(ENGINE, dev, stride, words, pl, 2, True, guide=(Fs, 6.0))
        m1 = run_nn(ENGINE, dev, stride, words, pl, 80, 0.8, True, guide=(Fs, 6.0))
    finally:
        ENGINE.set_match_chunk(2048)
    for x, y, z in zip(base, again, small):
        assert x.tobytes() == y.tobytes() == z.tobytes()
    assert m0.tobytes() == m1.tobytes()
    for m in (0, 17, 39):
        a, b = pl[m]
        r = ref_guided(frames[a][0], frames[b][0], frames[a][1], frames[b][1], Fs[m], 6.0)
        assert (base[0][m, :len(frames[a][0])] == r[0]).all() and (base[2][m, :len(frames[b][0])] == r[2]).all()


def test_bad_arguments():
    t = torch.zeros(4096, dtype=torch.int32, device=DEV)
    f = torch.zeros(64, dtype=torch.float32, device=DEV)
    for band in (float("nan"), float("inf"), -1.0, -1e-30):
        with pytest.raises(pg.ArgumentException):
            ENGINE.knn_guided_batch_dev(t, t, t, 16, 8, t, 1, f, band, 2, t, t)
        with pytest.raises(pg.ArgumentException):
            ENGINE.match_guided_batch_dev(t, t, t, 16, 8, t, 1, f, band, t, 100, 0.8)
    with pytest.raises(pg.ArgumentException):
        ENGINE.knn_guided_batch_dev(t, t, t, 16, 8, t, 1, f, 2.0, 3, t, t)            # k = 3
    with pytest.raises(pg.ArgumentException):
        ENGINE.knn_guided_batch_dev(t, t, t, 16, 0, t, 1, f, 2.0, 2, t, t)            # words = 0
    with pytest.raises(pg.ArgumentException):
        ENGINE.knn_guided_batch_dev(t, t, t, 16, 128, t, 1, f, 2.0, 2, t, t)          # words = 128
    with pytest.raises(pg.ArgumentException):
        ENGINE.knn_guided_batch_dev(t, t, t, 0, 8, t, 1, f, 2.0, 2, t, t)             # stride = 0
    with pytest.raises(pg.ArgumentException):
        ENGINE.match_guided_batch_dev(t, t, t, 16, 8, t, 1, f, 2.0, t, 100, 1.5)      # ratio > 1
    a = np.zeros((4, 8), np.uint32)
    kp = np.zeros(4, dtype=pg.KEYPOINT_DTYPE)
    with pytest.raises(pg.ArgumentException):
        ENGINE.knn_guided(a, kp, a, kp, np.eye(3), float("nan"))
    with pytest.raises(pg.ArgumentException):
        ENGINE.knn_guided(a, kp, a, kp, np.eye(3), 1.0, k=3)
    ENGINE.check_status()


def test_out_of_range_coordinate_rejects_its_pairs_and_reports():
    rng = np.random.default_rng(13)
    words = 8
    frames = random_frames(rng, [200, 300, 250], words)
    frames[0][1][0] = (-(1 << 20), (1 << 20) - 1)   # the extremes of the range are fine
    bad = (frames[2][0], frames[2][1].copy())
    bad[1][17, 0] = 1 << 20
    frames.append(bad)
    stride = 320
    pl = [(0, 1), (3, 1), (1, 3), (1, 0)]
    Fs = [rng.normal(size=9).astype(np.float32) for _ in pl]
    dev = upload(stride, words, *zip(*frames))
    d_pl = torch.tensor(pl, dtype=torch.int32, device=DEV)
    d_F = torch.from_numpy(np.stack(Fs)).to(DEV)
    idx = torch.full((4, stride, 2), 77, dtype=torch.int32, device=DEV)
    dist = torch.full((4, stride, 2), 77, dtype=torch.int32, device=DEV)
    ENGINE.knn_guided_batch_dev(dev[0], dev[1], dev[2], stride, words, d_pl, 4, d_F, 50.0, 2, idx, dist)
    with pytest.raises(pg.ArgumentException):
        ENGINE.check_status()
    ENGINE.check_status()   # the status word was read and cleared
    idx, dist = idx.cpu().numpy(), dist.cpu().numpy()
    for m in (1, 2):
        n1 = len(frames[pl[m][0]][0])
        assert (idx[m, :n1] == -1).all() and (dist[m, :n1] == NONE).all() and (idx[m, n1:] == 77).all()
    found = 0
    for m in (0, 3):
        a, b = pl[m]
        r = ref_guided(frames[a][0], frames[b][0], frames[a][1], frames[b][1], Fs[m], 50.0)
        assert (idx[m, :len(frames[a][0])] == r[0]).all() and (dist[m, :len(frames[a][0])] == r[1]).all()
        found += int((r[0][:, 0] >= 0).sum())
    assert found > 0
    a = frames[3]
    with pytest.raises(pg.ArgumentException):
        ENGINE.knn_guided(a[0], kp_array(a[1]), frames[1][0], kp_array(frames[1][1]), Fs[0], 5.0)
    ENGINE.check_status()


# ---- 5. the chain: RANSAC's F in, track graph out -------------------------------------------------------------------------
def sequence(n_frames, n_pts, seed, words, flip=0.1):
    """One point cloud seen by a camera moving sideways: frames (desc, kp), true F per ordered pair, point id per keypoint."""
    rng = np.random.default_rng(seed)
    X = np.stack([rng.uniform(-3, 3, n_pts), rng.uniform(-4, 4, n_pts), rng.uniform(5, 10, n_pts)], 1)
    base = rng.integers(0, 2**32, size=(n_pts, words), dtype=np.uint32)
    poses = [(synth.rot_y(0.02 * f), np.array([0.25 * f, 0.02 * f, 0.0])) for f in range(n_frames)]
    frames, ids = [], []
    for R, t in poses:
        x = (K @ (R @ X.T + t[:, None])).T
        p = np.rint(x[:, :2] / x[:, 2:3]).astype(np.int32)
        keep = np.nonzero((p[:, 0] >= 0) & (p[:, 0] < 3000) & (p[:, 1] >= 0) & (p[:, 1] < 4000))[0]
        keep = rng.permutation(keep)[: int(len(keep) * 0.9)]
        bits = np.unpackbits(base[keep].view(np.uint8), axis=1)
        bits ^= (rng.random(bits.shape) < flip).astype(np.uint8)
        frames.append((np.ascontiguousarray(np.packbits(bits, axis=1).view(np.uint32)), p[keep]))
        ids.append(keep)

    def F_of(a, b):   # x_a ~ K (Ra X + ta), x_b ~ K (Rb X + tb): relative motion a -> b
        (Ra, ta), (Rb, tb) = poses[a], poses[b]
        R = Rb @ Ra.T
        return synth.fundamental_from_pose(K, R, tb - R @ ta)
    return frames, ids, F_of


def test_nn_lists_feed_the_track_graph():
    words, Fn = 8, 6
    frames, _, F_of = sequence(Fn, 700, 21, words)
    stride = max(len(f[0]) for f in frames)
    dev = upload(stride, words, *zip(*frames))
    counts = dev[3]
    pl = [(i, j) for i in range(Fn) for j in range(i + 1, Fn)]
    Fs = [F_of(a, b) for a, b in pl]
    m = run_nn(ENGINE, dev, stride, words, pl, 70, 0.8, True, guide=(Fs, 2.0))
    for q in (0, len(pl) - 1):
        a, b = pl[q]
        r = ref_guided(frames[a][0], frames[b][0], frames[a][1], frames[b][1], Fs[q], 2.0)
        assert (m[q, :counts[a]] == ref_select(*r, 70, 0.8, True)).all()
    off, nod, tof, s = run_tracks(ENGINE, counts, pl, m, stride, 70, 2)
    e_off, e_nodes, e_tof, e_s = tracks_np.tracks_arrays(counts, pl, m, stride, 70, 2)
    assert (off == e_off).all() and (nod == e_nodes).all() and (tof == e_tof).all()
    assert s[0] == e_s["n_tracks"] > 100 and s[1] == e_s["n_nodes"]


def test_ransac_F_is_accepted_as_is():
    """d_F of pgx_fundamental_ransac_dev goes in unchanged: the results equal the yardstick on the matrices read back.
    RANSAC scores h_a^T F h_b like this header, but its estimate keeps the reference's column-major fill, so the matrix it fits
    to true correspondences satisfies h_b^T F h_a = 0 (include/pgx.h): transposed, it fits them."""
    words = 8
    da, kpa, db, kpb, _, truth = two_views(600, 0, 31, words)
    n = len(da)
    j = np.nonzero(truth >= 0)[0]
    stride = n
    frames = [(da, kpa), (db, kpb)]
    dev = upload(stride, words, *zip(*frames))
    ml = np.zeros((1, stride, 3), dtype=np.int32)
    ml[0, :len(j), 0], ml[0, :len(j), 1] = truth[j], j          # the true list: (row, column, 0)
    d_pl = torch.tensor([[0, 1]], dtype=torch.int32, device=DEV)
    d_F = torch.zeros((1, 9), dtype=torch.float32, device=DEV)
    d_in = torch.zeros(1, dtype=torch.int32, device=DEV)
    d_bs = torch.zeros(1, dtype=torch.int32, device=DEV)
    d_counts1 = torch.tensor([len(j), len(j)], dtype=torch.int32, device=DEV)
    torch.cuda.synchronize()
    ENGINE.fundamental_ransac_dev(dev[1], torch.from_numpy(ml).to(DEV), d_counts1, d_pl, 1, stride, 64, 8, 0.001, d_F, d_in, d_bs,
                                  seed=5)
    ENGINE.check_status()
    F = d_F.cpu().numpy()[0]
    idx = torch.full((1, stride, 2), 77, dtype=torch.int32, device=DEV)
    dist = torch.full((1, stride, 2), 77, dtype=torch.int32, device=DEV)
    ENGINE.knn_guided_batch_dev(dev[0], dev[1], dev[2], stride, words, d_pl, 1, d_F, 8.0, 2, idx, dist)
    ENGINE.check_status()
    r = ref_guided(da, db, kpa, kpb, F, 8.0)
    assert (idx.cpu().numpy()[0] == r[0]).all() and (dist.cpu().numpy()[0] == r[1]).all()
    fit = admissible(kpa, kpb, F, 8.0)[truth[j], j].mean()
    fit_t = admissible(kpa, kpb, F.reshape(3, 3).T, 8.0)[truth[j], j].mean()
    assert fit_t > 0.5 and fit_t > fit, (fit, fit_t)
    idx_t = torch.full((1, stride, 2), 77, dtype=torch.int32, device=DEV)
    ENGINE.knn_guided_batch_dev(dev[0], dev[1], dev[2], stride, words, d_pl, 1, d_F.view(1, 3, 3).transpose(1, 2).contiguous(),
                                8.0, 2, idx_t, dist)
    ENGINE.check_status()
    assert (idx_t.cpu().numpy()[0, truth[j], 0] == j).mean() > 0.8


# ---- 6. what it is for: repeated texture ---------------------------------------------------------------------------------------
def test_guided_lists_hold_more_correct_and_fewer_wrong_matches():
    """Descriptors drawn from a small pool (repeated texture): the unguided ratio test rejects most rows or picks a twin
    elsewhere in the image; the band keeps only the twins near the line."""
    words = 8
    rng = np.random.default_rng(55)
    da, kpa, db, kpb, F, truth = two_views(1500, 0, 56, words)
    pool = rng.integers(0, 2**32, size=(40, words), dtype=np.uint32)
    nt = len(da)
    src = pool[rng.integers(0, 40, nt)]
    flip = lambda d, p: np.packbits(np.unpackbits(d.view(np.uint8), axis=1) ^ (rng.random((len(d), 32 * words)) < p)   # noqa: E731
                                    .astype(np.uint8), axis=1).view(np.uint32)
    da = np.ascontiguousarray(flip(src, 0.01))
    inv = np.argsort(truth)                      # column of each row
    db = np.ascontiguousarray(flip(da[truth], 0.02))
    assert (truth[inv] == np.arange(nt)).all()
    frames = [(da, kpa), (db, kpb)]
    stride = nt
    dev = upload(stride, words, *zip(*frames))
    nn = run_nn(ENGINE, dev, stride, words, [(0, 1)], 60, 0.8, False)[0]
    gd = run_nn(ENGINE, dev, stride, words, [(0, 1)], 60, 0.8, False, guide=([F], 2.0))[0]
    r = ref_guided(da, db, kpa, kpb, F, 2.0)
    assert (gd == ref_select(*r, 60, 0.8, False)).all()

    def score(lst):
        acc = lst[lst[:, 1] >= 0]
        ok = truth[acc[:, 1]] == acc[:, 0]
        return int(ok.sum()), int((~ok).sum())
    c_nn, w_nn = score(nn)
    c_gd, w_gd = score(gd)
    assert c_gd > c_nn and w_gd < w_nn, (c_nn, w_nn, c_gd, w_gd)
    assert c_gd > 2 * c_nn, (c_nn, c_gd)
