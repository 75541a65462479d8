"""GPU tests of the exact nearest-neighbour mode (pgx_knn_batch_dev, pgx_match_nn_batch_dev, pgx_knn; include/pgx.h).

Everything is an exact integer result, so every check is entry by entry.  The yardstick is the numpy brute force of
tests/knn_ref.py (a popcount table over uint8 views, then lexsort((j, d)) per row; the column side a first-occurrence argmin),
itself checked here against its literal Python loop over bin(x ^ y).count("1").  Two checks tie the mode to paths that
already exist: a mutual nearest pair under the (d, index) order is always taken by the greedy assignment
(pgx_match_batch_dev), and NN lists go through the track graph (pgx_tracks_dev) like the oracle's and the host form's.
"""
import numpy as np
import pytest
import torch

from geom_gpu import as_lists, run_tracks
from knn_ref import NONE, loop_knn, rand_desc, ref_knn, ref_select
from match_gpu import DEV, run_knn, run_nn, upload
from oracle import tracks_np
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


def check_host(a, b, k, col):
    r_idx, r_dist, r_col = ref_knn(a, b)
    out = ENGINE.knn(a, b, k=k, col=col)
    assert out[0].shape == (len(a), k) and out[1].shape == (len(a), k)
    assert (out[0] == r_idx[:, :k]).all(), "idx"
    assert (out[1] == r_dist[:, :k]).all(), "dist"
    if col:
        assert (out[2] == r_col).all(), "col"


# ---- host form, shapes ----------------------------------------------------------------------------------------------------
def test_ref_and_library_match_the_literal_loop():
    rng = np.random.default_rng(0)
    for words, n1, n2 in [(8, 7, 5), (3, 6, 9), (1, 5, 1), (10, 4, 2), (8, 3, 0)]:
        a, b = rand_desc(rng, n1, words), rand_desc(rng, n2, words)
        if n1 and n2:
            b[-1] = a[0]   # a zero distance
        rows, cols = loop_knn(a, b)
        r_idx, r_dist, r_col = ref_knn(a, b)
        idx, dist, cnn = ENGINE.knn(a, b, k=2, col=True)
        for i, row in enumerate(rows):
            exp = row + [(NONE, -1)] * (2 - len(row))
            assert [(int(r_dist[i, e]), int(r_idx[i, e])) for e in range(2)] == exp
            assert [(int(dist[i, e]), int(idx[i, e])) for e in range(2)] == exp
        assert list(r_col) == cols and list(cnn) == cols


@pytest.mark.parametrize("words", [8, 1, 2, 3, 10])
def test_ragged_sizes(words):
    rng = np.random.default_rng(words)
    for n1, n2 in [(100, 37), (300, 65), (257, 200), (64, 2), (50, 1), (33, 0), (1, 300)]:
        a, b = rand_desc(rng, n1, words), rand_desc(rng, n2, words)
        for k in (1, 2):
            for col in (False, True):
                check_host(a, b, k, col)


@pytest.mark.parametrize("words,n1,n2", [(8, 300, 5000), (8, 130, 20000), (2, 200, 5000), (8, 3000, 3), (8, 3, 3000),
                                         (3, 2500, 4), (3, 4, 2500)])
def test_beyond_one_chunk_and_lopsided(words, n1, n2):
    rng = np.random.default_rng(n1 * 7 + n2)
    a, b = rand_desc(rng, n1, words), rand_desc(rng, n2, words)
    check_host(a, b, 2, True)
    check_host(a, b, 1, True)


@pytest.mark.parametrize("words", [8, 2])
def test_tie_heavy_pool(words):
    """Descriptors drawn from a pool of 20 with duplicates: nearly every distance ties, the index rule decides."""
    rng = np.random.default_rng(5)
    pool = rand_desc(rng, 20, words)
    for n1, n2 in [(500, 700), (700, 33), (40, 4500)]:
        a, b = pool[rng.integers(0, 20, n1)], pool[rng.integers(0, 20, n2)]
        check_host(a, b, 2, True)
        check_host(a, b, 1, False)


# ---- device batch ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("words", [8, 3])
def test_batch_padded_repeated_swapped_and_untouched(words):
    rng = np.random.default_rng(11)
    sizes = [300, 0, 1000, 77, 2, 513]
    descs = [rand_desc(rng, n, words) for n in sizes]
    stride = 1100
    dev = upload(stride, words, descs)
    counts = dev[3]
    pl = [(0, 2), (2, 0), (0, 2), (3, 5), (5, 3), (2, 1), (1, 2), (4, 0), (0, 4), (5, 5)]
    refs = {p: ref_knn(descs[p[0]], descs[p[1]]) for p in set(pl)}
    for k in (1, 2):
        for col in (False, True):
            idx, dist, cnn = run_knn(ENGINE, dev, stride, words, pl, k, col)
            for m, (a, b) in enumerate(pl):
                r_idx, r_dist, r_col = refs[(a, b)]
                n1, n2 = counts[a], counts[b]
                assert (idx[m, :n1] == r_idx[:, :k]).all() and (dist[m, :n1] == r_dist[:, :k]).all(), (m, k, col)
                assert (idx[m, n1:] == 77).all() and (dist[m, n1:] == 77).all(), "rows >= counts[a] written"
                if col:
                    assert (cnn[m, :n2] == r_col).all() and (cnn[m, n2:] == 77).all(), (m, k)
                if k == 2 and col:   # the host form gives the same
                    h = ENGINE.knn(descs[a], descs[b], k=2, col=True)
                    assert (h[0] == idx[m, :n1]).all() and (h[1] == dist[m, :n1]).all() and (h[2] == cnn[m, :n2]).all()
    # max_count below the stride still covers every count
    idx, dist, _ = run_knn(ENGINE, dev, stride, words, pl, 2, False, max_count=int(counts.max()))
    for m, (a, b) in enumerate(pl):
        assert (idx[m, :counts[a]] == refs[(a, b)][0]).all()


@pytest.mark.parametrize("words", [8, 2])
def test_match_nn_grid(words):
    rng = np.random.default_rng(21)
    a, b, _ = synth.true_match_descriptors(700, words, 3, flip=0.2)
    descs = [a, b[:650], rand_desc(rng, 400, words), np.zeros((0, words), np.uint32)]
    descs.append(descs[0][rng.integers(0, 700, 300)])   # duplicates: equal nearest distances, ratio 1.0 rejects them
    stride = 704
    dev = upload(stride, words, descs)
    counts = dev[3]
    pl = [(0, 1), (1, 0), (0, 2), (2, 3), (4, 0), (0, 4)]
    refs = {p: ref_knn(descs[p[0]], descs[p[1]]) for p in set(pl)}
    dmax = 32 * words
    for max_dist in (0, dmax // 5, dmax // 3, dmax):
        for ratio in (0.0, 0.6, 0.8, 1.0):
            for cross in (False, True):
                out = run_nn(ENGINE, dev, stride, words, pl, max_dist, ratio, cross)
                for m, (fa, fb) in enumerate(pl):
                    exp = ref_select(*refs[(fa, fb)], max_dist, ratio, cross)
                    n1 = counts[fa]
                    assert (out[m, :n1] == exp).all(), (m, max_dist, ratio, cross)
                    assert (out[m, n1:] == 77).all()


@pytest.mark.parametrize("words", [8, 3])
def test_match_nn_across_a_chunk_boundary(words):
    """17 image pairs at 16 pairs per chunk (the smallest): the second chunk of pgx_match_nn_batch_dev holds one pair.  Byte
    equal to the default chunk's output, equal to the yardstick, and rows at or beyond counts[a] keep the sentinel."""
    rng = np.random.default_rng(17 + words)
    base = rand_desc(rng, 150, words)
    descs = []
    for n in (150, 97, 0, 133, 1, 64):   # every frame sees a noisy subset of one scene: distances well inside the gate
        bits = np.unpackbits(base[rng.permutation(150)[:n]].view(np.uint8), axis=1)
        bits ^= (rng.random(bits.shape) < 0.08).astype(np.uint8)
        descs.append(np.ascontiguousarray(np.packbits(bits, axis=1).view(np.uint32)).reshape(n, words))
    stride = 160
    dev = upload(stride, words, descs)
    counts = dev[3]
    pl = [(i, j) for i in range(6) for j in range(i + 1, 6)] + [(5, 0), (3, 3)]
    assert len(pl) == 17
    max_dist = 32 * words // 3
    whole = run_nn(ENGINE, dev, stride, words, pl, max_dist, 0.8, True)
    try:
        ENGINE.set_match_chunk(16)
        chunked = run_nn(ENGINE, dev, stride, words, pl, max_dist, 0.8, True)
    finally:
        ENGINE.set_match_chunk(2048)
    assert chunked.tobytes() == whole.tobytes()
    for m, (fa, fb) in enumerate(pl):   # pairs 0, 15 and 16 are the ends of the two chunks
        exp = ref_select(*ref_knn(descs[fa], descs[fb]), max_dist, 0.8, True)
        assert (chunked[m, :counts[fa]] == exp).all(), m
        assert (chunked[m, counts[fa]:] == 77).all(), m
    assert (chunked[0, :, 1] >= 0).sum() > 40 and (chunked[15, :, 1] >= 0).sum() > 20 and (chunked[16, :133, 1] >= 0).all()


def test_bad_arguments():
    t = torch.zeros(4096, dtype=torch.int32, device=DEV)
    with pytest.raises(pg.ArgumentException):
        ENGINE.knn_batch_dev(t, t, 16, 8, t, 1, 3, t, t)            # k = 3
    with pytest.raises(pg.ArgumentException):
        ENGINE.knn_batch_dev(t, t, 16, 0, t, 1, 2, t, t)            # words = 0
    with pytest.raises(pg.ArgumentException):
        ENGINE.knn_batch_dev(t, t, 16, 128, t, 1, 2, t, t)          # words = 128
    with pytest.raises(pg.ArgumentException):
        ENGINE.match_nn_batch_dev(t, t, 16, 8, t, 1, t, 100, 1.5, False)
    with pytest.raises(pg.ArgumentException):
        ENGINE.match_nn_batch_dev(t, t, 16, 8, t, 1, t, 100, float("nan"), False)
    a = np.zeros((4, 8), np.uint32)
    with pytest.raises(pg.ArgumentException):
        ENGINE.knn(a, a, k=3)
    with pytest.raises(pg.ArgumentException):
        ENGINE.knn(np.zeros((4, 128), np.uint32), np.zeros((4, 128), np.uint32))
    ENGINE.check_status()


# ---- ties to the existing paths -------------------------------------------------------------------------------------------
def test_mutual_nearest_pairs_are_taken_by_the_greedy():
    """cross_check = 1, ratio = 0, no gate: every accepted (i, j1, d1) is in the greedy list of pgx_match_batch_dev."""
    rng = np.random.default_rng(3)
    a, b, _ = synth.true_match_descriptors(4096, 8, 9, flip=0.2)
    descs = [rand_desc(rng, 4096, 8), rand_desc(rng, 4096, 8), a, b]
    stride = 4096
    dev = upload(stride, 8, descs)
    pl = [(0, 1), (2, 3)]
    out = run_nn(ENGINE, dev, stride, 8, pl, 10**6, 0.0, True)
    greedy = torch.zeros((len(pl), stride, 3), dtype=torch.int32, device=DEV)
    ENGINE.match_batch_dev(dev[0], dev[2], stride, 8, torch.tensor(pl, dtype=torch.int32, device=DEV), len(pl), greedy)
    ENGINE.check_status()
    greedy = greedy.cpu().numpy()
    for m in range(len(pl)):
        acc = out[m][out[m, :, 1] >= 0]
        assert len(acc) > (3000 if m == 1 else 0), len(acc)
        g = {tuple(r) for r in greedy[m].tolist()}
        assert all(tuple(r) in g for r in acc.tolist()), m


def test_nn_lists_feed_the_track_graph():
    rng = np.random.default_rng(8)
    base, _, _ = synth.true_match_descriptors(600, 8, 4, flip=0.0)
    F, stride = 6, 640
    descs = []
    for f in range(F):   # every frame sees a noisy permuted subset of one scene
        keep = rng.permutation(600)[: 450 + 30 * f]
        bits = np.unpackbits(base[keep].view(np.uint8), axis=1)
        bits ^= (rng.random(bits.shape) < 0.08).astype(np.uint8)
        descs.append(np.ascontiguousarray(np.packbits(bits, axis=1).view(np.uint32)))
    dev = upload(stride, 8, descs)
    counts = dev[3]
    pl = [(i, j) for i in range(F) for j in range(i + 1, F)]
    m = run_nn(ENGINE, dev, stride, 8, pl, 60, 0.8, True)
    M = len(pl)
    off, nod, tof, s = run_tracks(ENGINE, counts, pl, m, stride, 60, 2)
    e_off, e_nodes, e_tof, e_s = tracks_np.tracks_arrays(counts, pl, m, stride, 60, 2)
    assert (off == e_off).all() and (nod == e_nodes).all() and (tof == e_tof).all()
    assert s[0] == e_s["n_tracks"] > 100 and s[1] == e_s["n_nodes"]
    host, dropped, dropped_nodes = pg.tracks_host(counts, pl, [m[p] for p in range(M)], 60, 2)
    assert host == as_lists(off, nod)
    assert (dropped, dropped_nodes) == (s[2], s[3])


# ---- the bench job's size -------------------------------------------------------------------------------------------------
def test_bench_size_sample_and_repeatability():
    F, N = 64, 4096
    rng = np.random.default_rng(64)
    desc = rng.integers(0, 2**32, size=(F, N, 8), dtype=np.uint32)
    dev = upload(N, 8, desc)
    pl = [(i, j) for i in range(F) for j in range(i + 1, F)]
    r1 = run_knn(ENGINE, dev, N, 8, pl, 2, True)
    r2 = run_knn(ENGINE, dev, N, 8, pl, 2, True)
    for x, y in zip(r1, r2):
        assert x.tobytes() == y.tobytes()
    for m in rng.choice(len(pl), 16, replace=False):
        a, b = pl[m]
        r_idx, r_dist, r_col = ref_knn(desc[a], desc[b], block=256)
        assert (r1[0][m] == r_idx).all() and (r1[1][m] == r_dist).all() and (r1[2][m] == r_col).all(), (a, b)
