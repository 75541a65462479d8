"""CPU test (no GPU): tests/pairs_ref.py, the numpy yardstick of the vocabulary quantiser, the k-majority trainer and the pair
selection, against a second, independent formulation of each rule, and on the planted scene that the GPU chain runs too."""
import math

import numpy as np
import pytest

import pairs_ref as R


def _rng_desc(seed, n):
    return R.random_desc(np.random.default_rng(seed), n)


def test_quantiser_equals_the_pm1_matrix_product():
    """hamming = (256 - a.b) / 2 for a, b in {-1, +1}^256: a float32 product of +-1 matrices is exact (|sum| <= 256)."""
    X, Vc = _rng_desc(1, 300), _rng_desc(2, 777)
    Vc[500] = Vc[20]          # a duplicate word: the tie goes to the smaller index
    X[7] = Vc[20]             # distance 0
    X[8] = ~Vc[33]            # distance 256 from word 33
    word, dist = R.quantize_rows(X, Vc, budget=1 << 16)   # several row chunks
    A = 1.0 - 2.0 * R.unpack_bits(X).astype(np.float32)
    B = 1.0 - 2.0 * R.unpack_bits(Vc).astype(np.float32)
    D = ((256.0 - A @ B.T) / 2.0).astype(np.int64)
    key = D * (1 << 20) + np.arange(len(Vc))[None, :]
    assert (word == key.argmin(axis=1)).all()
    assert (dist == D.min(axis=1)).all()
    assert word[7] == 20 and dist[7] == 0
    assert (R.popcount32(X[8] ^ Vc[33]).sum() == 256)


def test_quantiser_merges_column_chunks_by_distance_then_index():
    X = _rng_desc(3, 40)
    Vc = _rng_desc(4, 9000)   # three column chunks of 4096
    Vc[8500] = Vc[100]        # the same word in two chunks
    X[0] = Vc[100]
    word, dist = R.quantize_rows(X, Vc)
    D = R.popcount32(X[:, None, :] ^ Vc[None, :, :]).sum(axis=2, dtype=np.int64)
    assert (word == (D * (1 << 20) + np.arange(9000)).argmin(axis=1)).all() and word[0] == 100 and dist[0] == 0


def test_quantize_leaves_entries_past_the_count_alone():
    desc = _rng_desc(5, 3 * 6).reshape(3, 6, 8)
    word, wd = R.quantize(desc, [4, -2, 9], _rng_desc(6, 5), np.full((3, 6), -7), np.full((3, 6), -9))
    assert (word[0, 4:] == -7).all() and (word[1] == -7).all() and (word[2] >= 0).all() and (wd[0, 4:] == -9).all()


def test_bit_order_and_pack_round_trip():
    X = np.zeros((1, 8), dtype=np.uint32)
    X[0, 1] = 1 << 3          # descriptor bit 35
    assert np.flatnonzero(R.unpack_bits(X)[0]).tolist() == [35]
    Y = _rng_desc(7, 10)
    assert (R.pack_bits(R.unpack_bits(Y)) == Y).all()


def test_training_against_a_per_word_loop():
    desc = _rng_desc(8, 4 * 50).reshape(4, 50, 8)
    counts = [50, 0, 37, 60]   # an empty slot and a count above the stride
    X = R.valid_rows(desc, counts)
    assert len(X) == 137
    V = 9
    vocab, report = R.train(desc, counts, V, 2, seed=5)
    v = R.train_init(X, V, 5)
    for j in range(V):         # the initial word of j is drawn inside its own stratum of ranks
        lo, hi = j * 137 // V, (j + 1) * 137 // V
        assert any((X[r] == v[j]).all() for r in range(lo, hi))
    for _ in range(2):
        D = R.popcount32(X[:, None, :] ^ v[None, :, :]).sum(axis=2, dtype=np.int64)
        w = (D * 1024 + np.arange(V)).argmin(axis=1)
        new, changed, empty = v.copy(), 0, 0
        for j in range(V):
            mem = R.unpack_bits(X[w == j]).astype(int)
            if len(mem) == 0:
                empty += 1
                continue
            old = R.unpack_bits(v[j:j + 1])[0]
            ones, c = mem.sum(axis=0), len(mem)
            bits = [1 if 2 * o > c else (0 if 2 * o < c else int(ob)) for o, ob in zip(ones, old)]
            changed += sum(int(b != ob) for b, ob in zip(bits, old))
            new[j] = R.pack_bits(np.array([bits]))[0]
        v = new
    assert (vocab == v).all()
    assert report.tolist() == [137, empty, changed, 0]
    assert R.train(desc, counts, V, 0, seed=5)[1].tolist() == [137, -1, -1, 0]
    assert (R.train(desc, counts, V, 0, seed=6)[0] != R.train(desc, counts, V, 0, seed=5)[0]).any()


def test_weight_rule_against_log2():
    """q = 256 (e - 16) + m with a LINEAR mantissa: log2(1 + t) - t lies in [0, 0.0861] on [0, 1], which is 22.04 units of
    256, and the floor of m costs less than one more: q is never above floor(256 log2(Fv / df)) and at most 23 below it."""
    worst = 0
    for Fv in (1, 2, 3, 24, 64, 1000, 4096):
        prev = None
        for df in range(1, Fv + 1):
            q = R.weight(Fv, df)
            exact = math.floor(256.0 * math.log2(Fv / df))
            assert 0 <= exact - q <= 23, (Fv, df, q, exact)
            worst = max(worst, exact - q)
            assert prev is None or q <= prev, (Fv, df)   # monotone: a rarer word never weighs less
            prev = q
        assert R.weight(Fv, Fv) == 0 and R.weight(Fv, 0) == 0
    assert worst == 23   # the bound is reached: it is the rule's, not slack


def test_scores_dense_against_a_sparse_merge():
    rng = np.random.default_rng(9)
    F, V = 7, 40
    h = rng.integers(0, 4, size=(F, V)) * (rng.random((F, V)) < 0.3)
    h[3] = 0                                   # an empty slot
    h = h.astype(np.int64)
    for weighting in (0, 1):
        q, Fv, df = R.weights(h, weighting)
        assert Fv == 6
        sc = R.score_matrix(h, q)
        for a in range(F):
            for b in range(F):
                if a == b or a == 3 or b == 3:
                    assert sc[a, b] == -1
                    continue
                wa, wb = np.flatnonzero(h[a]).tolist(), np.flatnonzero(h[b]).tolist()
                i = j = s = 0
                while i < len(wa) and j < len(wb):   # two sorted word lists merged
                    if wa[i] == wb[j]:
                        s += int(q[wa[i]]) * min(int(h[a, wa[i]]), int(h[b, wb[j]]))
                        i, j = i + 1, j + 1
                    elif wa[i] < wb[j]:
                        i += 1
                    else:
                        j += 1
                sa = sum(int(q[w]) * int(h[a, w]) for w in wa)
                sb = sum(int(q[w]) * int(h[b, w]) for w in wb)
                assert sc[a, b] == (s << 20) // max(1, min(sa, sb))
        assert (sc == sc.T).all() and sc.max() <= 1 << 20


def test_selection_rules_on_a_hand_made_score_matrix():
    sc = np.array([[-1, 50, 50, 10, -1],
                   [50, -1, 20, 50, -1],
                   [50, 20, -1, 30, -1],
                   [10, 50, 30, -1, -1],
                   [-1, -1, -1, -1, -1]], dtype=np.int64)   # slot 4 is empty
    r = R.select_from_scores(sc, top_k=1, window=0, min_score=1, max_pairs=10)
    # 0 nominates 1 (the tie 50 / 50 goes to the smaller index), 1 nominates 0, 2 nominates 0, 3 nominates 1
    assert r["pairlist"][:r["n"]].tolist() == [[0, 1], [0, 2], [1, 3]] and r["pair_score"][:3].tolist() == [50, 50, 50]
    assert (r["pairlist"][3:] == -1).all() and (r["pair_score"][3:] == -1).all()
    assert r["n_window"] == 0 and r["min_nominated"] == 50 and not r["capacity"]
    r = R.select_from_scores(sc, top_k=0, window=1, min_score=1, max_pairs=2)   # the sliding window, cut
    assert r["n"] == 3 and r["capacity"] and r["pairlist"].tolist() == [[0, 1], [1, 2]] and r["n_window"] == 3
    assert r["min_nominated"] == -1
    r = R.select_from_scores(sc, top_k=9, window=0, min_score=30, max_pairs=10)
    assert r["pairlist"][:r["n"]].tolist() == [[0, 1], [0, 2], [1, 3], [2, 3]] and r["min_nominated"] == 30
    assert R.select_from_scores(sc, top_k=9, window=0, min_score=51, max_pairs=10)["n"] == 0


@pytest.fixture(scope="module")
def scene():
    return R.planted_scene(11)


@pytest.mark.parametrize("weighting", [0, 1])
@pytest.mark.parametrize("iters,V", [(2, 1024), (0, 1024), (2, 1000)])
def test_planted_scene_selects_exactly_the_within_group_pairs(scene, weighting, iters, V):
    """24 frames in 4 groups of 6.  Every frame's 5 best partners must be its group: the smallest within-group score has to
    stay above the largest cross-group score.  The margin is stated here: at least 1 % of the score range (2^20) at iters = 0
    (measured when the rules were written: 3.65e5 against 3.49e5) and 10 % after two iterations (5.4e5 against 3.4e5)."""
    desc, counts, group = scene
    vocab, report = R.train(desc, counts, V, iters, seed=1)
    assert report[0] == 24 * 512
    r = R.select(desc, counts, vocab, weighting, top_k=5, window=0, min_score=1, max_pairs=300)
    want = R.within_group_pairs(group)
    assert len(want) == 60 and r["summary"][0] == 60 and not r["capacity"]
    assert (r["pairlist"][:60] == want).all() and (r["pairlist"][60:] == -1).all()
    same = group[:, None] == group[None, :]
    off = ~np.eye(24, dtype=bool)
    within, cross = r["scores"][same & off].min(), r["scores"][~same].max()
    print("iters %d V %d weighting %d: smallest within-group %d, largest cross-group %d" % (iters, V, weighting, within, cross))
    assert within - cross >= (0.10 if iters else 0.01) * (1 << 20)
    assert r["summary"][5] == within and r["summary"][1] == 24 and r["summary"][4] == 0
