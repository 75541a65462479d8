"""GPU tests of the pair selection (pgx_select_pairs_dev, pgx_select_pairs; include/pgx.h): the scores, the nominations, the window,
the compacted list and the summary, entry by entry against tests/pairs_ref.py, and the planted scene as one chain from training
to the exact matcher."""
import numpy as np
import pytest
import torch

import pairs_ref as R
from pairs_gpu import I32, check_select, dev_i32, dev_u32, run_select, run_train, same_selection, slots
import photogrammetry_amd as pg

pytestmark = pytest.mark.gpu

ENGINE = None


@pytest.fixture(scope="module", autouse=True)
def _engine():
    global ENGINE
    ENGINE = pg.Engine(0)
    yield
    ENGINE.close()
    ENGINE = None


def rnd(seed, n):
    return R.random_desc(np.random.default_rng(seed), n)


def collection(seed, F, n=40, stride=48, V=64, empty=()):
    """F frames of n descriptors drawn near V random words, so that frames share words; -> desc, counts, vocab"""
    rng = np.random.default_rng(seed)
    vocab = R.random_desc(rng, V)
    sets = []
    for f in range(F):
        k = 0 if f in empty else int(rng.integers(n // 2, n + 1))
        d = vocab[rng.integers(0, max(1, V // 2), size=k) + (f % 3) * (V // 8)].copy()
        d[:, 0] ^= (1 << rng.integers(0, 32, size=k)).astype(np.uint32)
        sets.append(d)
    desc, counts = slots(sets, stride)
    return desc, counts, vocab


# ---- the planted scene: train -> select -> match ------------------------------------------------------------------------------
@pytest.mark.parametrize("weighting", [0, 1])
def test_planted_scene_chain(weighting):
    desc, counts, group = R.planted_scene(11)
    F, S = desc.shape[:2]
    d_desc, d_counts = dev_u32(desc), dev_i32(counts)
    d_vocab, d_report = torch.zeros((1024, 8), **I32), torch.zeros((4,), **I32)
    d_pl, d_ps, d_sum = torch.zeros((300, 2), **I32), torch.zeros((300,), **I32), torch.zeros((8,), **I32)
    torch.cuda.synchronize()
    ENGINE.vocab_train_dev(d_desc, d_counts, F, S, 1024, d_vocab, d_report, iters=2, seed=1)
    ENGINE.select_pairs_dev(d_desc, d_counts, F, S, d_vocab, 1024, 300, d_pl, d_ps, d_sum, weighting=weighting, top_k=5, window=0,
                            min_score=1)
    ENGINE.check_status()
    want = R.within_group_pairs(group)
    M = int(d_sum[0])
    assert M == 60 and (d_pl.cpu().numpy()[:60] == want).all() and (d_pl.cpu().numpy()[60:] == -1).all()
    r_vocab, r_report = R.train(desc, counts, 1024, 2, 1)
    assert (d_vocab.cpu().numpy().view(np.uint32) == r_vocab).all() and d_report.cpu().numpy().tolist() == r_report.tolist()
    ref = R.select(desc, counts, r_vocab, weighting, 5, 0, 1, 300)
    assert (d_ps.cpu().numpy() == ref["pair_score"]).all() and (d_sum.cpu().numpy() == ref["summary"]).all()
    # the list goes to the exact matcher as it is: within a group 70 % of the descriptors have a partner 16 bits away at most
    d_out = torch.full((M, S, 3), -7, **I32)
    ENGINE.match_nn_batch_dev(d_desc, d_counts, S, 8, d_pl, M, d_out, 40, 0.0, True)
    ENGINE.check_status()
    out = d_out.cpu().numpy()
    matched = (out[:, :, 1] >= 0).sum(axis=1)
    assert (out[:, :, 0] == np.arange(S)[None, :]).all() and (matched >= 300).all() and (matched <= 358).all(), matched


# ---- sizes and parameters -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("F", [1, 2, 3, 17])
@pytest.mark.parametrize("weighting", [0, 1])
def test_small_collections(F, weighting):
    desc, counts, vocab = collection(F, F)
    for top_k in sorted({0, 1, max(F - 1, 0), F + 5}):
        for window in sorted({0, 1, F}):
            check_select(ENGINE, desc, counts, vocab, weighting=weighting, top_k=top_k, window=window)


def test_the_largest_collection():
    """F = 4096: 256 x 256 score tiles, the whole key array of the top-k kernel, empty slots throughout."""
    F = 4096
    rng = np.random.default_rng(5)
    vocab = R.random_desc(rng, 16)
    desc = vocab[rng.integers(0, 16, size=(F, 4))]
    counts = rng.integers(0, 5, size=F).astype(np.int32)
    ref = check_select(ENGINE, desc, counts, vocab, weighting=1, top_k=2, window=3, max_pairs=70000)
    assert 10000 < ref["summary"][0] < 70000 and ref["summary"][4] > 0 and ref["summary"][1] < F


def test_vocabulary_past_one_histogram_chunk_and_odd():
    desc, counts, _ = collection(7, 9, n=60, stride=64)
    vocab = rnd(8, 777)   # odd: the histogram row is padded; four chunks of 256 words, the last ragged
    vocab[:40] = desc[0, :40]
    check_select(ENGINE, desc, counts, vocab, top_k=2)


def test_ties_of_the_score_go_to_the_smaller_index():
    """Identical frames score 2^20 with each other: with top_k = 1 each nominates the smallest other index."""
    desc, counts, vocab = collection(9, 6)
    for f in (1, 3, 4):
        desc[f], counts[f] = desc[0], counts[0]
    ref = check_select(ENGINE, desc, counts, vocab, top_k=1)
    assert ref["scores"][0, 1] == ref["scores"][3, 4] == 1 << 20
    pairs = ref["pairlist"][:ref["summary"][0]].tolist()
    assert [0, 1] in pairs and [0, 3] in pairs and [0, 4] in pairs and [3, 4] not in pairs and [1, 3] not in pairs


def test_min_score_at_a_pair_and_one_above():
    desc, counts, vocab = collection(10, 5)
    sc = R.select(desc, counts, vocab, 1, 4, 0, 0, 20)["scores"]
    s = int(sc[1, 2])
    assert s > 0
    at = check_select(ENGINE, desc, counts, vocab, top_k=9, min_score=s)
    above = check_select(ENGINE, desc, counts, vocab, top_k=9, min_score=s + 1)
    assert [1, 2] in at["pairlist"].tolist() and [1, 2] not in above["pairlist"].tolist()
    assert at["summary"][5] == s and above["summary"][5] > s


def test_empty_slots_in_the_middle():
    desc, counts, vocab = collection(11, 8, empty=(2, 3, 6))
    counts[3] = -4
    ref = check_select(ENGINE, desc, counts, vocab, top_k=2, window=2)
    assert ref["summary"][1] == 5 and (ref["scores"][2] == -1).all() and (ref["scores"][:, 6] == -1).all()
    assert not {2, 3, 6} & set(ref["pairlist"][:ref["summary"][0]].ravel().tolist())


def test_all_weights_zero():
    """V = 2 with every frame holding both words: df == Fv, every weight and every score is 0, nothing is nominated."""
    vocab = rnd(12, 2)
    desc, counts = slots([np.concatenate([vocab, vocab[:1]])] * 5, 4)
    ref = check_select(ENGINE, desc, counts, vocab, weighting=1, top_k=3, window=0, min_score=1)
    assert ref["summary"].tolist() == [0, 5, 0, 2, 0, -1, 0, 0] and ref["scores"].max() == 0
    ref = check_select(ENGINE, desc, counts, vocab, weighting=1, top_k=3, window=1, min_score=1)
    assert ref["summary"][0] == 4 == ref["summary"][4]


def test_capacity():
    desc, counts, vocab = collection(13, 7)
    full = R.select(desc, counts, vocab, 1, 2, 1, 1, 30)
    n = int(full["summary"][0])
    assert 6 < n < 21
    exact = check_select(ENGINE, desc, counts, vocab, top_k=2, window=1, max_pairs=n)
    assert not exact["capacity"]
    cut = check_select(ENGINE, desc, counts, vocab, top_k=2, window=1, max_pairs=n - 1)
    assert cut["capacity"] and cut["summary"][0] == n and (cut["pairlist"] == full["pairlist"][:n - 1]).all()
    ENGINE.check_status()   # the flag was cleared by the check that reported it


def test_without_the_score_matrix_and_repeated():
    desc, counts, vocab = collection(14, 12)
    ref = check_select(ENGINE, desc, counts, vocab, top_k=3, scores=False)
    check_select(ENGINE, desc, counts, vocab, top_k=3, scores=True, ref=ref)
    check_select(ENGINE, desc, counts, vocab, top_k=3, scores=False, ref=ref)


def test_host_forms_equal_the_device_forms():
    desc, counts, vocab = collection(15, 10)
    ref = R.select(desc, counts, vocab, 1, 3, 1, 1, 45)
    n = int(ref["summary"][0])
    for _ in range(2):
        for scores in (True, False):
            r = ENGINE.select_pairs(desc, counts, vocab, weighting=1, top_k=3, window=1, min_score=1, scores=scores)
            assert (r["summary"] == ref["summary"]).all() and len(r["pairs"]) == n
            assert (r["pairs"] == ref["pairlist"][:n]).all() and (r["pair_score"] == ref["pair_score"][:n]).all()
            assert (r["scores"] is None) if not scores else (r["scores"] == ref["scores"]).all()
    with pytest.raises(pg.CapacityError):
        ENGINE.select_pairs(desc, counts, vocab, weighting=1, top_k=3, window=1, min_score=1, max_pairs=n - 1)
    hv, hrep = ENGINE.vocab_train(desc, counts, 16, iters=2, seed=4)
    dv, drep = run_train(ENGINE, desc, counts, 16, 2, 4)
    assert (hv == dv).all() and hrep.tolist() == drep.tolist()


def test_bad_arguments():
    desc, counts, vocab = collection(16, 3)
    ok = dict(weighting=1, top_k=1, window=0, min_score=1, max_pairs=3)
    for bad in (dict(weighting=2), dict(weighting=-1), dict(top_k=-1), dict(window=-1), dict(max_pairs=-1)):
        with pytest.raises(pg.ArgumentException):
            run_select(ENGINE, desc, counts, vocab, **{**ok, **bad})
    d, c, v = dev_u32(desc), dev_i32(counts), dev_u32(vocab)
    pl, ps, sm = torch.zeros((3, 2), **I32), torch.zeros((3,), **I32), torch.zeros((8,), **I32)
    for F, S, V in [(0, 48, 64), (4097, 48, 64), (3, 0, 64), (3, 65536, 64), (3, 48, 0), (3, 48, 65537)]:
        with pytest.raises(pg.ArgumentException):
            ENGINE.select_pairs_dev(d, c, F, S, v, V, 3, pl, ps, sm)
    with pytest.raises(pg.ArgumentException):
        ENGINE.select_pairs_dev(d, c, 3, 48, v, 64, 3, None, ps, sm)
    same_selection(run_select(ENGINE, desc, counts, vocab, **ok), R.select(desc, counts, vocab, 1, 1, 0, 1, 3))
