"""What the GPU tests of the vocabulary and the pair selection share (test_gpu_vocab.py, test_gpu_select_pairs.py): the run
wrappers of the three device entry points with sentinel-filled outputs, and the comparison of a selection with tests/pairs_ref.py.
The engine is always the caller's.  A plain helper module: no test module imports another."""
import numpy as np
import torch

import pairs_ref as R
import photogrammetry_amd as pg

DEV = "cuda:0"
I32 = dict(dtype=torch.int32, device=DEV)
SENTINEL = -77


def dev_u32(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint32).view(np.int32)).to(DEV)


def dev_i32(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).to(DEV)


def run_quantize(engine, desc, counts, vocab, dist=True):
    """pgx_vocab_quantize_dev -> word, wdist [F][stride] (wdist None without dist); untouched entries hold SENTINEL"""
    F, S = desc.shape[:2]
    d_desc, d_counts, d_vocab = dev_u32(desc), dev_i32(counts), dev_u32(vocab)
    word = torch.full((F, S), SENTINEL, **I32)
    wd = torch.full((F, S), SENTINEL, **I32) if dist else None
    torch.cuda.synchronize()
    engine.vocab_quantize_dev(d_desc, d_counts, F, S, d_vocab, len(vocab), word, wd)
    engine.check_status()
    return word.cpu().numpy(), (wd.cpu().numpy() if dist else None)


def check_quantize(engine, desc, counts, vocab, dist=True):
    """the library against the yardstick, entry by entry, the untouched entries included -> (word, wdist)"""
    word, wd = run_quantize(engine, desc, counts, vocab, dist)
    F, S = desc.shape[:2]
    r_word, r_wd = R.quantize(desc, counts, vocab, np.full((F, S), SENTINEL), np.full((F, S), SENTINEL))
    assert (word == r_word).all(), "word: %d entries differ" % int((word != r_word).sum())
    if dist:
        assert (wd == r_wd).all(), "wdist"
    return r_word, r_wd


def run_train(engine, desc, counts, V, iters, seed):
    """pgx_vocab_train_dev -> vocab [V][8] uint32 (SENTINEL where not written), report [4]"""
    F, S = desc.shape[:2]
    d_desc, d_counts = dev_u32(desc), dev_i32(counts)
    vocab, report = torch.full((V, 8), SENTINEL, **I32), torch.full((4,), SENTINEL, **I32)
    torch.cuda.synchronize()
    engine.vocab_train_dev(d_desc, d_counts, F, S, V, vocab, report, iters=iters, seed=seed)
    engine.check_status()
    return vocab.cpu().numpy().view(np.uint32), report.cpu().numpy()


def run_select(engine, desc, counts, vocab, weighting, top_k, window, min_score, max_pairs, scores=True):
    """pgx_select_pairs_dev -> dict(pairlist, pair_score, scores or None, summary, capacity); capacity: pgx_check_status
    answered PGX_E_CAPACITY"""
    F, S = desc.shape[:2]
    d_desc, d_counts, d_vocab = dev_u32(desc), dev_i32(counts), dev_u32(vocab)
    pl, ps = torch.full((max(max_pairs, 1), 2), SENTINEL, **I32), torch.full((max(max_pairs, 1),), SENTINEL, **I32)
    sc = torch.full((F, F), SENTINEL, **I32) if scores else None
    summary = torch.full((8,), SENTINEL, **I32)
    torch.cuda.synchronize()
    engine.select_pairs_dev(d_desc, d_counts, F, S, d_vocab, len(vocab), max_pairs, pl, ps, summary, weighting=weighting,
                            top_k=top_k, window=window, min_score=min_score, d_scores=sc)
    capacity = False
    try:
        engine.check_status()
    except pg.CapacityError:
        capacity = True
    return dict(pairlist=pl.cpu().numpy()[:max_pairs], pair_score=ps.cpu().numpy()[:max_pairs],
                scores=sc.cpu().numpy() if scores else None, summary=summary.cpu().numpy(), capacity=capacity)


def same_selection(got, ref):
    assert (got["summary"] == ref["summary"]).all(), (got["summary"], ref["summary"])
    assert got["capacity"] == ref["capacity"]
    assert (got["pairlist"] == ref["pairlist"]).all(), "pairlist"
    assert (got["pair_score"] == ref["pair_score"]).all(), "pair_score"
    if got["scores"] is not None:
        assert (got["scores"] == ref["scores"]).all(), "scores"


def check_select(engine, desc, counts, vocab, weighting=1, top_k=3, window=0, min_score=1, max_pairs=None, scores=True, ref=None):
    """the library against the yardstick (computed here unless given) -> the yardstick's result"""
    F = desc.shape[0]
    max_pairs = F * (F - 1) // 2 + 3 if max_pairs is None else max_pairs   # + 3: rows behind the count, filled with -1
    if ref is None:
        ref = R.select(desc, counts, vocab, weighting, top_k, window, min_score, max_pairs)
    same_selection(run_select(engine, desc, counts, vocab, weighting, top_k, window, min_score, max_pairs, scores), ref)
    return ref


def slots(sets, stride):
    """per-slot descriptor sets -> (desc [F][stride][8] with random rows behind every set, counts [F])"""
    rng = np.random.default_rng(len(sets) * 1000 + stride)
    desc = R.random_desc(rng, len(sets) * stride).reshape(len(sets), stride, 8)
    for f, d in enumerate(sets):
        desc[f, :len(d)] = d
    return desc, np.array([len(d) for d in sets], dtype=np.int32)
