"""The vocabulary quantiser and the exact k = 1 nearest-neighbour matcher are one computation (csrc/pgx_fp4_nn.h is the body of
both k_vocab_fp4 and k_knn_fp4): with the vocabulary as one more frame of the descriptor buffer, pgx_vocab_quantize_dev on the
other slots and pgx_knn_batch_dev with k = 1 on the pairs (slot, vocabulary) give the same words and distances, bit for bit.
Counts at the 256-row block of a workgroup (0, 1, 256, 257 and a full slot of 4100), vocabularies at the 32-column tile and the
4096-column chunk (1, 32, 33, 4096, 4097: a second chunk of one ragged column); words repeat and some descriptors are words, so
ties (the smaller word wins) and distance 0 occur."""
import numpy as np
import pytest

import pairs_ref as R
from match_gpu import run_knn, upload
from pairs_gpu import run_quantize

pytestmark = pytest.mark.gpu

STRIDE = 4100
COUNTS = (0, 1, 256, 257, 4100)
PLANT = 3    # every third descriptor is a word


def scene(V):
    """-> (sets: the descriptors of the len(COUNTS) slots, vocab [V][8], planted: per slot the word each planted row copies)"""
    rng = np.random.default_rng(4100 + V)
    vocab = R.random_desc(rng, V)
    vocab[V - V // 2:] = vocab[:V // 2]                    # the second half repeats the first: every such word ties with its copy
    sets, planted = [], []
    for n in COUNTS:
        near = vocab[rng.integers(0, V, n)] ^ (np.uint32(1) << rng.integers(0, 32, (n, 8)).astype(np.uint32))   # 8 bits off a word
        j = rng.integers(0, V, len(near[::PLANT]))
        near[::PLANT] = vocab[j]
        sets.append(near)
        planted.append(j)
    return sets, vocab, planted


@pytest.mark.parametrize("V", [1, 32, 33, 4096, 4097])
def test_quantiser_equals_knn_against_the_vocabulary_slot(engine, V):
    sets, vocab, planted = scene(V)
    F = len(sets)
    counts = np.array(COUNTS, dtype=np.int32)
    desc = np.zeros((F, STRIDE, 8), dtype=np.uint32)
    for f, d in enumerate(sets):
        desc[f, :len(d)] = d
    word, wdist = run_quantize(engine, desc, counts, vocab)
    # the same buffer with the vocabulary in slot F, every slot paired with it
    idx, dist, _ = run_knn(engine, upload(STRIDE, 8, sets + [vocab]), STRIDE, 8, [(f, F) for f in range(F)], 1, False)
    _, at, inv = np.unique(vocab, axis=0, return_index=True, return_inverse=True)
    first = at[inv.ravel()]                                                      # the smallest index of an equal word
    for f, n in enumerate(COUNTS):
        assert (word[f, :n] == idx[f, :n, 0]).all(), (f, int((word[f, :n] != idx[f, :n, 0]).sum()))
        assert (wdist[f, :n] == dist[f, :n, 0]).all(), f
        assert (word[f, :n:PLANT] == first[planted[f]]).all() and (wdist[f, :n:PLANT] == 0).all(), f   # distance 0, ties downwards
    assert V == 1 or (first != np.arange(V)).any()
