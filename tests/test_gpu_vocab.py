"""GPU tests of the vocabulary quantiser and the k-majority trainer (pgx_vocab_quantize_dev, pgx_vocab_train_dev, pgx_vocab_train;
include/pgx.h) at the limits of k_vocab.hip: the 32-column tile, the 4096-column chunk, the 256-row block of a workgroup.
Every output is an integer and is compared entry by entry with tests/pairs_ref.py; sentinel-filled outputs prove what is left
alone."""
import numpy as np
import pytest
import torch

import pairs_ref as R
from pairs_gpu import I32, SENTINEL, check_quantize, dev_i32, dev_u32, run_quantize, run_train, slots
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


# ---- the quantiser ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("V", [1, 31, 32, 33, 4095, 4096, 4097, 8193, 65536])
def test_vocabulary_sizes(V):
    """Tile and chunk edges of the columns; a slot with count 0, a negative count and a count above the stride; the winner in
    the last column (index 65535 at V = 65536) at distance 0; distance 256 at V = 1."""
    stride = 96
    vocab = rnd(V, V)
    desc = rnd(V + 1, 4 * stride).reshape(4, stride, 8)
    counts = np.array([70, 0, -3, 999], dtype=np.int32)
    desc[0, 0] = vocab[V - 1]
    desc[0, 1] = ~vocab[0]
    desc[3, stride - 1] = vocab[V // 2]
    word, wd = check_quantize(ENGINE, desc, counts, vocab)
    assert word[0, 0] == V - 1 and wd[0, 0] == 0 and word[3, stride - 1] == V // 2
    assert (word[1] == SENTINEL).all() and (word[2] == SENTINEL).all() and (word[0, 70:] == SENTINEL).all()
    assert (word[3] != SENTINEL).all()   # 999 is clamped to the stride
    if V == 1:
        assert wd[0, 1] == 256


@pytest.mark.parametrize("n", [1, 127, 128, 129, 255, 256, 257])
def test_rows_around_the_row_block(n):
    stride = 260
    for V in (33, 4097):
        desc, counts = slots([rnd(n, n), rnd(n + 1, n), rnd(n + 2, 3)], stride)
        check_quantize(ENGINE, desc, counts, rnd(V + n, V))


def test_ties_go_to_the_smaller_word():
    """Duplicate words across a tile edge (31 | 32), across a chunk edge (4095 | 4096) and in two different chunks, at distance
    0 and at distance 3 (a descriptor equidistant from words of two chunks)."""
    V = 8300
    vocab = rnd(1, V)
    vocab[32] = vocab[31]
    vocab[4096] = vocab[4095]
    vocab[6000] = vocab[200]
    vocab[8299] = vocab[4200]
    rows = rnd(2, 50)
    rows[0], rows[1], rows[2], rows[3] = vocab[31], vocab[4095], vocab[200], vocab[4200]
    near = vocab[200].copy()
    near[0] ^= 0b111          # three bits from words 200 and 6000
    rows[4] = near
    near = vocab[4095].copy()
    near[7] ^= 1 << 31
    rows[5] = near
    desc, counts = slots([rows], 64)
    word, wd = check_quantize(ENGINE, desc, counts, vocab)
    assert word[0, :6].tolist() == [31, 4095, 200, 4200, 200, 4095] and wd[0, :6].tolist() == [0, 0, 0, 0, 3, 1]


def test_no_distance_output_and_repeated_calls():
    desc, counts = slots([rnd(3, 300), rnd(4, 17)], 300)
    vocab = rnd(5, 5000)
    first = run_quantize(ENGINE, desc, counts, vocab, dist=False)
    assert first[1] is None
    r_word, _ = check_quantize(ENGINE, desc, counts, vocab)
    assert (first[0] == r_word).all()
    run_train(ENGINE, desc, counts, 64, 1, 0)        # uses the workspace
    again = run_quantize(ENGINE, desc, counts, vocab, dist=True)
    assert (again[0] == r_word).all()


def test_quantiser_bad_arguments():
    desc, counts = slots([rnd(6, 4)], 4)
    vocab = rnd(7, 2)
    d, c, v, w = dev_u32(desc), dev_i32(counts), dev_u32(vocab), torch.zeros((1, 4), **I32)
    for F, S, V in [(0, 4, 2), (4097, 4, 2), (1, 0, 2), (1, 65536, 2), (1, 4, 0), (1, 4, 65537)]:
        with pytest.raises(pg.ArgumentException):
            ENGINE.vocab_quantize_dev(d, c, F, S, v, V, w)
    with pytest.raises(pg.ArgumentException):
        ENGINE.vocab_quantize_dev(d, c, 1, 4, v, 2, None)


# ---- training ----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def train_data():
    return slots([rnd(10, 200), np.zeros((0, 8), np.uint32), rnd(11, 150)], 200)


@pytest.mark.parametrize("iters", [0, 1, 3])
def test_training_iterations(train_data, iters):
    desc, counts = train_data
    vocab, report = run_train(ENGINE, desc, counts, 40, iters, seed=9)
    r_vocab, r_report = R.train(desc, counts, 40, iters, 9)
    assert report.tolist() == r_report.tolist()
    assert (vocab == r_vocab).all()
    assert report[0] == 350 and (iters > 0 or report[1:3].tolist() == [-1, -1])


@pytest.mark.parametrize("V", [9, 8])
def test_as_many_descriptors_as_words_and_one_more(V):
    desc, counts = slots([rnd(12, 5), np.zeros((0, 8), np.uint32), rnd(13, 4)], 6)   # N = 9
    for iters in (0, 1):
        vocab, report = run_train(ENGINE, desc, counts, V, iters, seed=3)
        r_vocab, r_report = R.train(desc, counts, V, iters, 3)
        assert report.tolist() == r_report.tolist() and (vocab == r_vocab).all()
    if V == 9:   # every stratum holds one rank: the vocabulary is the data
        assert (R.train(desc, counts, 9, 0, 3)[0] == R.valid_rows(desc, counts)).all()


def test_fewer_descriptors_than_words():
    desc, counts = slots([rnd(14, 5)], 6)
    with pytest.raises(pg.ArgumentException):
        run_train(ENGINE, desc, counts, 6, 1, seed=0)     # the device form: through pgx_check_status
    with pytest.raises(pg.ArgumentException):
        ENGINE.vocab_train(desc, counts, 6, iters=1)       # the host form: at once
    for iters in (-1, 65):
        with pytest.raises(pg.ArgumentException):
            ENGINE.vocab_train(desc, counts, 2, iters=iters)
    ENGINE.check_status()


def test_a_word_without_members_keeps_its_bits():
    """Identical descriptors give identical words; the tie sends every member to the smallest of them."""
    one = rnd(15, 1)
    desc, counts = slots([np.repeat(one, 8, axis=0)], 8)
    vocab, report = run_train(ENGINE, desc, counts, 4, 2, seed=1)
    assert report.tolist() == [8, 3, 0, 0] == R.train(desc, counts, 4, 2, 1)[1].tolist()
    assert (vocab == one).all()


def test_a_bit_at_exact_equality_keeps_its_old_value():
    """One word, two members: every bit in which they differ has 2 ones == c and stays as the initial word has it."""
    two = rnd(16, 2)
    desc, counts = slots([two], 2)
    for seed in (0, 1, 2, 3):
        vocab, report = run_train(ENGINE, desc, counts, 1, 1, seed=seed)
        r_vocab, r_report = R.train(desc, counts, 1, 1, seed)
        assert (vocab == r_vocab).all() and report.tolist() == r_report.tolist() == [2, 0, 0, 0]
        assert (vocab[0] == two[0]).all() or (vocab[0] == two[1]).all()
    # three members of which two agree: a clear majority moves the word
    three = np.concatenate([two, two[1:]])
    desc, counts = slots([three], 3)
    vocab, _ = run_train(ENGINE, desc, counts, 1, 1, seed=0)
    assert (vocab[0] == two[1]).all()


def test_seeds_and_layouts(train_data):
    desc, counts = train_data
    a, _ = run_train(ENGINE, desc, counts, 40, 2, seed=1)
    b, _ = run_train(ENGINE, desc, counts, 40, 2, seed=2)
    again, _ = run_train(ENGINE, desc, counts, 40, 2, seed=1)
    assert (a != b).any() and (a == again).all()
    wide, wcounts = slots([desc[f, :counts[f]] for f in range(len(counts))], 333)   # the same data at another stride
    c, rep = run_train(ENGINE, wide, wcounts, 40, 2, seed=1)
    assert (a == c).all()
    host, hrep = ENGINE.vocab_train(desc, counts, 40, iters=2, seed=1)               # the host form
    assert (host == a).all() and hrep.tolist() == rep.tolist()
