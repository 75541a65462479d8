"""GPU tests of the vocabulary quantiser and trainer (csrc/k_vocab.hip: pgx_vocab_quantize_dev, pgx_vocab_train_dev) past the launch
limits that tests/test_gpu_vocab.py stays below: pgx_xcd_map's first branch (F >= 8) together with more than one row block per
slot and F % 8 != 0, the stride limit of 65535 (256 row blocks per slot), and the slot scan's carry (F > 256) feeding the
trainer's rank-to-slot search over runs of empty slots.  The shapes, the launch rules they restate and the proof that each shape
reaches its path are tests/pairs_limits_cases.py and tests/test_pairs_limits_cases.py; each test asserts its path again from
those rules.  Every output is an integer and is compared entry by entry with tests/pairs_ref.py, sentinel entries included.

Wall time on an MI355X: 3.0 s of pytest time for the file's 21 tests; the slowest is F = 17, S = 515, V = 4097 at 0.42 s, almost
all of it the yardstick; the quantiser at the stride limit takes 0.12 s."""
import pytest

import pairs_limits_cases as pc
import pairs_ref as R
from pairs_gpu import SENTINEL, check_quantize, run_train
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


# ---- the quantiser's block map ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("V", pc.QUANT_V)
@pytest.mark.parametrize("S", pc.QUANT_S)
@pytest.mark.parametrize("F", pc.QUANT_F)
def test_block_map_with_several_row_blocks(F, S, V):
    """F >= 8 and nrb of 2 and 3: both branches of pgx_xcd_map with a non-trivial split; counts of 0, below 0, 256, 257 and
    above the stride; distinct data per slot, so a workgroup that took another slot's rows or left a block out shows."""
    desc, counts, vocab = pc.quantiser_case(F, S, V)
    nrb = pc.nrb(S)
    assert F >= 8 and nrb >= 2 and sorted(pc.xcd_map(l, nrb, F) for l in range(nrb * F)) == [(f, b) for f in range(F) for b in range(nrb)]
    work = pc.working_blocks(F, S, counts)
    assert any(f < (F & ~7) and b == nrb - 1 for f, b in work) and (F % 8 == 0 or any(f >= (F & ~7) and b == nrb - 1 for f, b in work))
    word, wd = check_quantize(ENGINE, desc, counts, vocab)
    n = R.clamp_counts(counts, S)
    for f in range(F):
        assert (word[f, :n[f]] != SENTINEL).all() and (word[f, n[f]:] == SENTINEL).all() and (wd[f, n[f]:] == SENTINEL).all()
    assert word[F - 1, S - 1] == V - 1 and wd[F - 1, S - 1] == 0 and word[0, pc.VOC_BM] == 0 and wd[0, pc.VOC_BM] == 0


def test_quantiser_at_the_stride_limit():
    """S = 65535: 256 row blocks per slot, the last with 255 rows; a slot that ends one row into the last block."""
    desc, counts, vocab = pc.stride_limit_case()
    assert desc.shape[1] == 65535 and pc.nrb(65535) == 256
    word, wd = check_quantize(ENGINE, desc, counts, vocab)
    for f, i, w in pc.STRIDE_LIMIT_ROWS:
        assert word[f, i] == w and wd[f, i] == 0, (f, i)
    assert (word[0] != SENTINEL).all() and (word[2] != SENTINEL).all() and (word[1, 65281:] == SENTINEL).all()


# ---- training with more than 256 slots -------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def train_data():
    return pc.train_case()


@pytest.mark.parametrize("iters", [0, 2])
@pytest.mark.parametrize("which", ["third", "all"])
def test_training_past_one_scan_pass(train_data, which, iters):
    """F = 600: k_voc_slots' scan takes three passes, and k_voc_train_init's binary search walks offsets that carry over the
    passes, with runs of empty slots at the front, across the index 256 and at the end.  V == N: the vocabulary before the
    first iteration is the data by rank, so every rank is looked up."""
    desc, counts = train_data
    assert pc.scan_passes(len(counts)) == 3
    N = int(counts.sum())
    V = N // 3 if which == "third" else N
    vocab, report = run_train(ENGINE, desc, counts, V, iters, seed=9)
    r_vocab, r_report = R.train(desc, counts, V, iters, 9)
    assert report.tolist() == r_report.tolist() and report[0] == N
    assert (vocab == r_vocab).all(), "%d words differ" % int((vocab != r_vocab).any(1).sum())
    if which == "all" and iters == 0:
        assert (vocab == R.valid_rows(desc, counts)).all()
    # the same valid rows at another stride: the vocabulary must not change
    wide, wcounts = pc.restride(desc, counts, 7)
    v2, rep2 = run_train(ENGINE, wide, wcounts, V, iters, seed=9)
    assert (v2 == r_vocab).all() and rep2.tolist() == r_report.tolist()
