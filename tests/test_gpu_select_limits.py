"""GPU tests of the pair selection (csrc/k_vocab.hip: pgx_select_pairs_dev) past the launch limits that tests/test_gpu_select_pairs.py
stays below: several histogram chunks per workgroup of k_sel_scores (wpb of 512 and 768, the shape class of tools/bench_pairs.py),
both uint16 halves of a histogram cell at 65535, the top-k threshold search on rows of more than 256 candidates that all tie,
ncand at top_k and one above it, the capacity cut inside the second 256-block of a row of k_sel_write, max_pairs == 0,
min_score <= 0, top_k >= 4096 and window >= F.  The shapes, the launch rules they restate and the proof that each shape reaches
its path are tests/pairs_limits_cases.py and tests/test_pairs_limits_cases.py; each test asserts its path again from those
rules.  Every output is an integer and is compared entry by entry with tests/pairs_ref.py, sentinel entries included.

Wall time on an MI355X: 6.4 s of pytest time for the file's 44 tests, 5 s of it the six yardstick runs of the multi-chunk
collections (0.8 to 0.9 s each, computed once per collection and weighting and shared); every other case takes 0.01 to 0.05 s."""
import numpy as np
import pytest
import torch

import pairs_limits_cases as pc
import pairs_ref as R
from pairs_gpu import I32, SENTINEL, check_select, dev_i32, dev_u32, same_selection
import photogrammetry_amd as pg

pytestmark = pytest.mark.gpu

ENGINE = None
GUARD = 700          # rows behind max_pairs that must keep their sentinel


@pytest.fixture(scope="module", autouse=True)
def _engine():
    global ENGINE
    ENGINE = pg.Engine(0)
    yield
    ENGINE.close()
    ENGINE = None


def run_guarded(desc, counts, vocab, weighting, top_k, window, min_score, max_pairs, null_lists=False):
    """pairs_gpu.run_select with GUARD sentinel rows behind max_pairs (returned as `behind`), or without any list at all"""
    F, S = desc.shape[:2]
    d_desc, d_counts, d_vocab = dev_u32(desc), dev_i32(counts), dev_u32(vocab)
    pl, ps = torch.full((max_pairs + GUARD, 2), SENTINEL, **I32), torch.full((max_pairs + GUARD,), SENTINEL, **I32)
    sc, summary = torch.full((F, F), SENTINEL, **I32), torch.full((8,), SENTINEL, **I32)
    torch.cuda.synchronize()
    ENGINE.select_pairs_dev(d_desc, d_counts, F, S, d_vocab, len(vocab), max_pairs, None if null_lists else pl, None if null_lists else ps,
                            summary, weighting=weighting, top_k=top_k, window=window, min_score=min_score, d_scores=sc)
    capacity = False
    try:
        ENGINE.check_status()
    except pg.CapacityError:
        capacity = True
    pl, ps = pl.cpu().numpy(), ps.cpu().numpy()
    return dict(pairlist=pl[:max_pairs], pair_score=ps[:max_pairs], scores=sc.cpu().numpy(), summary=summary.cpu().numpy(),
                capacity=capacity, behind=np.concatenate([pl[max_pairs:].ravel(), ps[max_pairs:]]))


# ---- several histogram chunks per workgroup -------------------------------------------------------------------------------------------
CHUNK_SEL = dict(top_k=3, window=0, min_score=1)


@pytest.fixture(scope="module")
def chunk_refs():
    """(F, V, weighting, with the planted words) -> (desc, counts, vocab, the yardstick's selection), computed once"""
    cache = {}

    def get(F, V, weighting, planted=True):
        key = (F, V, weighting, planted)
        if key not in cache:
            desc, counts, vocab = pc.chunk_collection(F, V, planted)
            cache[key] = (desc, counts, vocab, R.select(desc, counts, vocab, weighting, max_pairs=3 * F + 3, **CHUNK_SEL))
        return cache[key]
    return get


@pytest.mark.parametrize("scores", [True, False])
@pytest.mark.parametrize("weighting", [0, 1])
@pytest.mark.parametrize("shape", sorted(pc.CHUNK_SHAPES))
def test_several_chunks_per_workgroup(chunk_refs, shape, weighting, scores):
    F, V = shape
    tri, chunks, wpb, nz, last = pc.score_split(F, V)
    assert (wpb, nz, last) == {(257, 3329): (512, 7, 257), (529, 1537): (768, 3, 1)}[shape] and wpb > pc.SEL_WC
    desc, counts, vocab, ref = chunk_refs(F, V, weighting)
    check_select(ENGINE, desc, counts, vocab, weighting=weighting, max_pairs=3 * F + 3, scores=scores, ref=ref, **CHUNK_SEL)
    assert ref["summary"][0] > F and ref["summary"][1] == F - 2


@pytest.mark.parametrize("shape", sorted(pc.CHUNK_SHAPES))
def test_a_word_of_a_later_chunk_counts(chunk_refs, shape):
    """Each planted word -- the last of a first chunk, the first of a second (and third) chunk, the single word of the ragged
    tail -- is held by two frames alone: their score differs from the run in which the word is not there."""
    F, V = shape
    wpb = pc.score_split(F, V)[2]
    assert {pc.chunk_place(w, wpb)[1:] for w, _ in pc.CHUNK_SHAPES[shape]} >= {(0, 255), (1, 0)}
    desc, counts, vocab, ref = chunk_refs(F, V, 1)
    bare, bcounts, _, bref = chunk_refs(F, V, 1, planted=False)
    check_select(ENGINE, desc, counts, vocab, weighting=1, max_pairs=3 * F + 3, ref=ref, **CHUNK_SEL)
    check_select(ENGINE, bare, bcounts, vocab, weighting=1, max_pairs=3 * F + 3, ref=bref, **CHUNK_SEL)
    for w, (a, b) in pc.CHUNK_SHAPES[shape]:
        assert ref["scores"][a, b] > bref["scores"][a, b] >= 0, (w, a, b)
        assert ref["scores"][b, a] == ref["scores"][a, b]


# ---- the uint16 halves of a histogram cell ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", pc.HALVES)
@pytest.mark.parametrize("weighting", [0, 1])
def test_histogram_halves_at_65535(case, weighting):
    """65535 descriptors of one slot in one word, in the low half and in the high half of a cell, with the other half of the
    same cell at 65535 in another slot's row, and in the last word of an odd vocabulary, whose cell's high half is padding."""
    V, w0, w1 = case
    desc, counts, vocab = pc.halves_case(V, w0, w1)
    assert desc.shape[1] == 65535 and pc.half_of(0, V, w0)[1] == w0 % 2
    ref = check_select(ENGINE, desc, counts, vocab, weighting=weighting, top_k=2, window=0, min_score=1)
    if w0 != w1:
        assert ref["scores"][0, 1] == 0 and ref["scores"][1, 0] == 0
    elif weighting == 0:
        assert ref["scores"][0, 1] == 1 << 20
    assert ref["scores"][0, 2] >= 0 and ref["scores"][1, 2] >= 0 and (weighting == 1 or ref["scores"][0, 2] > 0)


# ---- long tied rows ---------------------------------------------------------------------------------------------------------------------
F_T = pc.TIED_F
N_LIVE = F_T - len(pc.TIED_EMPTY)


@pytest.mark.parametrize("top_k", [1, 255, 256, 257, F_T - 2, F_T - 1, F_T, 4096, 100000])
def test_rows_of_600_tied_candidates(top_k):
    """Every score is 2^20: bit 32 of every key is set and the order is 4095 - b alone, across the thread stride of the
    threshold search.  top_k >= ncand = 599 selects every candidate."""
    desc, counts, vocab = pc.tied_case()
    assert F_T > 2 * 256
    ref = check_select(ENGINE, desc, counts, vocab, weighting=0, top_k=top_k, window=0, min_score=1)
    assert ref["scores"][0, 1] == 1 << 20 and ref["scores"][F_T - 1, F_T - 2] == 1 << 20
    if top_k == 1:
        assert ref["summary"][0] == F_T - 1 and (ref["pairlist"][:F_T - 1, 0] == 0).all()
    if top_k >= F_T - 1:
        assert ref["summary"][0] == F_T * (F_T - 1) // 2


@pytest.mark.parametrize("top_k", [1, 256, N_LIVE - 2, N_LIVE - 1, N_LIVE])
def test_tied_rows_with_empty_slots(top_k):
    """595 live slots: a live row has 594 candidates, so ncand is top_k + 1, top_k and top_k - 1 over the last three cases."""
    desc, counts, vocab = pc.tied_case(pc.TIED_EMPTY)
    ref = check_select(ENGINE, desc, counts, vocab, weighting=0, top_k=top_k, window=0, min_score=1)
    assert ref["summary"][1] == N_LIVE and (ref["scores"][list(pc.TIED_EMPTY)] == -1).all()
    if top_k >= N_LIVE - 1:
        assert ref["summary"][0] == N_LIVE * (N_LIVE - 1) // 2
    if top_k == N_LIVE - 2:                      # every live row leaves out its last candidate; (a, b) goes unless both do
        assert 0 < N_LIVE * (N_LIVE - 1) // 2 - ref["summary"][0] <= 2


# ---- capacity and parameters ------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def grouped():
    desc, counts, vocab = pc.grouped_case()
    full = R.select(desc, counts, vocab, 1, 2, pc.GROUPED_F, 1, pc.GROUPED_F * (pc.GROUPED_F - 1) // 2)
    return desc, counts, vocab, full


def test_capacity_cut_past_the_first_block_of_a_row(grouped):
    desc, counts, vocab, full = grouped
    n = int(full["summary"][0])
    row = np.bincount(full["pairlist"][:n, 0], minlength=pc.GROUPED_F)
    assert row[0] > 256 + 10 and row[1] > 0      # row 0 of k_sel_write has a second block of 256
    for max_pairs in (256 + 10, int(row[0]), int(row[0] + row[1]), n - 1, n):
        ref = R.select(desc, counts, vocab, 1, 2, pc.GROUPED_F, 1, max_pairs)
        got = run_guarded(desc, counts, vocab, 1, 2, pc.GROUPED_F, 1, max_pairs)
        same_selection(got, ref)
        assert got["capacity"] == (max_pairs < n) and got["summary"][0] == n
        assert (got["pairlist"] == full["pairlist"][:max_pairs]).all() and (got["pair_score"] == full["pair_score"][:max_pairs]).all()
        assert (got["behind"] == SENTINEL).all()
    ENGINE.check_status()


@pytest.mark.parametrize("null_lists", [True, False])
def test_no_room_for_any_pair(grouped, null_lists):
    """max_pairs == 0: k_sel_fill is not launched and k_sel_write writes nothing, with the list pointers null or real."""
    desc, counts, vocab, full = grouped
    got = run_guarded(desc, counts, vocab, 1, 2, pc.GROUPED_F, 1, 0, null_lists=null_lists)
    same_selection(got, R.select(desc, counts, vocab, 1, 2, pc.GROUPED_F, 1, 0))
    assert got["capacity"] and got["summary"][0] == full["summary"][0] > 0 and (got["behind"] == SENTINEL).all()
    assert (got["scores"] == full["scores"]).all()


@pytest.mark.parametrize("min_score", [0, -5])
def test_min_score_of_zero_and_below(grouped, min_score):
    """score-0 pairs become candidates: frames of two groups share no word"""
    desc, counts, vocab, _ = grouped
    ref = check_select(ENGINE, desc, counts, vocab, weighting=1, top_k=40, window=0, min_score=min_score)
    strict = R.select(desc, counts, vocab, 1, 40, 0, 1, 10)
    assert ref["summary"][5] == 0 and ref["summary"][0] > strict["summary"][0] and (ref["pair_score"][:ref["summary"][0]] == 0).any()


@pytest.mark.parametrize("window", [pc.GROUPED_F - 1, pc.GROUPED_F, 10 * pc.GROUPED_F])
def test_window_as_wide_as_the_collection(grouped, window):
    desc, counts, vocab, _ = grouped
    ref = check_select(ENGINE, desc, counts, vocab, weighting=1, top_k=1, window=window, min_score=1)
    live = int((counts > 0).sum())
    assert ref["summary"][0] == live * (live - 1) // 2 and ref["summary"][4] > 0
