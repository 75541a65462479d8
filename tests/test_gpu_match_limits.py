"""The greedy Hamming matcher (k_ham_fp4 -> k_match_select -> k_tail_rows_fp4 -> k_match_order / k_match_gs) past the limits
of its arithmetic and blockings: the lower half of the biased accumulator (nearest neighbour further than 128), the tile field
of the key at every column-chunk width, short and ragged last chunks, distance 255 against 256 in the residual byte matrix,
residuals of exactly PGX_TAIL_MAX, a lapping free-row ring, and the finish's two launch forms with its emit paths.

Every comparison is bit-exact against the oracle (cref.match up to a few hundred entries, cref.match_sorted above): k1, k2,
dist, and the sentinel rows behind a list.  Every case first checks what the ORACLE's list says about its input (the property
the case is built for), then that the intended path ran: pgx_match_stats (wide rounds, evaluations of the first round), the
launch counts of the profile hooks, and pgx_debug_counters, to which k_match_gs adds ring pushes [3], scans [4] and
proposals [6] on its fast path only -- the any-size fallback adds none.  What the library does not report -- the column
chunk of k_ham_fp4, the thread count of k_match_gs -- follows from (stride, M) by the host arithmetic that wide_plan mirrors
(DESIGN.md section 4).  k_match_order's `order == nullptr` form needs more than ORDER_MAX = 4096 pairs in one chunk, and a
chunk holds at most 4096: it is unreachable through the ABI and not tested.

The generators (photogrammetry_amd/synth.py: far_descriptors, tiled_ties) are checked without a GPU at the end of the file.
"""
import functools

import numpy as np
import pytest

from knn_ref import dist_matrix, ref_knn
from oracle import cref
from photogrammetry_amd import synth

gpu = pytest.mark.gpu
TAIL_MAX, GS_QN, EM_MAXROWS = 2048, 2048, 4096
SENTINEL = -7


def wide_plan(max_n, M):
    """pgx_enqueue_match's and pgx_launch_ham_mfma's host arithmetic for 256-bit descriptors
    -> (skip_below, wide rounds, cols_per_wg)"""
    skip = TAIL_MAX // 2 if M <= 2 else TAIL_MAX
    rounds, n = 0, max_n
    while n > skip and rounds < 8:
        rounds, n = rounds + 1, (n + 1) // 2
    if 0 < rounds < 8:
        rounds += 1
    rowtiles, cpw = -(-max_n // 384), 4096
    while cpw > 128 and rowtiles * -(-max_n // cpw) * M < 1024:
        cpw //= 2
    return skip, rounds, cpw


def nearest(a, b):
    """(every row's, every column's) smallest distance"""
    D = np.concatenate([dist_matrix(a, b, i, i + 128) for i in range(0, len(a), 128)])
    return D.min(1), D.min(0)


def matched(exp):
    return exp[exp["dist"] != 2**31 - 1]


def run(engine, descs, pl, stride):
    """run_match with every counter read around it -> (lists [M][stride][3], dict of what ran)"""
    from match_gpu import run_match
    engine.debug_counters()          # reading clears them
    engine.profile_reset()
    engine.profile_enable(True)
    try:
        out = run_match(engine, descs, pl, stride, sentinel=SENTINEL)
    finally:
        engine.profile_enable(False)
    rounds, _, evals0 = engine.match_stats()
    dbg = engine.debug_counters()
    return out, dict(rounds=rounds, evals0=evals0, wide=engine.profile_get("ham_argmin")[0],
                     rows=engine.profile_get("tail_rows")[0], finish=engine.profile_get("match_finish")[0],
                     pushes=dbg[3], scans=dbg[4], proposals=dbg[6])


def same(out_m, n1, exp):
    from match_gpu import pairs_equal
    return pairs_equal(out_m[:n1], exp) and bool((out_m[n1:] == SENTINEL).all())


# ---- the inputs, made once and left alone ---------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def far_pair(n1, n2, lo, hi):
    a, b = synth.far_descriptors(n1, n2, lo, hi, 1000 + n1)
    return a, b, cref.match_sorted(a, b)


@functools.lru_cache(maxsize=None)
def tie_pair(n1, n2, period, row_period, seed=0):
    a, b = synth.tiled_ties(n1, n2, period, 31 * n1 + period + seed, row_period)
    return a, b, cref.match_sorted(a, b)


def ties_resolved_both_ways(exp, period):
    """near copies were matched to columns of the repeated blocks AND to their originals: the (dist, k1, k2) rule was needed"""
    m = matched(exp)
    blk = (m["k2"][m["dist"] <= 2] // period) & 1
    return bool((blk == 0).any() and (blk == 1).any())


# ---- 1: the lower half of the accumulator in the wide kernel ---------------------------------------------------------------
@gpu
@pytest.mark.parametrize("n1,n2,lo,hi", [(1100, 1060, 150, 200), (1060, 1100, 150, 200), (1030, 1030, 256, 256),
                                         (1030, 1030, 255, 255)])
def test_wide_kernel_nearest_beyond_128(engine, n1, n2, lo, hi):
    """One image pair (wide rounds from 1025 entries on): every row's and column's nearest lies in [150, 200], or is exactly
    256 / 255 with every distance tied (the all-256 set is ONE prototype against its complement: with two prototypes P, Q the
    cross distances would be 256 - hamming(P, Q) < 256).  k_ham_fp4 decodes `raw - F4_RAW0` NEGATIVE for all of them, on both
    sides."""
    a, b, exp = far_pair(n1, n2, lo, hi)
    rmin, cmin = nearest(a, b)
    assert lo <= rmin.min() and rmin.max() <= hi and lo <= cmin.min() and cmin.max() <= hi
    assert len(matched(exp)) == min(n1, n2) and matched(exp)["dist"].min() >= max(lo, 129)
    out, ran = run(engine, [a, b], [(0, 1)], max(n1, n2))
    rounds = wide_plan(max(n1, n2), 1)[1]
    assert ran["rounds"] == rounds >= 2 and ran["wide"] == rounds and ran["evals0"] == n1 * n2
    # 256 does not fit the byte matrix: the fallback; all else the fast path
    assert ran["scans"] == 0 if lo == 256 else ran["scans"] > 0
    assert same(out[0], n1, exp)


@functools.lru_cache(maxsize=None)
def border_128_pair():
    """1030 x 1030: rows 0 .. 383 (the first row block) are one prototype P, all others P with bit 0 flipped; every column is
    ~P with 127 bits of words 1 .. 7 flipped back: 129 from every row of the first block, 128 from every other row"""
    rng = np.random.default_rng(128)
    a = np.repeat(rng.integers(0, 2**32, (1, 8), dtype=np.uint32), 1030, axis=0)
    b = ~a
    b[:, 1:] = synth.flip_bits(rng, b[:, 1:], 127)
    a[384:, 0] ^= np.uint32(1)
    return a, b, cref.match_sorted(a, b)


@gpu
def test_wide_kernel_distances_on_both_sides_of_128(engine):
    """`raw - F4_RAW0` negative in one row block and not in the next, for the SAME column: a column's candidates of 129 (rows
    0 .. 383) and 128 (rows 384 ..) meet in the atomicMin on its key, where the row block's smaller row numbers win as soon as
    the decode rounds 129 towards 128 (a division for the shift; the far sets above lie wholly below 128 and do not notice).
    The greedy takes rows 384 .. 1029 first, at 128, and only then rows 0 .. 383 at 129."""
    a, b, exp = border_128_pair()
    D = np.concatenate([dist_matrix(a, b, i, i + 128) for i in range(0, 1030, 128)])
    assert (D[:384] == 129).all() and (D[384:] == 128).all()
    assert (exp["k1"] == np.r_[384:1030, 0:384]).all() and (exp["k2"] == np.arange(1030)).all()
    assert (exp["dist"] == np.r_[[128] * 646, [129] * 384]).all()
    out, ran = run(engine, [a, b], [(0, 1)], 1030)
    rounds = wide_plan(1030, 1)[1]
    assert ran["rounds"] == rounds == 2 and ran["wide"] == 2 and ran["evals0"] == 1030 * 1030 and ran["scans"] > 0
    assert same(out[0], 1030, exp)


# ---- 2: the full tile field, cols_per_wg = 4096, ties across tiles, the XCD map ----------------------------------------
TIE_SETS = [(1000, 4096, 32, 384), (868, 4096, 2048, 96), (1000, 4096, 4064, 32)]   # n1, n2, period, row_period


@gpu
@pytest.mark.parametrize("M,cpw", [(96, 4096), (100, 4096), (5, 128)])
def test_wide_kernel_ties_across_tiles(engine, M, cpw):
    """4096 columns in ONE chunk (tile field 127 - ct over its whole range) with every row minimum tied between two tiles
    (period 32), between the halves (2048) and between the first and the last tile (4064); 1000 rows = 384 + 384 + 232 (the
    two-tile form of the last row block), 868 = 384 + 384 + 100 (the one-tile form); rows repeat across the 32-row tile, the
    96 rows of a wavefront and the 384-row block.  The three pairs alternate through the list, so a slip in the workgroup ->
    (pair, row block, chunk) map shows: M = 96 is all groups of 8, M = 100 has the remainder branch, M = 5 only that."""
    sets, exps = [], []
    for n1, n2, period, rp in TIE_SETS:
        a, b, exp = tie_pair(n1, n2, period, rp)
        assert ties_resolved_both_ways(exp, period) and (matched(exp)["dist"] <= 2).mean() > 0.4
        sets += [a, b]
        exps.append(exp)
    pl = [(2 * (m % 3), 2 * (m % 3) + 1) for m in range(M)]
    _, rounds, plan_cpw = wide_plan(4096, M)
    assert plan_cpw == cpw
    out, ran = run(engine, sets, pl, 4096)
    assert ran["rounds"] == rounds == 2 and ran["wide"] == 2
    assert ran["evals0"] == sum(len(sets[a]) * len(sets[b]) for a, b in pl)
    for m in range(M):
        assert same(out[m], TIE_SETS[m % 3][0], exps[m % 3]), m


# ---- 3: intermediate chunk widths, short last chunk ----------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def last_chunk_pair(n2):
    """300 rows against n2 = 2048 + t columns: the t columns of the last chunk alternate between a descriptor of their own,
    which row i equals (its unique best column), and a repeat of column j - 2048, which row 100 + i equals (two columns at
    distance 0: the earlier one must win); every other row is a column with 1 or 2 bits flipped"""
    rng = np.random.default_rng(n2)
    b = synth.repeat_blocks(rng.integers(0, 2**32, (n2, 8), dtype=np.uint32), 2048)
    own, rep = np.arange(2048, n2, 2), np.arange(2049, n2, 2)
    b[own] = rng.integers(0, 2**32, (len(own), 8), dtype=np.uint32)
    a = synth.flip_bits(rng, b[rng.integers(0, n2, 300)], rng.integers(1, 3, 300))
    a[:len(own)] = b[own]
    a[100:100 + len(rep)] = b[rep]
    return a, b, cref.match_sorted(a, b)


@gpu
@pytest.mark.parametrize("M,cpw", [(90, 2048), (40, 512), (6, 128)])
def test_wide_kernel_chunk_widths_and_short_last_chunk(engine, M, cpw):
    """n2 = 2049, 2081, 2145 = cpw k + 1, + 33, + 97 for every chunk width of this test: the last column chunk has 1, 2 and 4
    tiles (fewer than the prefetch ring is deep, and than HAM_PAD), the last tile 1 column."""
    stride, n2s = 2176, (2049, 2081, 2145)
    sets, exps = [], []
    for n2 in n2s:
        a, b, exp = last_chunk_pair(n2)
        k2 = {int(r["k1"]): int(r["k2"]) for r in matched(exp)}
        own, rep = np.arange(2048, n2, 2), np.arange(2049, n2, 2)
        assert all(k2[i] == j for i, j in enumerate(own))                    # unique best columns in the last chunk
        assert all(k2[100 + i] == j - 2048 for i, j in enumerate(rep))       # the earlier of two tied columns
        sets += [a, b]
        exps.append(exp)
    pl = [(2 * (m % 3), 2 * (m % 3) + 1) for m in range(M)]
    _, rounds, plan_cpw = wide_plan(stride, M)
    assert plan_cpw == cpw and [n2 % cpw for n2 in n2s] == [1, 33, 97]
    out, ran = run(engine, sets, pl, stride)
    assert ran["rounds"] == rounds == 2 and ran["wide"] == 2 and ran["evals0"] == sum(300 * n2s[m % 3] for m in range(M))
    for m in range(M):
        assert same(out[m], 300, exps[m % 3]), m


# ---- 4: more than one column chunk at 4096 -------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def border_pair(n2):
    """300 rows against 4096 + t columns: column 4096 + j repeats column j; rows 0 .. 9 ARE columns 0 .. 9 and rows 32 .. 41
    are again, so row 0 takes column 0 and row 32 its repeat in the second chunk"""
    a, b = synth.tiled_ties(300, n2, 4096, n2, 32)
    a[0:10] = b[0:10]
    a[32:42] = b[0:10]
    return a, b, cref.match_sorted(a, b)


@gpu
def test_wide_kernel_two_chunks_of_4096(engine):
    """4097 and 8191 columns at cols_per_wg = 4096: a second chunk of one column and one of 4095, with ties across the chunk
    border.  300 rows keep it cheap; more than 2048 columns stay, so the finish is the any-size fallback."""
    M, stride = 24, 8192
    sets, exps = [], []
    for n2 in (4097, 8191):
        a, b, exp = border_pair(n2)
        k2 = {int(r["k1"]): (int(r["k2"]), int(r["dist"])) for r in matched(exp)}
        assert (b[4096] == b[0]).all() and k2[0] == (0, 0) and k2[32] == (4096, 0)
        assert n2 == 4097 or (k2[5] == (5, 0) and k2[37] == (4101, 0))
        sets += [a, b]
        exps.append(exp)
    _, rounds, cpw = wide_plan(stride, M)
    assert cpw == 4096 and rounds == 3
    pl = [(2 * (m % 2), 2 * (m % 2) + 1) for m in range(M)]
    out, ran = run(engine, sets, pl, stride)
    assert ran["rounds"] == 3 and ran["wide"] == 3 and ran["evals0"] == 12 * 300 * (4097 + 8191) and ran["scans"] == 0
    for m in range(M):
        assert same(out[m], 300, exps[m % 2]), m


# ---- 5: 255 against 256 in the residual matrix -----------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def byte_limit_sets(n1, n2):
    rng = np.random.default_rng(n1)
    a255, b255 = synth.far_descriptors(n1, n2, 255, 255, n1)
    ac, bc = rng.integers(0, 2**32, (n1, 8), dtype=np.uint32), rng.integers(0, 2**32, (n2, 8), dtype=np.uint32)
    bc[7] = ~ac[5]                                                            # ONE exact complement
    ap, bp = rng.integers(0, 2**32, (n1, 8), dtype=np.uint32), rng.integers(0, 2**32, (n2, 8), dtype=np.uint32)
    sets = [a255, b255, ac, bc, ap, bp]
    return sets, [cref.match(sets[2 * m], sets[2 * m + 1]) for m in range(3)]


@gpu
@pytest.mark.parametrize("n1,n2", [(257, 130), (130, 257)])
def test_tail_distance_255_stays_fast_and_256_falls_back_alone(engine, n1, n2):
    """255 is the largest byte of the residual matrix, 256 sets its overflow flag: a pair at 255 everywhere, a pair with one
    exact complement and a plain pair in ONE launch, each against its oracle (the flag of one pair must not reach its
    neighbours, nor its distances theirs); then the 255 pair and the complement pair alone, for the path each takes."""
    sets, exps = byte_limit_sets(n1, n2)
    r255, c255 = nearest(sets[0], sets[1])
    assert r255.min() == r255.max() == c255.min() == c255.max() == 255 and (matched(exps[0])["dist"] == 255).all()
    assert dist_matrix(sets[2], sets[3]).max() == 256 and (dist_matrix(sets[2], sets[3]) == 256).sum() == 1
    assert dist_matrix(sets[4], sets[5]).max() < 255
    stride = max(n1, n2)
    out, ran = run(engine, sets, [(0, 1), (2, 3), (4, 5)], stride)
    assert ran["wide"] == 0 and ran["rows"] == 1 and ran["finish"] == 1 and ran["scans"] > 0
    for m in range(3):
        assert same(out[m], n1, exps[m]), m
    out, ran = run(engine, sets, [(0, 1)], stride)
    assert ran["wide"] == 0 and ran["scans"] > 0 and same(out[0], n1, exps[0])          # fast path
    out, ran = run(engine, sets, [(2, 3)], stride)
    assert ran["wide"] == 0 and ran["scans"] == 0 and ran["pushes"] == 0 and same(out[0], n1, exps[1])   # fallback


# ---- 6: the tail at its size limits -------------------------------------------------------------------------------------
TAIL_SHAPES = [(2048, 2048, "random"), (2048, 1, "random"), (1, 2048, "random"), (2047, 2049, "ties"), (257, 2048, "ties"),
               (2048, 129, "ties"), (33, 513, "random"), (256, 512, "ties"), (255, 511, "random")]


@functools.lru_cache(maxsize=None)
def tail_shape_sets():
    sets, exps = [], []
    for k, (R, C, kind) in enumerate(TAIL_SHAPES):
        if kind == "ties":
            a, b = synth.tiled_ties(R, C, 128 if C > 128 else 32, 600 + k, 32)
        else:
            a, b = synth.random_descriptors(R, 8, 600 + k), synth.random_descriptors(C, 8, 700 + k)
        sets += [a, b]
        exps.append(cref.match_sorted(a, b))
    return sets, exps


@gpu
def test_tail_at_its_size_limits(engine):
    """Residuals that enter k_tail_rows_fp4 / k_match_gs as they are (M >= 3: up to 2048 x 2048 goes straight to the tail) at
    and around 32 (row tile), 256 (rows per workgroup), 128 and 512 (a wavefront's and a workgroup's column stride) and 2048
    (PGX_TAIL_MAX, the ring, the lanes' dwords of a matrix row); 2047 x 2049 takes wide rounds first, alone."""
    sets, exps = tail_shape_sets()
    for (R, C, kind), exp in zip(TAIL_SHAPES, exps):
        assert len(matched(exp)) == min(R, C)
        assert kind != "ties" or (matched(exp)["dist"] <= 2).mean() > 0.5
    M, stride = len(TAIL_SHAPES), 2176
    skip, rounds, _ = wide_plan(stride, M)
    assert skip == TAIL_MAX and rounds == 2
    out, ran = run(engine, sets, [(2 * m, 2 * m + 1) for m in range(M)], stride)
    assert ran["wide"] == 2 and ran["evals0"] == 2047 * 2049           # every other pair skipped the wide rounds
    assert ran["rows"] == 1 and ran["finish"] == 1 and ran["scans"] > 0
    for m, (R, C, kind) in enumerate(TAIL_SHAPES):
        assert same(out[m], R, exps[m]), (R, C)


# ---- 7: the ring of free rows laps ---------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def ring_sets():
    rng = np.random.default_rng(77)
    protos = rng.integers(0, 2**32, (4, 8), dtype=np.uint32)
    a = synth.flip_bits(rng, protos[rng.integers(0, 4, 2048)], rng.integers(0, 2, 2048))
    b = synth.flip_bits(rng, protos[rng.integers(0, 4, 2048)], rng.integers(0, 3, 2048))
    one = protos[:1]
    return [a, b, one], cref.match_sorted(a, b)


@gpu
def test_tail_ring_laps(engine):
    """2048 x 2048 of four prototypes with 0..2 bits flipped, straight into the tail (M = 3; the two other pairs are 1 x 1 and
    push at most one row each): more than GS_QN = 2048 pushes in one pair, so ring slots are reused while rows are in flight."""
    sets, exp = ring_sets()
    m = matched(exp)
    assert len(m) == 2048 and (m["dist"] <= 3).mean() > 0.5                                # tie-heavy: a few prototypes, distances 0..3
    out, ran = run(engine, sets, [(0, 1), (2, 2), (2, 2)], 2048)
    assert ran["wide"] == 0 and ran["rows"] == 1 and ran["scans"] > 0
    assert ran["pushes"] > GS_QN + 2, ran
    engine.check_status()                                               # no PGX_ST_INTERNAL: no guard of the queue tripped
    assert same(out[0], 2048, exp)
    assert out[1][0].tolist() == [0, 0, 0] and out[2][0].tolist() == [0, 0, 0]


# ---- 8: the finish's launch forms and its emit paths ----------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def emit_sets():
    """200 x 150 and 150 x 200 (N1 > N2: a (0, 0, int.MaxValue) tail), 4096 x 2100 (emit of 4096 rows, 1996 of them the tail)
    and 4097 x 2100 (one row more than count_and_emit takes: the sort).  The 2100 columns are noisy copies of 2100 of the
    rows, so the wide rounds match nearly every column."""
    rng = np.random.default_rng(8)
    a, b = synth.random_descriptors(200, 8, 81), synth.random_descriptors(150, 8, 82)
    big = synth.random_descriptors(4097, 8, 83)
    cols = synth.flip_bits(rng, big[rng.permutation(4096)[:2100]], rng.integers(0, 20, 2100))
    cols[-1] = synth.flip_bits(rng, big[4096:], 3)[0]                       # row 4096 has a partner
    sets = [a, b, big[:4096], cols, big]
    pairs = [(0, 1), (1, 0), (2, 3), (4, 3)]
    exps = [cref.match(a, b), cref.match(b, a), cref.match_sorted(big[:4096], cols), cref.match_sorted(big, cols)]
    return sets, pairs, exps


@gpu
@pytest.mark.parametrize("M", [512, 511])
def test_finish_launch_forms_and_emit(engine, M):
    """512 pairs: k_match_gs with 512 threads (eight emit sub-rounds at 4096 rows); 511: 1024 threads.  Four pairs alternate:
    lists with and without the (0, 0, int.MaxValue) tail, n1 = 4096 (1996 tail entries, across multiples of 64 and of the
    thread count) and n1 = 4097 (beyond count_and_emit: the bitonic sort of 8192 keys)."""
    sets, pairs, exps = emit_sets()
    assert (exps[0]["dist"][150:] == 2**31 - 1).all() and len(matched(exps[1])) == 150
    assert len(matched(exps[2])) == 2100 and (exps[2]["dist"][2100:] == 2**31 - 1).all() and len(exps[2]) == EM_MAXROWS
    assert len(matched(exps[3])) == 2100 and len(exps[3]) == EM_MAXROWS + 1 and 4096 in matched(exps[3])["k1"]
    stride = 4224
    rounds = wide_plan(stride, M)[1]
    pl = [pairs[m % 4] for m in range(M)]
    out, ran = run(engine, sets, pl, stride)
    # ONE finish launch: all M pairs are one chunk, and pgx_launch_match_finish gives a chunk of GS_SMALL_FROM = 512 pairs or
    # more 512 threads, a smaller one 1024 -- the library reports no thread count, so this launch count is what pins the form
    assert ran["rounds"] == rounds == 3 and ran["wide"] == 3 and ran["finish"] == 1
    assert ran["evals0"] == sum(len(sets[a]) * len(sets[b]) for a, b in pl if len(sets[a]) > TAIL_MAX)
    for m in range(M):
        assert same(out[m], len(sets[pl[m][0]]), exps[m % 4]), m


# ---- 9: the shared fp4 arithmetic in k_knn.hip ---------------------------------------------------------------------------
@gpu
def test_knn_nearest_beyond_128(engine):
    """pgx_fp4.h is shared with the exact nearest-neighbour kernel: 300 rows against 5000 columns (more than one chunk) whose
    two nearest columns, and every column's nearest row, are all further than 128.  k_knn has no counters: that 5000 columns
    are more than one of its passes over F4_CHUNK = 4096 columns follows from the constant alone."""
    from match_gpu import run_knn, upload
    a, b = synth.far_descriptors(300, 5000, 150, 200, 9)
    r_idx, r_dist, r_col = ref_knn(a, b)
    rmin, cmin = nearest(a, b)
    assert r_dist.min() >= 129 and cmin.min() >= 129 and (r_dist[:, 0] == rmin).all()
    idx, dist, col = run_knn(engine, upload(5000, 8, [a, b]), 5000, 8, [(0, 1), (1, 0)], 2, True)
    assert (idx[0, :300] == r_idx).all() and (dist[0, :300] == r_dist).all() and (col[0, :5000] == r_col).all()
    assert (idx[0, 300:] == 77).all() and (dist[0, 300:] == 77).all()
    t_idx, t_dist, t_col = ref_knn(b, a)
    assert t_dist.min() >= 129
    assert (idx[1] == t_idx).all() and (dist[1] == t_dist).all() and (col[1, :300] == t_col).all() and (col[1, 300:] == 77).all()


# ---- the generators, without a GPU ---------------------------------------------------------------------------------------
def test_far_descriptors_keep_their_range():
    for n1, n2 in [(1100, 1060), (1060, 1100), (300, 5000)]:
        a, b = synth.far_descriptors(n1, n2, 150, 200, 1000 + n1)
        assert a.shape == (n1, 8) and b.shape == (n2, 8) and a.dtype == b.dtype == np.uint32
        rmin, cmin = nearest(a, b)
        assert 150 <= rmin.min() and rmin.max() <= 200 and 150 <= cmin.min() and cmin.max() <= 200
    exp = far_pair(1100, 1060, 150, 200)[2]
    assert matched(exp)["dist"].min() >= 150 and len(matched(exp)) == 1060
    for exact in (255, 256):
        a, b = synth.far_descriptors(70, 50, exact, exact, 5)
        assert (dist_matrix(a, b) == exact).all()
        exp = cref.match(a, b)                    # every distance ties: (k1, k2) ascending alone decides
        assert (exp["k1"][:50] == np.arange(50)).all() and (exp["k2"][:50] == np.arange(50)).all()
        assert (exp["dist"][:50] == exact).all() and (exp["dist"][50:] == 2**31 - 1).all()
    assert (synth.far_descriptors(40, 40, 150, 200, 3)[1] == synth.far_descriptors(40, 40, 150, 200, 3)[1]).all()   # seeded


@pytest.mark.parametrize("n1,n2,period,row_period", [(300, 600, 32, 96), (500, 700, 128, 32), (400, 4100, 4064, 384)])
def test_tiled_ties_tie_where_they_say(n1, n2, period, row_period):
    a, b = synth.tiled_ties(n1, n2, period, 1, row_period)
    j = np.arange(n2 - period)
    j = j[(j // period) % 2 == 0]
    assert (b[j + period] == b[j]).all()
    i = np.arange(n1 - row_period)
    i = i[(i // row_period) % 2 == 0]
    assert (a[i + row_period] == a[i]).all()
    idx, dist, col = ref_knn(a, b)
    tied = dist[:, 0] == dist[:, 1]
    assert dist[:, 0].max() <= 2 and tied.any() and (idx[tied, 1] - idx[tied, 0] == period).all()
    assert len(np.unique(b, axis=0)) >= n2 // 2                        # half of the columns stay distinct
    exp = cref.match_sorted(a, b)
    assert ties_resolved_both_ways(exp, period) and (matched(exp)["dist"] <= 2).mean() > 0.4
    assert (cref.match_sorted(a[:60], b[:90])["k2"] == cref.match(a[:60], b[:90])["k2"]).all()


def test_wide_plan_thresholds():
    """the (stride, M) -> path arithmetic the GPU cases rely on.  wide_plan is a hand copy of the host code: its round count is
    held to pgx_match_stats in every GPU case, its column chunk to nothing the library reports -- a change of that heuristic in
    pgx_launch_ham_mfma has to be made here and in DESIGN.md section 4 as well"""
    assert wide_plan(1024, 1)[:2] == (1024, 0) and wide_plan(1025, 2)[:2] == (1024, 2) and wide_plan(2048, 3)[:2] == (2048, 0)
    assert wide_plan(2049, 3)[:2] == (2048, 2) and wide_plan(8192, 24) == (2048, 3, 4096)
    assert [wide_plan(4096, M)[2] for M in (94, 93, 47, 46)] == [4096, 2048, 2048, 1024]
    assert [wide_plan(2176, M)[2] for M in (171, 170, 86, 85, 57, 56, 35, 34, 19, 18, 3)] == \
        [4096, 2048, 2048, 1024, 1024, 512, 512, 256, 256, 128, 128]
