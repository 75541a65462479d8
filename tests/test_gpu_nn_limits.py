"""The exact nearest-neighbour matcher (k_knn_fp4, k_knn_rows_valu / k_knn_cols_valu), the epipolar-guided matcher
(k_guided_slots -> k_guided_bucket -> k_guided_walk) and the selection they share (k_knn_select, pgx_pairlist.h) past the limits
of their blockings and key fields: column counts on both sides of a tile (32) and of a chunk (4096), row counts on both sides
of the 128- and 256-row blocks with the padded duplicates of the last row, ties laid exactly across a tile, a chunk, a wave
and a workgroup, distances 0 and 256 (the two ends of the biased accumulator's binade), distance 4064 at 127 words, the index
2^20 - 1, counts above max_count and below 0, the guided grid at its cell cap and at one cell, degenerate boxes, vertical,
diagonal and missing lines, band 0, the whole coordinate range, colliding and wrapping frame-table probes, the ratio rule
where float32 would give the other answer, the max_dist edge and the cross-check on tied rows.

Every value is an exact integer, so every comparison is == against tests/knn_ref.py and tests/guided_ref.py: idx, dist, col,
the NN lists, and the sentinel behind every list.  The inputs are made once by cached builders that FIRST assert, on the
reference's result, the property the case is built for; the builders run without a GPU at the end of the file, so an input
that has drifted fails there and no GPU case passes vacuously.  The kernels report no path counters: which blocking an input
reaches follows from the constants mirrored below.
"""
import functools

import numpy as np
import pytest

from guided_ref import admissible, ref_guided
from knn_ref import NONE, dist_matrix, ref_knn, ref_select
from photogrammetry_amd import synth

gpu = pytest.mark.gpu
SENT = 77
FORMS = [(1, False), (1, True), (2, False), (2, True)]   # (k, column side): the four instantiations of both producers

# constants of the kernels, mirrored once
F4_CHUNK = 4096                  # pgx_fp4.h: columns per pass of k_knn_fp4 (KNN_CHUNK); a tile is 32 columns
ROWS_RT1, ROWS_RT2 = 128, 256    # k_knn.hip launch_fp4: rows per workgroup of the K == 2 && !COL form / of the other forms
IDX_BITS = 20                    # pgx_internal.h PGX_IDX_BITS: (distance << 20 | index) keys, PGX_KEY_NONE = 0xFFFFFFFF
GUIDED_MAX_CELLS = 8192          # k_guided.hip: LDS counters of the bucketing pass
COORD_LIM = 1 << 20              # k_guided.hip: used coordinates lie in [-2^20, 2^20)
BIG = 1 << IDX_BITS


def table_size(E):
    """k_guided.hip table_size: the smallest power of two >= max(16, 2 E)"""
    H = 16
    while H < 2 * E:
        H <<= 1
    return H


def table_home(f, H):
    """k_guided_slots: the first probe of frame f"""
    return ((f * 2654435761) & 0xFFFFFFFF) & (H - 1)


def table_occupied(frames, H):
    """the positions linear probing fills for the distinct frames (the set does not depend on the insertion order)"""
    used = set()
    for f in dict.fromkeys(frames):
        h = table_home(f, H)
        while h in used:
            h = (h + 1) & (H - 1)
        used.add(h)
    return used


def grid_plan(kp, max_n):
    """k_guided_bucket's cell choice for keypoints kp [n][2] under cells_cap(max_n) -> (shift, gx, gy)"""
    n = len(kp)
    cap = min(max(max_n // 2, 1), GUIDED_MAX_CELLS)
    target = min(max(1, n // 2), cap)
    w, h = (int(kp[:, 0].max() - kp[:, 0].min()), int(kp[:, 1].max() - kp[:, 1].min())) if n else (0, 0)
    for sh in range(22):
        gx, gy = (w >> sh) + 1, (h >> sh) + 1
        if gx * gy <= target:
            break
    return sh, gx, gy


def last_tile_first_col(n2):
    """the first column of the last 32-column tile of the last chunk of n2 columns"""
    cb = (n2 - 1) // F4_CHUNK * F4_CHUNK
    return cb + (n2 - cb - 1) // 32 * 32


def rnd(rng, n, words):
    return rng.integers(0, 2**32, size=(n, words), dtype=np.uint32)


def pts(rng, n, W, H, x0=0, y0=0):
    return np.stack([rng.integers(x0, x0 + W, n), rng.integers(y0, y0 + H, n)], 1).astype(np.int32).reshape(n, 2)


def flip1(rng, d, k):
    """one descriptor with k bits flipped"""
    return synth.flip_bits(rng, d[None, :], k)[0]


def ref_wide(a, b, adm=None, block=65536):
    """ref_knn / ref_guided for a FEW rows against very many columns: the distance matrix in column blocks, the two nearest
    by two first-occurrence argmins, the column side by argmin over the rows (its first occurrence: the smallest row)"""
    D = np.concatenate([dist_matrix(a, b[c:c + block]) for c in range(0, len(b), block)], axis=1).astype(np.int64)
    if adm is not None:
        D = np.where(adm, D, np.int64(NONE))
    n1 = len(a)
    idx, dist = np.full((n1, 2), -1, np.int32), np.full((n1, 2), NONE, np.int32)
    W = D.copy()
    for e in range(2):
        j = W.argmin(1)
        d = W[np.arange(n1), j]
        ok = d < NONE
        idx[:, e], dist[:, e] = np.where(ok, j, -1), np.where(ok, d, NONE)
        W[np.arange(n1), j] = np.int64(NONE) + 1
    mn, am = D.min(0), D.argmin(0)
    return idx, dist, np.where(mn < NONE, am, -1).astype(np.int32)


def same(got, exp, what):
    if got.shape != exp.shape or not (got == exp).all():
        bad = np.argwhere(got != exp)[:4] if got.shape == exp.shape else []
        raise AssertionError("%s: shapes %s / %s, %d entries differ; first %s" % (
            what, got.shape, exp.shape, len(np.argwhere(got != exp)) if got.shape == exp.shape else -1,
            [(tuple(int(v) for v in q), int(got[tuple(q)]), int(exp[tuple(q)])) for q in bad]))


def check(engine, dev, stride, words, pl, refs, forms=FORMS, guide=None, max_count=None, tag=""):
    """every form of one batch against refs[m] = (idx [n1][2], dist [n1][2], col [n2]); what lies behind a list is untouched"""
    from match_gpu import run_knn
    got = None
    for k, col in forms:
        got = run_knn(engine, dev, stride, words, pl, k, col, sentinel=SENT, max_count=max_count, guide=guide)
        idx, dist, cnn = got
        for m, (r_idx, r_dist, r_col) in enumerate(refs):
            n1, n2, w = len(r_idx), len(r_col), "%s pair %d %s k=%d col=%d " % (tag, m, pl[m], k, col)
            same(idx[m, :n1], r_idx[:, :k], w + "idx")
            same(dist[m, :n1], r_dist[:, :k], w + "dist")
            assert (idx[m, n1:] == SENT).all() and (dist[m, n1:] == SENT).all(), w + "rows behind the list written"
            if col:
                same(cnn[m, :n2], r_col, w + "col")
                assert (cnn[m, n2:] == SENT).all(), w + "columns behind the list written"
    return got


def check_nn(engine, dev, stride, words, pl, refs, max_dist, ratio, cross, guide=None, max_count=None, tag=""):
    from match_gpu import run_nn
    out = run_nn(engine, dev, stride, words, pl, max_dist, ratio, cross, sentinel=SENT, guide=guide, max_count=max_count)
    for m, r in enumerate(refs):
        exp = ref_select(*r, max_dist, ratio, cross)
        w = "%s pair %d %s max_dist=%d ratio=%g cross=%d" % (tag, m, pl[m], max_dist, ratio, cross)
        same(out[m, :len(exp)], exp, w)
        assert (out[m, len(exp):] == SENT).all(), w + ": rows behind the list written"
    return out


def both_orders(n):
    """pairs (0, q), (q, 0) for q = 1 .. n"""
    return [p for q in range(1, n + 1) for p in ((0, q), (q, 0))]


# ==== A. k_knn_fp4 blockings ===================================================================================================
N2S = (31, 32, 33, 4095, 4096, 4097, 4128, 8192, 8193)
N1S = (1, 127, 128, 129, 255, 256, 257)


@functools.lru_cache(maxsize=None)
def column_edge_sets(words):
    """70 rows against the first n2 of 8193 columns, n2 on both sides of a tile and of one and two chunks (4097: a second
    chunk of ONE column, ntile == 1, every look-ahead fetch clamped).  Rows 3q + 1 are copies, with 0 .. 2 bits flipped, of the
    last column of every n2, of the first column of its last tile and of columns 4095 / 4096."""
    rng = np.random.default_rng(100 + words)
    b, a = rnd(rng, N2S[-1], words), rnd(rng, 70, words)
    plant = sorted({n2 - 1 for n2 in N2S} | {last_tile_first_col(n2) for n2 in N2S} | {4095, 4096})
    assert plant == [0, 30, 31, 32, 4064, 4094, 4095, 4096, 4127, 8160, 8191, 8192]
    row_of = {}
    for q, j in enumerate(plant):
        a[3 * q + 1] = flip1(rng, b[j], q % 3)
        row_of[j] = 3 * q + 1
    descs, pl, refs = [a], [], []
    for q, n2 in enumerate(N2S):
        descs.append(b[:n2])
        fwd, rev = ref_knn(a, b[:n2]), ref_knn(b[:n2], a)
        # some row's nearest column is the last one, and that column's nearest row is the planted row -- in both orders
        assert fwd[0][row_of[n2 - 1], 0] == n2 - 1 and fwd[1][row_of[n2 - 1], 0] <= 2 and fwd[2][n2 - 1] == row_of[n2 - 1]
        assert rev[0][n2 - 1, 0] == row_of[n2 - 1] and rev[2][row_of[n2 - 1]] == n2 - 1
        j0 = last_tile_first_col(n2)
        assert fwd[0][row_of[j0], 0] == j0 and fwd[2][j0] == row_of[j0]
        pl += [(0, q + 1), (q + 1, 0)]
        refs += [fwd, rev]
    return descs, pl, refs


@functools.lru_cache(maxsize=None)
def row_edge_sets(words):
    """n1 rows on both sides of the 128- and 256-row blocks against 200 columns.  Columns 10 and 11 are equal and equal row
    n1 - 1 -- the row whose duplicates pad the block -- and column 20 is row 128 with one bit flipped where that row exists
    and is not the last."""
    rng = np.random.default_rng(200 + words)
    b = rnd(rng, 200, words)
    b[11] = b[10]
    descs, pl, refs = [b], [], []
    for q, n1 in enumerate(N1S):
        a = rnd(rng, n1, words)
        a[n1 - 1] = b[10]
        if n1 - 1 > 128:
            a[128] = flip1(rng, b[20], 1)
        descs.append(a)
        fwd, rev = ref_knn(a, b), ref_knn(b, a)
        assert fwd[2][10] == fwd[2][11] == n1 - 1 and list(fwd[0][n1 - 1]) == [10, 11] and list(fwd[1][n1 - 1]) == [0, 0]
        assert rev[0][10, 0] == rev[0][11, 0] == n1 - 1 and rev[2][n1 - 1] == 10      # the smaller of the two tied rows
        assert n1 - 1 <= 128 or (fwd[2][20] == 128 and rev[0][20, 0] == 128)
        pl += [(q + 1, 0), (0, q + 1)]
        refs += [fwd, rev]
    return descs, pl, refs


ROW_TIES = [(5, 0, (31, 32)), (6, 0, (17, 4095)), (7, 0, (4096, 8191)), (8, 1, (4095, 4096)), (6, 2, (17, 4095))]
COL_TIES = [(31, 32), (63, 64), (127, 128), (255, 256)]   # tile, wave (RT = 2), RT = 1 block, workgroup (the global atomicMin)


@functools.lru_cache(maxsize=None)
def boundary_tie_sets():
    """300 rows against three sets of 8200 columns.  Row side (ROW_TIES: row, column set, expected top-2 at (0, 0)): equal
    columns in neighbouring tiles, in the first and the last tile of a chunk, on both sides of the chunk border, and in two
    chunks; in set 2 columns 17, 4095 and 4096 are all equal, and the third must lose.  Column side (COL_TIES): equal rows on
    both sides of a tile, a wave, a 128-row block and a 256-row block, each pair the nearest of column 1000 + q."""
    rng = np.random.default_rng(300)
    base, a = rnd(rng, 8200, 8), rnd(rng, 300, 8)
    b0, b1, b2 = base.copy(), base.copy(), base.copy()
    b0[32], b0[4095], b0[8191] = base[31], base[17], base[4096]
    b1[4096] = base[4095]
    b2[4095] = b2[4096] = base[17]
    a[5], a[6], a[7], a[8] = base[31], base[17], base[4096], base[4095]
    for q, (i, i2) in enumerate(COL_TIES):
        a[i] = a[i2] = flip1(rng, base[1000 + q], 1)
    sets = [b0, b1, b2]
    refs = [ref_knn(a, b) for b in sets]
    for row, s, top in ROW_TIES:
        assert list(refs[s][0][row]) == list(top) and list(refs[s][1][row]) == [0, 0], (row, s)
    assert dist_matrix(a[6:7], b2)[0, 4096] == 0                                    # a third column at 0, and it is not listed
    for r in refs:
        for q, (i, i2) in enumerate(COL_TIES):
            assert r[2][1000 + q] == i and (a[i] == a[i2]).all() and (r[0][i] == r[0][i2]).all()
    return [a] + sets, [(0, 1), (0, 2), (0, 3)], refs


@functools.lru_cache(maxsize=None)
def distance_end_sets():
    """70 x 4097 (a second chunk of one column) with every distance 256, every distance 255, every distance 0, and a mixed
    set: identical rows, column 4096 equal to them (0), column 4095 one bit away (1), every other column at 255 or 256."""
    rng = np.random.default_rng(400)
    descs = []
    for e in (256, 255, 0):
        a, b = synth.far_descriptors(70, 4097, e, e, 5)
        assert (dist_matrix(a, b) == e).all()
        descs += [a, b]
    P = rnd(rng, 1, 8)
    b = synth.flip_bits(rng, ~np.repeat(P, 4097, axis=0), rng.integers(0, 2, 4097))
    b[4096], b[4095] = P[0], flip1(rng, P[0], 1)
    a = np.repeat(P, 70, axis=0)
    D = dist_matrix(a, b)
    assert (D[:, 4096] == 0).all() and (D[:, 4095] == 1).all() and set(np.unique(D[:, :4095])) == {255, 256}
    descs += [a, b]
    pl = [p for q in range(4) for p in ((2 * q, 2 * q + 1), (2 * q + 1, 2 * q))]
    refs = [ref_knn(descs[x], descs[y]) for x, y in pl]
    for q in range(3):      # every distance ties: the index order alone decides
        assert list(refs[2 * q][0][69]) == [0, 1] and (refs[2 * q][2] == 0).all() and (refs[2 * q + 1][0][:, 0] == 0).all()
    assert list(refs[6][0][0]) == [4096, 4095] and list(refs[6][1][69]) == [0, 1]
    return descs, pl, refs


@functools.lru_cache(maxsize=None)
def big_sets():
    """Frame 0: 2^20 descriptors (the last index the 20-bit fields hold is in use); frame 1: three.  small[0] equals
    big[2^20 - 1] and big[0] is one bit from it, so row 0 of pair (1, 0) has (2^20 - 1, 0) at (0, 1) as its top-2, and
    column 0 of pair (0, 1) has row 2^20 - 1 as its nearest.  Keypoints spread over a 4000 x 3000 window (with duplicates)
    for the guided runs."""
    rng = np.random.default_rng(500)
    big, small = rnd(rng, BIG, 8), rnd(rng, 3, 8)
    small[0] = big[BIG - 1]
    big[0] = flip1(rng, small[0], 1)
    small[1] = flip1(rng, big[BIG - 1], 2)
    small[2] = flip1(rng, big[100 * F4_CHUNK + 5], 3)
    kps = [pts(rng, BIG, 4000, 3000, -700, -500), np.array([[3, 2], [1500, 900], [-600, 2400]], np.int32)]
    refs = [ref_knn(big, small, block=4096), ref_wide(small, big)]
    assert list(refs[1][0][0]) == [BIG - 1, 0] and list(refs[1][1][0]) == [0, 1]
    assert refs[0][2][0] == BIG - 1 and refs[0][0][BIG - 1, 0] == 0 and refs[1][2][BIG - 1] == 0
    assert refs[1][0][2, 0] == 100 * F4_CHUNK + 5
    return [big, small], kps, [(0, 1), (1, 0)], refs


@functools.lru_cache(maxsize=None)
def big_guided(band):
    descs, kps, pl, _ = big_sets()
    rng = np.random.default_rng(501)
    Fr = rng.normal(size=9).astype(np.float32)
    Fs = [Fr, Fr.reshape(3, 3).T.copy().reshape(9)]
    adm_rev = admissible(kps[1], kps[0], Fs[1], band)
    refs = [ref_guided(descs[0], descs[1], kps[0], kps[1], Fs[0], band, block=4096), ref_wide(descs[1], descs[0], adm_rev)]
    return Fs, refs, int(adm_rev.sum())


@pytest.fixture(scope="module")
def big_dev():
    """one upload (about 100 MB) for the two cases of the 20-bit index"""
    from match_gpu import upload
    descs, kps, _, _ = big_sets()
    dev = upload(BIG, 8, descs, kps)
    yield dev
    del dev


@gpu
@pytest.mark.parametrize("words", [8, 3])
def test_knn_column_edges(engine, words):
    from match_gpu import upload
    descs, pl, refs = column_edge_sets(words)
    check(engine, upload(N2S[-1], words, descs), N2S[-1], words, pl, refs, tag="A1")


@gpu
@pytest.mark.parametrize("words", [8, 3])
def test_knn_row_edges_and_padded_last_row(engine, words):
    from match_gpu import upload
    descs, pl, refs = row_edge_sets(words)
    check(engine, upload(264, words, descs), 264, words, pl, refs, tag="A2")


@gpu
def test_knn_ties_on_every_boundary(engine):
    from match_gpu import upload
    descs, pl, refs = boundary_tie_sets()
    check(engine, upload(8200, 8, descs), 8200, 8, pl, refs, tag="A3")


@gpu
def test_knn_ends_of_the_distance_range(engine):
    from match_gpu import upload
    descs, pl, refs = distance_end_sets()
    check(engine, upload(4097, 8, descs), 4097, 8, pl, refs, tag="A4")


@gpu
def test_knn_last_index_of_the_20_bit_field(engine, big_dev):
    _, _, pl, refs = big_sets()
    check(engine, big_dev, BIG, 8, pl, refs, forms=[(2, True)], tag="A5")


# ==== B. k_guided_*: grid, walk and table ======================================================================================
F_AXIS = np.array([0, 0, 0, 0, 0, -1, 0, 1, 0], np.float32)       # l = (0, 1, -y): the line v = y
F_VERT = np.array([0, 0, -1, 0, 0, 0, 1, 0, 0], np.float32)       # f6 = 1, f2 = -1: l = (1, 0, -x), the line u = x
F_ANTI = np.array([0, 0, -1, 0, 0, -1, 1, 1, 0], np.float32)      # l = (1, 1, -x - y): u + v = x + y
F_DIAG = np.array([0, 0, -1, 0, 0, 1, 1, -1, 0], np.float32)      # l = (1, -1, -x + y): u - v = x - y


def transposed(F):
    return np.ascontiguousarray(np.asarray(F, np.float32).reshape(3, 3).T).reshape(9)


def guided_refs(frames, pl, Fs, band, cut=None):
    """ref_guided of every pair; cut: every frame is sliced to its first `cut` entries"""
    out = []
    for (a, b), F in zip(pl, Fs):
        (da, ka), (db, kb) = frames[a], frames[b]
        out.append(ref_guided(da[:cut], db[:cut], ka[:cut], kb[:cut], F, band))
    return out


def n_found(refs):
    return sum(int((r[0][:, 0] >= 0).sum()) for r in refs)


@functools.lru_cache(maxsize=None)
def cell_cap_sets(words):
    """64 rows against the first 16384, 16383 and 20000 of 20000 keypoints in a 2048 x 1024 box with both corners in use:
    8192 cells of 16 pixels (the cap, and 128 x 64 of them exactly), 2048 cells, and 8192 cells again at 2.4 keypoints a cell"""
    rng = np.random.default_rng(600 + words)
    kb = pts(rng, 20000, 2048, 1024)
    kb[0], kb[1] = (0, 0), (2047, 1023)
    db = rnd(rng, 20000, words)
    frames = [(rnd(rng, 64, words), pts(rng, 64, 2048, 1024))] + [(db[:n], kb[:n]) for n in (16384, 16383, 20000)]
    assert [grid_plan(f[1], 20000) for f in frames[1:]] == [(4, 128, 64), (5, 64, 32), (4, 128, 64)]
    assert 128 * 64 == GUIDED_MAX_CELLS
    assert [grid_plan(f[1][:mc], mc)[1:] for f in frames for mc in (1, 2, 3)] == [(1, 1)] * 12   # cells_cap(1 .. 3) == 1
    Fr = rng.normal(size=9).astype(np.float32)
    pl = both_orders(3)
    Fs = [Fr if a == 0 else transposed(Fr) for a, b in pl]
    refs = guided_refs(frames, pl, Fs, 3.0)
    assert n_found(refs) > 300
    return frames, pl, Fs, refs, {mc: guided_refs(frames, pl, Fs, 3.0, cut=mc) for mc in (1, 2, 3)}


@functools.lru_cache(maxsize=None)
def degenerate_box_sets(words):
    """Frames whose box is a vertical line, a horizontal line, one point (1000 keypoints), one keypoint, and two keypoints at
    opposite corners of the coordinate range (one cell of 2^21 pixels), each as frame a and as frame b of a spread frame,
    under horizontal, vertical, diagonal and random lines"""
    rng = np.random.default_rng(700 + words)
    spread = pts(rng, 500, 2000, 1500)
    spread[0], spread[1], spread[2], spread[3] = (700, 40), (40, 900), (702, 333), (500, 500)
    lim = COORD_LIM
    boxes = [np.stack([np.full(300, 700), rng.integers(0, 1500, 300)], 1), np.stack([rng.integers(0, 2000, 300), np.full(300, 900)], 1),
             np.tile([[700, 900]], (1000, 1)), np.array([[700, 900]]), np.array([[-lim, -lim], [lim - 1, lim - 1]])]
    frames = [(rnd(rng, len(k), words), np.asarray(k, np.int32).reshape(-1, 2)) for k in [spread] + boxes]
    plans = [grid_plan(f[1], 1000)[1:] for f in frames[1:]]      # a single column of cells, a single row of cells, one cell
    assert plans[0][0] == 1 < plans[0][1] and plans[1][1] == 1 < plans[1][0] and plans[2:] == [(1, 1)] * 3
    assert grid_plan(frames[5][1], 1000)[0] == 21
    Fr = rng.normal(size=9).astype(np.float32)
    pl, Fs = [], []
    for q in range(1, 6):
        for F in (F_AXIS, F_VERT, F_DIAG, Fr):
            pl += [(0, q), (q, 0)]
            Fs += [F, F]
    refs = guided_refs(frames, pl, Fs, 5.0)
    found = [int((r[0][:, 0] >= 0).sum()) for r in refs]
    for q in range(5):      # every degenerate frame is reached from the spread frame, and reaches it, under some line
        assert max(found[8 * q:8 * q + 8:2]) > 0 and max(found[8 * q + 1:8 * q + 8:2]) > 0, q
    assert found[8 * 4 + 4] >= 1 and sorted(refs[8 * 4 + 4][0][3].tolist()) == [0, 1]    # row (500, 500) sees both corners on u - v = 0
    assert found[8 * 4 + 5] == 2                                                 # and both corners see the spread frame
    return frames, pl, Fs, refs


LINE_FS = [F_VERT, F_ANTI, F_DIAG,
           np.array([0, 0, 0, 0, 0, 0, 0, 1, -5000], np.float32),      # (iv) v = 5000: misses the box by more than the band
           np.array([0, 0, 0, 0, 0, 0, 1, 1, 0], np.float32),          # (v) u + v = 0: through the corner (0, 0) only
           np.array([0, 0, 0, 0, 0, 0, 1, -1, -1200], np.float32)]     # (v) u - v = 1200: through the corner (1200, 0) only


@functools.lru_cache(maxsize=None)
def line_sets(words):
    """40 rows; frame b holds, per row (x, y), two keypoints on each of u = x, u + v = x + y and u - v = x - y, the
    horizontal neighbours of those on u = x, and 100 keypoints anywhere, in a box with corners (0, 0) and (1200, 0)"""
    rng = np.random.default_rng(800 + words)
    ka = pts(rng, 40, 600, 600, 200, 200)
    kb = [(0, 0), (1200, 0)]
    for x, y in ka.tolist():
        for t in rng.choice(np.r_[-150:-1, 2:151], 2, replace=False).tolist():
            kb += [(x, y + t), (x - 1, y + t), (x + 1, y + t), (x + t, y - t), (x + t, y + t)]
    kb = np.concatenate([np.array(kb, np.int32), pts(rng, 100, 1000, 1000, 50, 50)])
    assert kb[2:, 0].min() >= 1 and kb[2:, 0].max() <= 1199 and kb[2:, 1].min() >= 1
    frames = [(rnd(rng, 40, words), ka), (rnd(rng, len(kb), words), kb)]
    x, y, u, v = ka[:, :1].astype(np.int64), ka[:, 1:].astype(np.int64), kb[None, :, 0].astype(np.int64), kb[None, :, 1].astype(np.int64)
    on = [u == x, u + v == x + y, u - v == x - y, np.zeros((40, len(kb)), bool),
          np.broadcast_to((u == 0) & (v == 0), (40, len(kb))), np.broadcast_to((u == 1200) & (v == 0), (40, len(kb)))]
    for F, mask in zip(LINE_FS, on):     # band 0 admits the keypoints exactly on the line and no other
        assert (admissible(ka, kb, F, 0.0) == mask).all()
    assert all(on[q].sum(1).min() >= 2 for q in range(3)) and on[4].sum() == 40 == on[5].sum()
    assert (admissible(ka, kb, F_VERT, 1.0) == (np.abs(u - x) <= 1)).all() and (np.abs(u - x) == 1).sum(1).min() >= 4
    pl = [(0, 1)] * 6 + [(1, 0)] * 3
    Fs = LINE_FS + [transposed(F) for F in LINE_FS[:3]]
    refs = {band: guided_refs(frames, pl, Fs, band) for band in (0.0, 1.0)}
    for q in range(3):
        assert (refs[0.0][q][0] >= 0).all() and (admissible(kb, ka, Fs[6 + q], 0.0) == on[q].T).all()
    assert n_found(refs[0.0][3:4]) == 0 and (refs[0.0][4][0][:, 0] == 0).all() and (refs[0.0][5][0] == [1, -1]).all()
    return frames, pl, Fs, refs


@functools.lru_cache(maxsize=None)
def full_range_sets(words):
    """2000 keypoints over the whole of [-2^20, 2^20)^2, corners included, in two frames, and a third frame confined to the
    2000 x 2000 pixels at the lowest corner: a box far from the origin, large line offsets"""
    lim = COORD_LIM
    corners = np.array([[-lim, -lim], [-lim, lim - 1], [lim - 1, -lim], [lim - 1, lim - 1]], np.int32)
    for seed in range(900 + words, 940 + words):
        rng = np.random.default_rng(seed)
        ka, kb = pts(rng, 2000, 2 * lim, 2 * lim, -lim, -lim), pts(rng, 2000, 2 * lim, 2 * lim, -lim, -lim)
        ka[:4], kb[:4] = corners, corners[::-1]
        kc = pts(rng, 2000, 2000, 2000, -lim, -lim)
        kc[0] = corners[0]
        Fr = rng.normal(size=9).astype(np.float32)
        n_far = int(admissible(ka, kc, Fr, 3000.0).sum()), int(admissible(kc, ka, transposed(Fr), 3000.0).sum())
        if min(n_far) >= 300:
            break
    frames = [(rnd(rng, 2000, words), k) for k in (ka, kb, kc)]
    pl = both_orders(2)
    Fs = [Fr, transposed(Fr)] * 2
    assert int(admissible(ka, kb, Fr, 3000.0).sum()) >= 300 and min(n_far) >= 300
    assert grid_plan(kb, 2000)[0] >= 15 and grid_plan(kc, 2000)[0] <= 7
    return frames, pl, Fs, guided_refs(frames, pl, Fs, 3000.0)


TABLE_FRAMES = (15, 31, 47, 63, 79, 95, 111)


@functools.lru_cache(maxsize=None)
def table_sets(words):
    """2048 frame slots at stride 64, 23 of them in use.  M = 4: eight entries, seven frames, all on position 15 of a table of
    16, the probe chain wrapping to 0 .. 5.  M = 17 at 16 pairs a chunk: frames f and f + 64 collide in the table of 64, and
    the one pair of the second chunk builds a table of 16 of its own.  M = 40 (80 entries, a table of 256): frames c + 256 k
    collide, one chain of eight starts three positions before the table's end."""
    rng = np.random.default_rng(1000 + words)
    H40 = table_size(2 * 40)
    c_end = next(c for c in range(H40) if table_home(c, H40) == H40 - 3)
    used = list(TABLE_FRAMES) + [c + H40 * k for c in (5, c_end) for k in range(8)]
    frames = [(np.zeros((0, words), np.uint32), np.zeros((0, 2), np.int32))] * (8 * H40)
    for f in used:
        n = int(rng.integers(30, 65))
        frames[f] = (rnd(rng, n, words), pts(rng, n, 300, 200))
    pl4 = [(15, 31), (47, 63), (79, 95), (111, 15)]
    assert 2654435761 % 16 == 1 and table_size(8) == 16 and {table_home(f, 16) for p in pl4 for f in p} == {15}
    assert table_occupied([f for p in pl4 for f in p], 16) == {15, 0, 1, 2, 3, 4, 5}
    pl17 = [(a, b) for a in TABLE_FRAMES for b in TABLE_FRAMES if a != b][:17]
    assert table_size(32) == 64 and table_home(15, 64) == table_home(79, 64) and table_home(47, 64) == table_home(111, 64)
    assert len({f for p in pl17[:16] for f in p}) == 7
    far = used[7:]
    pl40 = [(far[q % 16], far[(5 * q + 3) % 16]) for q in range(40)]
    assert H40 == 256 and len({f for p in pl40 for f in p}) == 16
    occ = table_occupied([f for p in pl40 for f in p], H40)
    assert {table_home(f, H40) for f in far} == {table_home(5, H40), H40 - 3} and len(occ) == 16
    assert {H40 - 1, 0, 4} <= occ                                                   # the chain from H - 3 wraps to 0 .. 4
    out = []
    for pl in (pl4, pl17, pl40):
        Fs = [rng.normal(size=9).astype(np.float32) for _ in pl]
        refs = guided_refs(frames, pl, Fs, 20.0)
        assert n_found(refs) > 5 * len(pl)
        out.append((pl, Fs, refs))
    return frames, out


F_PT = np.array([1, 0, 0, 0, 1, 0, -500, -300, 1], np.float32)      # l = (x - 500, y - 300, 1): no line for the row AT (500, 300)


@functools.lru_cache(maxsize=None)
def wide_key_sets():
    """words = 127.  Per n1 in 255, 256, 257: frame a_n (row 3 at (500, 300), row n1 - 1 at y = 777, row i at y = 1000 + i
    else) and frame b_n of 300 columns: columns 0 and 1 at v = 777, the bit-complement of row n1 - 1 and that with one bit
    flipped back (distances 4064 and 4063); column j at v = 1000 + j else.  Frame c is the complement of row 0, alone."""
    rng = np.random.default_rng(1100)
    base = rnd(rng, 257, 127)
    frames = []
    for n1 in (255, 256, 257):
        da, ka = base[:n1].copy(), pts(rng, n1, 1000, 1)
        ka[:, 1] = 1000 + np.arange(n1)
        ka[3], ka[n1 - 1, 1] = (500, 300), 777
        db, kb = rnd(rng, 300, 127), pts(rng, 300, 1000, 1)
        kb[:, 1] = 1000 + np.arange(300)
        kb[:2, 1] = 777
        db[0] = ~da[n1 - 1]
        db[1] = flip1(rng, db[0], 1)
        frames += [(da, ka), (db, kb)]
    frames.append((~base[:1], np.array([[10, 10]], np.int32)))
    pl1 = [p for q in range(3) for p in ((2 * q, 2 * q + 1), (2 * q + 1, 2 * q), (2 * q, 6), (6, 2 * q))]
    refs1 = guided_refs(frames, pl1, [F_PT] * 12, 1e30)
    pl2 = [p for q in range(3) for p in ((2 * q, 2 * q + 1), (2 * q + 1, 2 * q))]
    refs2 = guided_refs(frames, pl2, [F_AXIS] * 6, 0.0)
    for q, n1 in enumerate((255, 256, 257)):
        r = refs1[4 * q]                       # a huge band: everything but the row without a line
        assert r[0][3].tolist() == [-1, -1] and r[1][3].tolist() == [NONE, NONE] and (np.delete(r[0], 3, 0) >= 0).all()
        assert refs1[4 * q + 2][1][0, 0] == 4064 and refs1[4 * q + 2][0][0].tolist() == [0, -1]
        assert refs1[4 * q + 3][2][0] == 0 and refs1[4 * q + 3][2][3] == 0
        r = refs2[2 * q]                       # band 0 on v = y: row n1 - 1 has exactly two columns, at 4063 and 4064
        assert r[0][n1 - 1].tolist() == [1, 0] and r[1][n1 - 1].tolist() == [4063, 4064]
        assert r[2][0] == r[2][1] == n1 - 1 and r[0][0].tolist() == [-1, -1] and r[0][4].tolist() == [4, -1]
        assert refs2[2 * q + 1][0][0].tolist() == [n1 - 1, -1] and refs2[2 * q + 1][1][0, 0] == 4064
        assert (4064 << IDX_BITS | (n1 - 1)) < 0xFFFFFFFF
    return frames, (pl1, [F_PT] * 12, refs1), (pl2, [F_AXIS] * 6, refs2)


def guided_all_forms(engine, frames, stride, words, batches, max_count=None, tag=""):
    """batches: (pl, Fs, band, refs); one upload"""
    from match_gpu import upload
    dev = upload(stride, words, *zip(*frames))
    for pl, Fs, band, refs in batches:
        check(engine, dev, stride, words, pl, refs, guide=(Fs, band), max_count=max_count, tag="%s band %g" % (tag, band))
    return dev


@gpu
@pytest.mark.parametrize("words", [8, 3])
def test_guided_grid_at_its_cell_cap(engine, words):
    from match_gpu import upload
    frames, pl, Fs, refs, cut = cell_cap_sets(words)
    dev = upload(20000, words, *zip(*frames))
    check(engine, dev, 20000, words, pl, refs, guide=(Fs, 3.0), tag="B1")
    for mc in (1, 2, 3):      # one cell, and nothing behind the first max_count keypoints is seen
        check(engine, dev, 20000, words, pl, cut[mc], guide=(Fs, 3.0), max_count=mc, tag="B1 max_count %d" % mc)


@gpu
@pytest.mark.parametrize("words", [8, 5])
def test_guided_degenerate_boxes(engine, words):
    frames, pl, Fs, refs = degenerate_box_sets(words)
    guided_all_forms(engine, frames, 1000, words, [(pl, Fs, 5.0, refs)], tag="B2")


@gpu
@pytest.mark.parametrize("words", [8, 5])
def test_guided_line_directions_at_band_0_and_1(engine, words):
    frames, pl, Fs, refs = line_sets(words)
    guided_all_forms(engine, frames, len(frames[1][0]), words, [(pl, Fs, band, refs[band]) for band in (0.0, 1.0)], tag="B3")


@gpu
@pytest.mark.parametrize("words", [8, 5])
def test_guided_whole_coordinate_range(engine, words):
    frames, pl, Fs, refs = full_range_sets(words)
    guided_all_forms(engine, frames, 2000, words, [(pl, Fs, 3000.0, refs)], tag="B4")


@gpu
@pytest.mark.parametrize("words", [8, 3])
def test_guided_frame_table_collisions(engine, words):
    from match_gpu import upload
    frames, (b4, b17, b40) = table_sets(words)
    dev = upload(64, words, *zip(*frames))
    check(engine, dev, 64, words, b4[0], b4[2], guide=(b4[1], 20.0), tag="B5 M=4")
    check(engine, dev, 64, words, b40[0], b40[2], guide=(b40[1], 20.0), tag="B5 M=40")
    try:
        engine.set_match_chunk(16)
        check(engine, dev, 64, words, b17[0], b17[2], guide=(b17[1], 20.0), tag="B5 M=17")
        check_nn(engine, dev, 64, words, b17[0], b17[2], 32 * words, 0.0, True, guide=(b17[1], 20.0), tag="B5 M=17")
    finally:
        engine.set_match_chunk(2048)


@gpu
def test_guided_row_blocks_and_widest_keys(engine):
    frames, (pl1, Fs1, refs1), (pl2, Fs2, refs2) = wide_key_sets()
    dev = guided_all_forms(engine, frames, 300, 127, [(pl1, Fs1, 1e30, refs1), (pl2, Fs2, 0.0, refs2)], tag="B6")
    out = check_nn(engine, dev, 300, 127, pl2, refs2, 4064, 1.0, True, guide=(Fs2, 0.0), tag="B6")
    assert out[0, 254].tolist() == [254, 1, 4063]


@gpu
def test_guided_last_index_of_the_20_bit_field(engine, big_dev):
    from match_gpu import run_knn
    _, _, pl, refs = big_sets()
    Fs, _, _ = big_guided(2.0)
    got = check(engine, big_dev, BIG, 8, pl, refs, forms=[(2, True)], guide=(Fs, 1e30), tag="B7 band 1e30")
    plain = run_knn(engine, big_dev, BIG, 8, pl, 2, True, sentinel=SENT)
    for g, u in zip(got, plain):
        assert g.tobytes() == u.tobytes()
    check(engine, big_dev, BIG, 8, pl, big_guided(2.0)[1], forms=[(2, True)], guide=(Fs, 2.0), tag="B7 band 2")


# ==== C. the shared count and selection rules ==================================================================================
CLAMP_STRIDE, CLAMP_MAX = 320, 257
CLAMP_COUNTS = [300, 5000, CLAMP_STRIDE + 9, -5, 257, 100, 0]


@functools.lru_cache(maxsize=None)
def clamp_sets(words):
    """Seven frames of 320 stored entries each, noisy permuted copies of one set, under counts of 300, 5000, stride + 9
    (all clamped to max_count = 257), -5 (no entry), 257, 100 and 0"""
    rng = np.random.default_rng(1200 + words)
    base = rnd(rng, CLAMP_STRIDE, words)
    frames = [(synth.flip_bits(rng, base[rng.permutation(CLAMP_STRIDE)], rng.integers(0, 4, CLAMP_STRIDE)),
               pts(rng, CLAMP_STRIDE, 400, 300)) for _ in CLAMP_COUNTS]
    eff = [min(max(c, 0), CLAMP_MAX) for c in CLAMP_COUNTS]
    assert eff == [257, 257, 257, 0, 257, 100, 0]
    pl = [(0, 1), (1, 0), (2, 4), (4, 2), (3, 0), (0, 3), (5, 1), (1, 5), (2, 2), (6, 3), (5, 6)]
    cut = [(d[:n], k[:n]) for (d, k), n in zip(frames, eff)]
    Fs = [rng.normal(size=9).astype(np.float32) for _ in pl]
    refs = [ref_knn(cut[a][0], cut[b][0]) for a, b in pl]
    grefs = guided_refs(cut, pl, Fs, 25.0)
    # the clamp matters: with the entries up to the stored count the answers differ
    loose = ref_knn(frames[0][0][:300], frames[1][0])
    assert (loose[0][:257] != refs[0][0]).any() and (loose[2][:257] != refs[0][2]).any()
    assert n_found(grefs) > 300 and (refs[4][2] == -1).all() and (refs[5][0] == -1).all()
    return frames, pl, Fs, refs, grefs


@functools.lru_cache(maxsize=None)
def ratio_sets(words):
    """One image pair per case, one row against three columns (the third the row's complement).  Cases 0 .. kmax - 1: the
    columns at 4k and 5k bits from the row.  float32(0.8) = 0.800000011920929 > 0.8, so 4k < float32(0.8) * 5k holds in
    double; the float32 product rounds to 4k and would reject.  Then (d, d), (d - 1, d), (0, 0) and (0, 1)."""
    rng = np.random.default_rng(1300 + words)
    kmax = min(51, 32 * words // 5)
    cases = [(4 * k, 5 * k) for k in range(1, kmax + 1)] + [(40, 40), (39, 40), (0, 0), (0, 1)]
    frames, pl = [], []
    for q, (d1, d2) in enumerate(cases):
        base = rnd(rng, 1, words)
        c1, c2 = synth.flip_bits(rng, base, d1), synth.flip_bits(rng, base, d2)
        assert d1 != d2 or d1 == 0 or (c1 != c2).any()
        frames += [(base, pts(rng, 1, 100, 100)), (np.concatenate([c1, c2, ~base]), pts(rng, 3, 100, 100))]
        pl.append((2 * q, 2 * q + 1))
    refs = [ref_knn(frames[a][0], frames[b][0]) for a, b in pl]
    r32 = np.float32(0.8)
    for q, (d1, d2) in enumerate(cases):
        assert refs[q][0][0].tolist() == [0, 1] and refs[q][1][0].tolist() == [d1, d2]
        s8, s1 = ref_select(*refs[q], 10**6, 0.8, False)[0].tolist(), ref_select(*refs[q], 10**6, 1.0, False)[0].tolist()
        if q < kmax:
            assert s8 == [0, 0, d1] and not np.float32(d1) < r32 * np.float32(d2)       # accepted; float32 says no
            assert float(d1) < float(r32) * float(d2) and s1 == [0, 0, d1]
        else:
            assert s1 == ([0, 0, d1] if d1 < d2 else [0, -1, NONE])                     # ratio 1: (d - 1, d) and (0, 1) pass
            assert s8 == ([0, 0, d1] if (d1, d2) == (0, 1) else [0, -1, NONE])
    Fs = [rng.normal(size=9).astype(np.float32) for _ in pl]
    for (a, b), F in zip(pl, Fs):
        assert admissible(frames[a][1], frames[b][1], F, 1e30).all()
    return frames, pl, Fs, refs


@functools.lru_cache(maxsize=None)
def gate_sets(words):
    """40 rows against 60 columns, max_dist = 10: row 3 at exactly 10 from column 7, row 4 at 11 from column 8; rows 10 and
    20 are equal and two bits from column 9, their common nearest"""
    rng = np.random.default_rng(1400 + words)
    a, b = rnd(rng, 40, words), rnd(rng, 60, words)
    a[3], a[4] = flip1(rng, b[7], 10), flip1(rng, b[8], 11)
    a[10] = a[20] = flip1(rng, b[9], 2)
    frames = [(a, pts(rng, 40, 500, 500)), (b, pts(rng, 60, 500, 500))]
    r = ref_knn(a, b)
    assert r[1][3, 0] == 10 and r[1][4, 0] == 11 and r[0][10, 0] == r[0][20, 0] == 9 and r[2][9] == 10
    crossed, plain = ref_select(*r, 10, 0.0, True), ref_select(*r, 10, 0.0, False)
    assert crossed[3].tolist() == [3, 7, 10] and crossed[4].tolist() == [4, -1, NONE]
    assert crossed[10].tolist() == [10, 9, 2] and crossed[20].tolist() == [20, -1, NONE] and plain[20].tolist() == [20, 9, 2]
    assert (plain[:, 1] >= 0).sum() == 3 and (ref_select(*r, 11, 0.0, False)[:, 1] >= 0).sum() == 4
    F = rng.normal(size=9).astype(np.float32)
    assert admissible(frames[0][1], frames[1][1], F, 1e30).all()
    return frames, [(0, 1)], [F], [r]


@gpu
@pytest.mark.parametrize("words", [8, 3])
def test_counts_above_max_count_and_below_zero(engine, words):
    """knn, knn_guided, match_nn and match_guided under a counts tensor of the test's own"""
    import torch
    from match_gpu import DEV, upload
    frames, pl, Fs, refs, grefs = clamp_sets(words)
    d_desc, d_kp, _, _ = upload(CLAMP_STRIDE, words, *zip(*frames))
    dev = (d_desc, d_kp, torch.tensor(CLAMP_COUNTS, dtype=torch.int32, device=DEV), None)
    check(engine, dev, CLAMP_STRIDE, words, pl, refs, max_count=CLAMP_MAX, tag="C1 knn")
    check(engine, dev, CLAMP_STRIDE, words, pl, grefs, guide=(Fs, 25.0), max_count=CLAMP_MAX, tag="C1 guided")
    for cross in (False, True):
        check_nn(engine, dev, CLAMP_STRIDE, words, pl, refs, 32 * words // 4, 0.8, cross, max_count=CLAMP_MAX, tag="C1 nn")
        check_nn(engine, dev, CLAMP_STRIDE, words, pl, grefs, 32 * words // 4, 0.8, cross, guide=(Fs, 25.0), max_count=CLAMP_MAX,
                 tag="C1 guided nn")


@gpu
def test_greedy_counts_above_max_count_and_below_zero(engine):
    """pgx_match_batch_dev on the same frames and counts: tests/test_gpu_batch.py holds its clamp with counts of upload()'s
    making; here the stored count is past the stride as well, and one is negative (k_match_init clamps it to no entry)"""
    import torch
    from match_gpu import DEV, pairs_equal, upload
    from oracle import cref
    frames, _, _, _, _ = clamp_sets(8)
    eff = [min(max(c, 0), CLAMP_MAX) for c in CLAMP_COUNTS]
    pl = [(0, 1), (1, 0), (2, 4), (3, 0), (5, 1), (1, 5), (2, 2)]
    exps = [cref.match_sorted(frames[a][0][:eff[a]], frames[b][0][:eff[b]]) if eff[a] else None for a, b in pl]
    assert [len(e) if e is not None else 0 for e in exps] == [257, 257, 257, 0, 100, 257, 257]
    assert (exps[5]["dist"] != NONE).sum() == 100 and (exps[0]["dist"] != NONE).sum() == 257
    d_desc = upload(CLAMP_STRIDE, 8, [f[0] for f in frames])[0]
    d_counts = torch.tensor(CLAMP_COUNTS, dtype=torch.int32, device=DEV)
    d_pl = torch.tensor(pl, dtype=torch.int32, device=DEV)
    d_out = torch.full((len(pl), CLAMP_STRIDE, 3), -7, dtype=torch.int32, device=DEV)
    torch.cuda.synchronize()
    engine.match_batch_dev(d_desc, d_counts, CLAMP_STRIDE, 8, d_pl, len(pl), d_out, max_count=CLAMP_MAX)
    engine.check_status()
    out = d_out.cpu().numpy()
    for m, exp in enumerate(exps):
        n1 = 0 if exp is None else len(exp)
        assert n1 == 0 or pairs_equal(out[m, :n1], exp), (m, pl[m])
        assert (out[m, n1:] == -7).all(), (m, pl[m])


@gpu
@pytest.mark.parametrize("words", [8, 5])
def test_ratio_rule_is_evaluated_in_double(engine, words):
    from match_gpu import upload
    frames, pl, Fs, refs = ratio_sets(words)
    dev = upload(4, words, *zip(*frames))
    for ratio in (0.8, 1.0):
        check_nn(engine, dev, 4, words, pl, refs, 10**6, ratio, False, tag="C2 nn")
        check_nn(engine, dev, 4, words, pl, refs, 10**6, ratio, False, guide=(Fs, 1e30), tag="C2 guided")


@gpu
@pytest.mark.parametrize("words", [8, 3])
def test_gate_edge_and_cross_check_on_tied_rows(engine, words):
    from match_gpu import upload
    frames, pl, Fs, refs = gate_sets(words)
    dev = upload(64, words, *zip(*frames))
    for cross in (True, False):
        for max_dist in (10, 11):
            check_nn(engine, dev, 64, words, pl, refs, max_dist, 0.0, cross, tag="C3 nn")
            check_nn(engine, dev, 64, words, pl, refs, max_dist, 0.0, cross, guide=(Fs, 1e30), tag="C3 guided")


# ==== the builders and the mirrored arithmetic, without a GPU ==================================================================
def test_mirrored_arithmetic():
    assert [table_size(E) for E in (1, 8, 9, 32, 33, 64, 80)] == [16, 16, 32, 64, 128, 128, 256]
    assert [last_tile_first_col(n) for n in N2S] == [0, 0, 32, 4064, 4064, 4096, 4096, 8160, 8192]
    line = np.stack([np.arange(16384) % 2048, np.arange(16384) % 1024], 1)
    assert grid_plan(line, 16384) == (4, 128, 64) and grid_plan(line[:1], 16384) == (0, 1, 1) and grid_plan(line, 3)[1:] == (1, 1)
    assert sorted(table_occupied([3, 19, 35, 3], 16)) == [3, 4, 5]


@pytest.mark.parametrize("builder,args", [(column_edge_sets, (8,)), (column_edge_sets, (3,)), (row_edge_sets, (8,)),
                                          (row_edge_sets, (3,)), (boundary_tie_sets, ()), (distance_end_sets, ()),
                                          (cell_cap_sets, (8,)), (degenerate_box_sets, (8,)), (degenerate_box_sets, (5,)),
                                          (line_sets, (8,)), (line_sets, (5,)), (full_range_sets, (8,)), (full_range_sets, (5,)),
                                          (table_sets, (8,)), (table_sets, (3,)), (wide_key_sets, ()), (clamp_sets, (8,)),
                                          (clamp_sets, (3,)), (ratio_sets, (8,)), (ratio_sets, (5,)), (gate_sets, (8,)),
                                          (gate_sets, (3,))])
def test_inputs_have_the_properties_they_were_built_for(builder, args):
    """every builder asserts its properties on the reference's result as it runs"""
    assert builder(*args)


def test_big_inputs_and_the_wide_reference():
    """ref_wide against ref_knn / ref_guided on a small input, then the 2^20 sets (their builders assert the planted entries)"""
    rng = np.random.default_rng(1)
    a, b = rnd(rng, 3, 8), rnd(rng, 500, 8)
    b[7] = b[400] = a[1]
    for x, y in zip(ref_wide(a, b, block=128), ref_knn(a, b)):
        assert (x == y).all()
    ka, kb, F = pts(rng, 3, 100, 100), pts(rng, 500, 100, 100), rng.normal(size=9).astype(np.float32)
    adm = admissible(ka, kb, F, 4.0)
    assert 0 < adm.sum() < 1500 and not adm.all(1).any()
    for x, y in zip(ref_wide(a, b, adm, block=128), ref_guided(a, b, ka, kb, F, 4.0)):
        assert (x == y).all()
    descs, kps, pl, refs = big_sets()
    assert len(descs[0]) == BIG == 1 << 20 and kps[0].shape == (BIG, 2)
    Fs, grefs, n_adm = big_guided(2.0)
    assert admissible(kps[0], kps[1], Fs[0], 1e30).all() and admissible(kps[1], kps[0], Fs[1], 1e30).all()
    assert n_adm > 100 and (grefs[0][0][:, 0] >= 0).sum() > 100 and (grefs[1][2] >= 0).sum() == len(np.flatnonzero(
        admissible(kps[1], kps[0], Fs[1], 2.0).any(0)))
