"""GPU tests of the fused detect chain's NMS (photogrammetry_amd/csrc/k_nms.hip: pgx_detect_batch_dev -> pgx_launch_nms) past
its cell, reach, tile and sort limits.  Every check is exact equality with the oracle chain (match_gpu.oracle_detect): x, y,
fast_score, value bits, descriptors, counts, n_raw, and the untouched rows behind every list.  Every scene precondition is an
assert on the CPU, from the oracle alone.

  limit (k_nms.hip)                               one side                               other side
  ----------------------------------------------  -------------------------------------  ------------------------------------
  r < 0: no round, nms_finish gathers and sorts   row1[-1], row9[-1]                     row1[0] (general path, 14 rounds)
  champion radii 10 <= r <= 192                   row1[9] general, planes, cs 16         row1[10] mask, cs 8, R 2
                                                  row1[192] champion, cs 64, R 3         row1[193], row1[300], row8[300] lists
  reach R = ceil(r / cs): 2 | 3                   row1 + row2 [16 | 32 | 64 | 128]       row1 + row2 [17 | 33 | 65 | 129]
  cell size 8 | 16 | 32 | 64                      row1 + row2 [21 | 43 | 89]             row1 + row2 [22 | 44 | 90]
  distance == r at the far end of the reach       row2 (dropped, all four directions)    row2 (first offset beyond r: kept)
  mask tile 256 x 64 px (MT_W x MT_H cells)       row2 (pair inside: the corner group)   row2 (pair across, both axes), row3
  frame edge: last partial cell, 64-px segment    row3 (64 x 40), (256 x 64)             row3 (63 | 65 x 40), (257 x 65), row2
  hits on one row / one column, no hit at all     row3 (300 x 7), (7 x 300)              row3 (6 x 6)
  fixed rounds 5 (mask) | 8 (champion) -> tail    row1 (noise: done before the tail)     row4 (chains need 20+ rounds more)
  nms_mask_ok: W, H <= 16384                      row1[10..21]                           row5 (k_nms_bin_planes8 + phase_c, cs 8)
  n_cap <= 2^24 for champion rounds               row1[16]                               row6 (general path at r = 16, 30)
  tail_order, k_nmsm_tail: bitmap passes lp = 5   row1[12 is not there: 10..21]          row7 lp = 3, lp = 1
  tail_order, k_nms_tail: lp = 5                  row1[22..192]                          row7 lp = 2
  k_nmsm_tail: n <= 64 * MT_SORT_LDS (bitmap)     row7 lp = 1                            row7 bitonic (kept <= 8192), compaction (>)
  max_raw_per_frame                               row8 under frame                       row8 over frame (r = 8, 12, 25, 300)
  survivor limit: soft | hard, each order writer  row9 soft 50 (r = 12, 25, 8, -1)       row9 capacity 50 (same radii)

Two scenes do not come out as the limits' list first suggested, both by arithmetic that the tests restate: a single line of
hits 7 px apart across 700 px needs only 25 rounds at r = 22 and 15 at r = 44, fewer than 8 + 20, so row 4 runs the single
lines where they are long enough and a Z of row, anti-diagonal and row (one chain, 298 hits) at every radius; and at r = 1
the hits of row 2 are 1 or 2 px apart, and two of them lie on each other's circle and score 15 (asserted as such).  Row 7's frames
are the only ones above 1 Mpx; their oracle runs for seconds (the literal O(n * kept) loop), the GPU for milliseconds."""
import numpy as np
import pytest

from match_gpu import detect_equal, oracle_detect, run_detect
from oracle import cref
import photogrammetry_amd as pg

pytestmark = pytest.mark.gpu

T = np.float32(0.1)
RAW = 1 << 17                     # max_raw_per_frame unless a row sets its own
NO_LIMIT = 1 << 20                # max_keypoints_per_frame: none
MT_SORT_LDS, SORT_LDS_MAX = 8192, 16384
RADII = (-1, 0, 1, 9, 10, 16, 17, 21, 22, 32, 33, 43, 44, 64, 65, 89, 90, 128, 129, 192, 193, 300)


@pytest.fixture(scope="module")
def engine():
    """Own context: these tests change the radius and the capacities all the time."""
    e = pg.Engine(0)
    e.set_brief_pairs(brief_pairs())
    e.set_dewarp_map(None)
    yield e
    e.set_capacity(RAW, NO_LIMIT)
    e.set_dewarp_map(None)
    e.close()


def brief_pairs(_made=[]):
    if not _made:
        _made.append(pg.make_brief_pairs(1, 50, 256))
    return _made[0]


# ---- nms_layout()'s rule, restated

def nms_path(r, W, H, raw_cap=RAW):
    """-> (kind, cs, R, fixed whole-chip rounds): kind "none" (r < 0), "mask", "champion", "general" (plane binning) or
    "lists" (general path on the compacted raw lists)"""
    if r < 0:
        return "none", 0, 0, 0
    if 10 <= r <= 192 and raw_cap <= 1 << 24:
        cs = 64 if r >= 90 else 32 if r >= 44 else 16 if r >= 22 else 8
        mask = cs == 8 and W <= 16384 and H <= 16384
        return ("mask" if mask else "champion"), cs, -(-r // cs), (5 if mask else 8)
    cs = 16 if r <= 16 else 32 if r <= 32 else 64 if r <= 64 else r
    return ("general" if cs in (16, 32, 64) else "lists"), cs, 1, 14


def bitmap_levels_per_pass(n, lds_cap):
    """tail_order's rank-bitmap branch: score levels per pass, or None when n raster ranks do not fit (champion rounds only)"""
    nw = 2 * ((n + 63) // 64)
    return min(5, 2 * lds_cap // nw) if nw <= 2 * lds_cap else None


# ---- scenes

def noise(W, H, seed):
    return np.random.default_rng(seed).integers(0, 65536, (H, W, 4), dtype=np.uint16)


def planted(W, H, points):
    """flat grey with single pixels of another level: each an isolated FAST hit of score 16 where the points keep 3 px from the
    border and 4 px (Chebyshev) from each other, so every score ties and raster order decides"""
    f = np.full((H, W, 4), 16384, dtype=np.uint16)
    f[..., 3] = 65535
    for x, y in points:
        f[y, x, :3] = 49152
    return f


def raw_of(frame):
    return cref.detect(cref.gray(frame), T)


def assert_raw_is(frame, points):
    raw = raw_of(frame)
    exp = sorted(points, key=lambda p: (p[1], p[0]))
    assert [(int(x), int(y)) for x, y in zip(raw["x"], raw["y"])] == exp and (raw["fast_score"] == 16).all()


_ORACLE = {}


def oracle(key, frame, radius, raw_cap=None):
    """oracle_detect without a survivor limit, once per (scene, radius, raw capacity)"""
    k = (key, radius, raw_cap)
    if k not in _ORACLE:
        _ORACLE[k] = oracle_detect(frame, None, brief_pairs(), T, radius, NO_LIMIT, raw_cap)
    return _ORACLE[k]


def check(engine, keys, frames, radius, raw_cap=RAW):
    """one launch over frames [F][H][W][4] (keys: their names in the oracle cache) at `radius`, every frame against the oracle;
    the call's capacity is the longest expected list + 3 -> the oracle's triples"""
    exp = [oracle(k, f, radius) for k, f in zip(keys, frames)]
    cap = max(len(e[0]) for e in exp) + 3
    engine.set_detect_params(T, radius)
    engine.set_capacity(raw_cap, NO_LIMIT)
    out = run_detect(engine, frames, cap)
    engine.check_status()
    for f, (kept, edesc, n_raw) in enumerate(exp):
        assert n_raw <= raw_cap
        detect_equal(out, f, kept, edesc, n_raw)
    return exp


# ---------------------------------------------------------------------------------------------------------------- row 1

def test_row1_radii_reach_every_regime():
    """(not a kernel test: the list below) every (cs, R) of {8, 16, 32, 64} x {2, 3}, the general path below 10 with plane
    binning at cs = 16, the general path above 192 without planes, no round at all; and both sides of every switch."""
    got = {nms_path(r, 451, 383)[:3] for r in RADII}
    for cs in (8, 16, 32, 64):
        for R in (2, 3):
            assert ("mask" if cs == 8 else "champion", cs, R) in got
    assert ("general", 16, 1) in got and ("lists", 193, 1) in got and ("lists", 300, 1) in got and ("none", 0, 0) in got
    for a, b in ((9, 10), (16, 17), (21, 22), (32, 33), (43, 44), (64, 65), (89, 90), (128, 129), (192, 193)):
        assert a in RADII and b in RADII and nms_path(a, 451, 383) != nms_path(b, 451, 383)
    assert nms_path(9, 451, 383)[0] == "general" and nms_path(193, 451, 383)[0] == "lists"


ROW1_BIG = noise(451, 383, 101)[None]                                  # 8 x 6 cells at cs = 64, no side a multiple of 8
ROW1_SMALL = np.stack([noise(70, 66, 102 + i) for i in range(3)])      # F = 3, two 64-px segments per row


@pytest.mark.parametrize("radius", RADII)
def test_row1_every_regime_451x383(engine, radius):
    """row 1: dense noise (every score level, dozens of hits per cell) at every radius of the list"""
    (kept, _, n_raw), = check(engine, ["big"], ROW1_BIG, radius)
    assert n_raw > 20000 and len(kept) >= 3


@pytest.mark.parametrize("radius", RADII)
def test_row1_every_regime_three_frames_70x66(engine, radius):
    """row 1: three small frames per launch (blockIdx.y = frame in every kernel of the path)"""
    exp = check(engine, ["small0", "small1", "small2"], ROW1_SMALL, radius)
    assert all(e[2] > 300 for e in exp)


# ---------------------------------------------------------------------------------------------------------------- row 2

def diag_offsets(r):
    """by brute force over |dx - dy| <= 1 (dy >= dx): the longest offset with dx^2 + dy^2 <= r^2 and the shortest beyond"""
    cand = [(dx, dy) for dx in range(r + 2) for dy in (dx, dx + 1) if (dx, dy) != (0, 0)]
    d2 = lambda o: o[0] * o[0] + o[1] * o[1]
    return max((o for o in cand if d2(o) <= r * r), key=d2), min((o for o in cand if d2(o) > r * r), key=d2)


def last_of_cell(x0, cs):
    return x0 // cs * cs + cs - 1


def exact_r_scene(r):
    """-> (W, H, keep, drop, pairs): groups more than r apart from each other.  Every anchor sits on the last column and the last
    row of its cell, so that its partner at distance exactly r lies R cells away.
      D  anchor + partners at (r, 0), (0, r), the longest diagonal offset and its mirror image to the left: all dropped; the
         anchor is (255, 63), the last cell of mask tile (0, 0), wherever cells divide 64
      K  anchor + (r + 1, 0) + (0, r + 1), and a second anchor + the shortest diagonal offset beyond r: all kept
      E  anchor + (r, 0) + (0, r) with both partners in the frame's last, partial cell (3 px from the border): dropped"""
    cs = nms_path(r, 451, 383)[1]
    add = lambda p, o: (p[0] + o[0], p[1] + o[1])
    (dx, dy), (ex, ey) = diag_offsets(r)
    a = (255, 63) if cs <= 64 else (cs - 1, cs - 1)
    k1 = (last_of_cell(a[0] + 2 * r + 2, cs), a[1])
    k2 = (a[0], last_of_cell(a[1] + 2 * r + 2, cs))
    W = next(w for w in range(k1[0] + r + 6, k1[0] + r + 6 + 2 * cs) if 4 <= w % cs)
    H = next(h for h in range(max(k2[1] + ey + 4, a[1] + 3 * r + 7), 1 << 16) if 4 <= h % cs)
    e = (W - 4 - r, H - 4 - r)
    pairs = [(a, add(a, o)) for o in ((r, 0), (0, r), (dx, dy), (-dx, dy))] + [(e, add(e, (r, 0))), (e, add(e, (0, r)))]
    keep = {a, e, k1, add(k1, (r + 1, 0)), add(k1, (0, r + 1)), k2, add(k2, (ex, ey))}
    drop = {b for _, b in pairs}
    assert not (keep & drop) and all(3 <= x < W - 3 and 3 <= y < H - 3 for x, y in keep | drop)
    return W, H, keep, drop, pairs


@pytest.mark.parametrize("radius", [r for r in RADII if r >= 1])
def test_row2_distance_exactly_r_at_the_far_end_of_the_reach(engine, radius):
    """row 2: partners at distance exactly r, R cells away, are dropped; the first offset beyond r is kept: horizontally,
    vertically, diagonally, across a mask tile edge in x and in y, and into the frame's last partial cell"""
    W, H, keep, drop, pairs = exact_r_scene(radius)
    kind, cs, R, _ = nms_path(radius, W, H)
    frame = planted(W, H, keep | drop)
    raw = raw_of(frame)
    rawxy = [(int(x), int(y)) for x, y in zip(raw["x"], raw["y"])]
    if radius >= 4:
        assert_raw_is(frame, keep | drop)
    else:   # neighbours 2 px apart diagonally lie on each other's circle: score 15; every anchor still beats its partner
        score = {p: int(s) for p, s in zip(rawxy, raw["fast_score"])}
        assert set(rawxy) == keep | drop and len(rawxy) == len(score) and min(score.values()) >= 15
        assert all(score[a] >= score[b] and (a[1], a[0]) < (b[1], b[0]) for a, b in pairs)
    for a, b in pairs:
        assert (a[0] - b[0]) ** 2 + (a[1] - b[1]) ** 2 <= radius ** 2
        assert a[0] % cs == cs - 1 and a[1] % cs == cs - 1 or a == (W - 4 - radius, H - 4 - radius)
    (a, bh), (_, bv) = pairs[0], pairs[1]
    assert bh[0] // cs - a[0] // cs == R or kind in ("general", "lists")       # at the far end of the reach
    assert bv[1] // cs - a[1] // cs == R or kind in ("general", "lists")
    if kind == "mask":
        assert a[0] // 256 != bh[0] // 256 and a[1] // 64 != bv[1] // 64       # across a tile edge, both axes
    (_, eh), (_, ev) = pairs[4], pairs[5]
    assert W % cs and H % cs and eh[0] // cs == (W - 1) // cs and ev[1] // cs == (H - 1) // cs   # the last partial cell
    (kept, _, _), = check(engine, ["exact"], frame[None], radius)
    assert {(int(x), int(y)) for x, y in zip(kept["x"], kept["y"])} == keep


# ---------------------------------------------------------------------------------------------------------------- row 3

@pytest.mark.parametrize("radius", [12, 50])
@pytest.mark.parametrize("W,H", [(63, 40), (64, 40), (65, 40), (256, 64), (257, 65), (300, 7), (7, 300), (6, 6)])
def test_row3_frame_shapes_around_segment_cell_and_tile(engine, W, H, radius):
    """row 3: one 64-px segment exactly, one pixel less and more; one mask tile exactly and one pixel more; hits on a single
    row or column; a frame too small for any hit, which still runs"""
    (kept, _, n_raw), = check(engine, [("shape", W, H)], noise(W, H, 300 + W)[None], radius)
    if (W, H) == (6, 6):
        assert n_raw == 0
    elif min(W, H) == 7:
        assert n_raw > 20 and (len(set(kept["y"])) == 1 if H == 7 else len(set(kept["x"])) == 1)
    else:
        assert n_raw > 200


# ---------------------------------------------------------------------------------------------------------------- row 4

def rounds_needed(pts, r):
    """k_nms.hip's round rule on points of one score in raster (= priority) order: accept every undecided point with no
    better undecided point within r, then suppress within r of the accepted -> rounds until nothing is undecided"""
    p = np.array(sorted(pts, key=lambda q: (q[1], q[0])), dtype=np.int64)
    d = p[:, None, :] - p[None, :, :]
    within = (d * d).sum(2) <= r * r
    better = np.arange(len(p))[None, :] < np.arange(len(p))[:, None]        # [i][j]: j is better than i
    und = np.ones(len(p), dtype=bool)
    rounds = 0
    while und.any():
        acc = und & ~(within & better & und[None, :]).any(1)
        und &= ~acc & ~within[:, acc].any(1)
        rounds += 1
    return rounds


STEPS = range(100)   # 3, 10, ..., 696
CHAINS = {
    "row": [(3 + 7 * k, 3) for k in STEPS],
    "column": [(3, 3 + 7 * k) for k in STEPS],
    "diagonal": [(3 + 7 * k, 3 + 7 * k) for k in STEPS],
    # one chain: along the top row, back down the anti-diagonal, along the bottom row
    "z": [(3 + 7 * k, 3) for k in STEPS] + [(696 - 7 * k, 3 + 7 * k) for k in range(1, 99)] + [(3 + 7 * k, 696) for k in STEPS],
}
# a line of 100 hits is decided in 100 / (hits within r of the head + 1) rounds: 50 and 34 at r = 10 and 17 (diagonal, step
# 9.9 px: 50 and 50); at r = 22 only the diagonal (34) is long enough for 8 + 20, at r = 44 no line is (15, 15, 20).  The Z
# needs 148, 113, 81 and 47 rounds
CHAIN_CASES = [("row", 10), ("row", 17), ("column", 10), ("column", 17), ("diagonal", 10), ("diagonal", 17), ("diagonal", 22),
               ("z", 10), ("z", 17), ("z", 22), ("z", 44)]


def chain_frame(name, radius):
    pts = CHAINS[name]
    frame = planted(700, 700, pts)
    assert_raw_is(frame, pts)
    fixed = nms_path(radius, 700, 700)[3]
    need = rounds_needed(pts, radius)
    assert fixed in (5, 8) and need >= fixed + 20, (need, fixed)      # the tail kernel finishes, over 20 rounds or more
    return frame


@pytest.mark.parametrize("name,radius", CHAIN_CASES)
def test_row4_chain_finished_by_the_tail_kernel(engine, name, radius):
    """row 4: equal scores 7 px apart: each hit waits for its predecessor, far more rounds than the whole-chip launches run"""
    check(engine, [("chain", name)], chain_frame(name, radius)[None], radius)


@pytest.mark.parametrize("radius", [10, 17, 22, 44])
def test_row4_chain_between_noise_frames(engine, radius):
    """row 4: the chain as frame 1 of three: its tail workgroup runs dozens of rounds beside two that have nothing left"""
    frames = np.stack([noise(700, 700, 401), chain_frame("z", radius), noise(700, 700, 402)])
    check(engine, ["n700a", ("chain", "z"), "n700b"], frames, radius)


# ---------------------------------------------------------------------------------------------------------------- row 5

@pytest.mark.parametrize("radius", [12, 20, 25])
@pytest.mark.parametrize("W,H", [(16448, 40), (40, 16448)])
def test_row5_frames_beyond_16384(engine, W, H, radius):
    """row 5: coordinates that do not fit the mask rounds' 14 bits: r = 12 and 20 run champion rounds on 8-px cells with
    per-hit records (k_nms_bin_planes8, k_nms_phase_c at R = 2 and 3); r = 25 for comparison"""
    kind, cs, R, _ = nms_path(radius, W, H)
    assert (kind, cs, R) == {12: ("champion", 8, 2), 20: ("champion", 8, 3), 25: ("champion", 16, 2)}[radius]
    (kept, _, n_raw), = check(engine, [("long", W, H)], noise(W, H, 500 + H)[None], radius)
    assert n_raw > 70000 and max(kept["x"].max(), kept["y"].max()) > 16384 + 40


# ---------------------------------------------------------------------------------------------------------------- row 6

def test_row6_raw_capacity_above_2_24_turns_champion_rounds_off():
    """row 6: ranks no longer fit champ_key's 24 bits, so r = 16 and r = 30 take the general path (plane binning, cs 16 and 32).
    A context of its own, closed at the end: a workspace only ever grows, and this one is 0.7 GB."""
    raw_cap = (1 << 24) + 1
    frame = noise(200, 136, 601)[None]
    e = pg.Engine(0)
    try:
        e.set_brief_pairs(brief_pairs())
        e.set_dewarp_map(None)
        for radius in (16, 30):
            assert nms_path(radius, 200, 136, raw_cap)[:2] == ("general", 16 if radius == 16 else 32)
            assert nms_path(radius, 200, 136)[0] in ("mask", "champion")
            (_, _, n_raw), = check(e, ["cap24"], frame, radius, raw_cap=raw_cap)
            assert n_raw > 3000
        e.set_capacity(RAW, NO_LIMIT)
    finally:
        e.close()


# ---------------------------------------------------------------------------------------------------------------- row 7
# White noise at T = 0.1 (cref.detect): 0.1411 of the pixels 3 px or more inside the frame are hits (0.1410 .. 0.1412 on
# 451 x 383, 640 x 480 and 1000 x 1000; scores 12..16 as 13 : 13 : 7 : 41 : 25 %), and the survivors per pixel are 0.00653 at
# r = 10, 0.00494 at r = 12, 0.00187 at r = 21, 0.00136 at r = 25.  Each size below is the smallest odd square, to a few px,
# whose n_raw clears its interval's lower end by 2 % (the density varies by 0.5 % from seed to seed).

def order_case(engine, W, H, seed, radius, raw_cap, lds_cap, lp, n_min, kept_range):
    frame = noise(W, H, seed)
    kind = nms_path(radius, W, H, raw_cap)[0]
    assert kind == ("mask" if lds_cap == MT_SORT_LDS else "champion")
    (kept, _, n_raw), = check(engine, [("order", W, H, seed)], frame[None], radius, raw_cap=raw_cap)
    assert n_min < n_raw <= raw_cap and bitmap_levels_per_pass(n_raw, lds_cap) == lp, n_raw
    assert kept_range[0] < len(kept) <= kept_range[1], len(kept)
    _ORACLE.clear()
    return n_raw, len(kept)


def test_row7_mask_tail_bitmap_three_levels_per_pass(engine):
    """row 7: 131 072 < n <= 174 720 on the mask path: passes over levels 16..14 and 13..11 (the sc >= 12 guard)"""
    order_case(engine, 981, 981, 701, 12, 1 << 18, MT_SORT_LDS, 3, 131072, (0, 8192))          # n_raw 133 686, kept 4 735


def test_row7_mask_tail_bitmap_one_level_per_pass(engine):
    """row 7: 262 144 < n <= 524 288 on the mask path: five passes of one level"""
    order_case(engine, 1385, 1385, 702, 12, 1 << 19, MT_SORT_LDS, 1, 262144, (8192, 1 << 20))  # n_raw 267 873, kept 9 446


def test_row7_champion_tail_bitmap_two_levels_per_pass(engine):
    """row 7: 349 504 < n <= 524 288 on the champion tail (r = 25): passes over 16..15, 14..13, 12..11"""
    order_case(engine, 1597, 1597, 703, 25, 1 << 19, SORT_LDS_MAX, 2, 349504, (0, 16384))       # n_raw 357 800, kept 3 463


def test_row7_mask_tail_bitonic(engine):
    """row 7: n > 64 * MT_SORT_LDS leaves the bitmap branch; 8192 survivors or fewer are sorted in LDS (r = 21)"""
    order_case(engine, 1951, 1951, 704, 21, 1 << 20, MT_SORT_LDS, None, 524288, (4096, 8192))   # n_raw 533 278, kept 7 046


def test_row7_mask_tail_compaction(engine):
    """row 7: n > 64 * MT_SORT_LDS and more than 8192 survivors (r = 10): one compaction pass per score over accflag[0..n), at
    max_raw_per_frame = 2^20 -- the capacity at which the mask layout used to give accflag no bytes at all"""
    order_case(engine, 1951, 1951, 704, 10, 1 << 20, MT_SORT_LDS, None, 524288, (8192, 1 << 20))  # n_raw 533 278, kept 24 798


# ---------------------------------------------------------------------------------------------------------------- row 8

ROW8_OVER = noise(200, 136, 801)
ROW8_UNDER = noise(200, 136, 802)
ROW8_UNDER[:, 100:] = 0            # hits on the left half only


def row8_capacity():
    """a max_raw_per_frame inside a row slice of the over frame: the last hit kept and the first one dropped share an 8-px
    cell row (so a 16-, 32-, 64-px one and a 64-px segment too), and the value is no multiple of 8"""
    raw, n_under = raw_of(ROW8_OVER), len(raw_of(ROW8_UNDER))
    c = next(c for c in range(len(raw) * 3 // 5, len(raw))
             if c % 8 and raw["y"][c - 1] == raw["y"][c] and raw["x"][c - 1] // 8 == raw["x"][c] // 8)
    assert n_under < c < len(raw) - 500 and n_under > 1000
    seg_first = np.flatnonzero((raw["y"] == raw["y"][c]) & (raw["x"] // 64 == raw["x"][c] // 64))[0]
    assert c % 8 != 0 and seg_first < c
    return c


@pytest.mark.parametrize("radius", [8, 12, 25, 300])
def test_row8_raw_capacity_overflow_keeps_the_first_hits_in_raster_order(engine, radius):
    """row 8: "hits past the raw capacity are dropped everywhere": k_nms_bin_planes (r = 8), k_nmsm_setup (12),
    k_nms_bin_planes8 cannot be reached below 16384 px, so k_nms_bin_planes<2> (25), and the clamped list (300)"""
    raw_cap = row8_capacity()
    frames = np.stack([ROW8_OVER, ROW8_UNDER])
    exp = [oracle("over", ROW8_OVER, radius, raw_cap), oracle("under", ROW8_UNDER, radius)]
    assert exp[0][2] > raw_cap > exp[1][2]
    cap = max(len(e[0]) for e in exp) + 3
    engine.set_detect_params(T, radius)
    engine.set_capacity(raw_cap, NO_LIMIT)
    out = run_detect(engine, frames, cap)
    with pytest.raises(pg.CapacityError):
        engine.check_status()
    engine.check_status()                                  # the status word is read and cleared
    for f in (0, 1):                                       # d_nraw of the over frame is the true total
        detect_equal(out, f, *exp[f])
    engine.set_capacity(RAW, NO_LIMIT)


def test_row8_overflow_in_bin_planes8(engine):
    """row 8: the third binning kernel, k_nms_bin_planes8, runs only beyond 16384 px: the same statement on 16448 x 40"""
    W, H, radius = 16448, 40, 12
    frame = noise(W, H, 500 + H)
    raw = raw_of(frame)
    c = next(c for c in range(len(raw) * 3 // 5, len(raw))
             if c % 8 and raw["y"][c - 1] == raw["y"][c] and raw["x"][c - 1] // 8 == raw["x"][c] // 8)
    assert nms_path(radius, W, H)[:2] == ("champion", 8)
    exp = oracle_detect(frame, None, brief_pairs(), T, radius, NO_LIMIT, c)
    assert exp[2] > c
    engine.set_detect_params(T, radius)
    engine.set_capacity(c, NO_LIMIT)
    out = run_detect(engine, frame[None], len(exp[0]) + 3)
    with pytest.raises(pg.CapacityError):
        engine.check_status()
    engine.check_status()
    detect_equal(out, 0, *exp)
    engine.set_capacity(RAW, NO_LIMIT)


# ---------------------------------------------------------------------------------------------------------------- row 9

@pytest.mark.parametrize("radius", [12, 25, 8, -1])
def test_row9_soft_and_hard_survivor_limit(engine, radius):
    """row 9: each writer of order[] (rank bitmap after mask and champion rounds, bitonic sort, per-score compaction) guards
    o < kp_cap on its own: a soft limit of 50 cuts to the oracle's first 50 without an error; a call's capacity of 50 raises,
    and the next call is whole"""
    kept, edesc, n_raw = oracle("big", ROW1_BIG[0], radius)
    assert len(kept) > 200
    if radius == 8:
        assert len(kept) <= SORT_LDS_MAX                   # the general path's bitonic sort
    if radius == -1:
        assert len(kept) == n_raw > SORT_LDS_MAX           # nothing is dropped: per-score compaction
    engine.set_detect_params(T, radius)
    engine.set_capacity(RAW, 50)
    out = run_detect(engine, ROW1_BIG, 64)
    engine.check_status()
    detect_equal(out, 0, kept[:50], edesc[:50], n_raw)
    engine.set_capacity(RAW, NO_LIMIT)
    out = run_detect(engine, ROW1_BIG, 50)
    with pytest.raises(pg.CapacityError):
        engine.check_status()
    assert int(out[3][0]) == n_raw
    check(engine, ["big"], ROW1_BIG, radius)
