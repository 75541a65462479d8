"""GPU tests of the detect front end past its tile, scan, grid and table limits: dewarp-grey (photogrammetry_amd/csrc/k_image.hip:
k_dewarp_gray), FAST (csrc/k_fast.hip: k_fast_planes, k_seg_scan, k_fast_compact) and plain BRIEF (csrc/k_brief.hip:
k_brief_list, k_brief_kept; the evaluators brief_256 and brief_one of csrc/k_brief_core.inc).  Every comparison is exact.  The
stage entry points are held to the C oracle: pgx_fast to cref.detect (x, y, score, value bits, raster order), pgx_gray and
pgx_dewarp to cref.gray and cref.apply_distortion, pgx_brief to cref.brief.  What runs only inside the chain (k_fast_compact
behind a batch's scan, the grey image of a batch, k_brief_kept) goes through pgx_detect_batch_dev and is held to
match_gpu.oracle_detect: lists, value bits, descriptors, counts, n_raw and the untouched rows behind every list.  The device
is never its own reference, and every scene's precondition is an assert on the oracle alone
(tests/test_front_limits_cases.py).

  limit (file: constant)                            one side                               other side
  ------------------------------------------------  -------------------------------------  ---------------------------------------
  -- k_fast.hip
  k_seg_scan: 1024 * 4 = 4096 segments per pass,    scan[64 x 4096] one full pass          scan[64 x 4097] (n_raw through the carry),
    carry_s into the next                                                                  [63 x 8193] three passes, [64 x 4103],
                                                                                           [128 x 2053 | 2054] hits behind the pass
  k_seg_scan: (nseg & 3) == 0 vector | scalar load  scan[64 x 4096], [128 x 2050 | 2054]   scan[64 x 4097], [128 x 2049] (& 3 == 2),
                                                    (vector in a partial second pass)      [64 x 4103] (& 3 == 3), [63 x 8193] (1)
  TW x TH = 64 x 32 tile, queue[2048]               saturated[128 x 64] 61 hits a segment  saturated[192 x 70]: tile (1, 1) queues
                                                                                           all 2048 pixels
  64 hits per segment: ballot lane 63, 64 rounds    noise4 (3 a segment), [128 x 64]       saturated[192 x 70]: 32 full segments
    of the compaction loop
  HALO = 3: six halo lanes, hx < W                  edges[W = 63, 64, 65] no column right  edges[W = 66, 67, 69]: the halo ends inside
                                                    of the tile is read by a hit           the last three columns; [70, 71] all six
  tile edges x = 64, 128 and y = 32, 64             hits at x = 60 .. 63, y = 28 .. 31     hits at x = 64 .. 66, y = 32 .. 34 (the
                                                    (right / lower halo)                   neighbour's tile: left / upper halo)
  three score planes, code = score - 11             dense: score 16 alone                  noise4, nonfinite: every score 12 .. 16
  float compares with NaN, +-inf                    every other scene: finite grey         nonfinite[70 x 40]: hits ON NaN centres
  raw capacity: pos >= raw_cap, *n_out, status      capacity n                             n - 1, 64 k (a segment boundary), 64 k + 1
                                                                                           (inside a segment), 1, 0 with out = NULL
  chain: pgx_nms_fills_raw_lists (k_nms.hip)        batch r = -1, 0: k_fast_compact runs   batch[65 x 33] r = 12: champion rounds,
                                                                                           no k_fast_compact
  chain: frame f's counts at f * nseg               batch[65 x 33]: 66 segments, frame 1   batch[64 x 4097]: two passes per frame;
                                                    starts 8 bytes off 16, one pass        [64 x 4103]: hits behind the first pass
  -- k_image.hip
  grid cap 512 workgroups (F = 1): the stride loop  earlier tests: <= 172 733 px, and      host[1024 x 513] 525 312 px: a second pass
    starts above 512 * 256 * 4 = 524 288 px         batch[*]'s first pass                  of 256 groups
  F == 1: vector path whatever npix; the last       host[1024 x 513] npix & 3 == 0         host[1023 x 513] 524 799 px: the scalar
    partial group of four is scalar                                                        tail of three inside the second pass
  grid cap max(512 / ceil(F / 4), 32) per group     earlier tests: F <= 9, 512 / 3 = 170   batch F = 61, 64: 16 groups, the floor of
                                                    workgroups cover the frame             32, two passes over 34 000 px
  FB = 4 frames per thread: nf = min(4, F - f0)     batch F = 64: nf == 4 throughout       batch F = 61: the last group has nf == 1
  (npix & 3) == 0 || F == 1: vector | scalar path   batch[200 x 170] vector                batch[201 x 171] 34 371 px: scalar
  ok[k]: out-of-range entries give black pixels     good map: status clean                 three entries spoiled: in a full vector
    and PGX_ST_OOB_SOURCE                                                                  group, in the frame's last group (the
                                                                                           last pixel) and mid-frame; on 201 x 171
                                                                                           all three on the scalar path
  SRC8: widen8's two byte selectors                 16-bit sources                         every case again from RGBA8
  -- k_brief.hip, k_brief_core.inc, pgx_api.hip
  k_brief_core.inc: xs >= 0 && xs < W, ys likewise  inside points, both corners            outside[(-1, -1), (W, H)] some pairs still
    (brief_256 in[g]; brief_one's two tests)                                               inside; [(W + 50, 3), (3, -50),
                                                                                           (+-2^30, 5), (5, +-2^30)] none: all zero
  pgx_api.hip: P <= 4064 (127 words)                tables[4063, 4064]                     4065: PGX_E_BADARG, the table set before
                                                                                           it stays in force
  k_brief_core.inc: 64 pairs per ballot chunk,      tables[32, 64, 128, 4064] off = 0 or   tables[31, 63, 65, 127, 4033, 4063] a last
    off = P - 64 (c + 1) < 0 on the last chunk      -32: whole words                       chunk shifted down by 1 .. 63 bits
  k_brief.hip: P == 256 brief_256 | brief_one       outside[256], lengths[256], map[256]   outside[70], lengths[70], map[100], tables
  k_brief.hip: four keypoints per workgroup,        lengths[4, 8] full workgroups          lengths[0, 1, 3, 5, 9]; map: 7 and 5
    k >= n (list), k >= nk (kept)                                                          survivors in two blocks, the last ragged
  k_brief.hip: groups of eight frames, the map's    map[F = 8, 16] first branch alone      map[F = 7] remainder alone; [9, 10, 17] both
    branches Lid < nblk * F8 | remainder                                                   (10: a remainder of two frames, which a
                                                                                           round-robin remainder would not cover)
  k_brief.hip: counts_out[f] by block kb == 0 only  textured frames                        map: frame 3 flat (mid-group), and with
                                                                                           F >= 9 the last frame (the remainder's)
  pgx_api.hip: kp_eff = min(survivor limit, cap),   map[cap 7]: kp_eff == out_stride == 7  map[cap 9]: out_stride 9 above kp_eff 7;
    out_stride = cap                                                                       [cap 5]: cap lowers kp_eff (and
                                                                                           out_stride with it) to 5, a hard limit:
                                                                                           PGX_E_CAPACITY, the first 5 intact

FAST.  The dense 64 x 4097 frame of the batch has 237 278 hits, and the oracle's literal NMS loop takes n^2 / 2 steps whatever
the radius; at the radii that suppress nothing (-1 and 0: two hits never share a pixel) its result is its own stable sort by
score, which front_limits_cases.keep_all_detect restates and the CPU tests hold to cref.nms on the smaller frames.  Every
other comparison of the chain goes through match_gpu.oracle_detect itself.

Dewarp-grey.  The grey image of a batch is not an output of any entry point, which is why the batched cases compare keypoints
and descriptors, not pixels; for a map with out-of-range entries the expectation is the oracle chain on a dewarped frame whose
pixels there are black (cref.apply_distortion refuses such a map).  With more than one frame the path is the same for every
group of a frame (vec is block-uniform), so in a batch the "last partial group" of 201 x 171 takes the scalar path like the
rest of the frame; the partial group inside the vector path exists for F == 1 only and is host[1023 x 513]'s.

BRIEF.  pgx_prepare_detect takes kp_eff as the smaller of pgx_set_capacity's survivor limit and the call's cap, and the call's
cap is the output stride: the stride differs from kp_eff only when the call's cap is the larger one (cap 9), never the other
way round."""
import ctypes as C

import numpy as np
import pytest

import front_limits_cases as fc
from match_gpu import detect_equal, oracle_detect, run_detect
from oracle import cref
import photogrammetry_amd as pg
from photogrammetry_amd._lib import PGX_E_BADARG, PGX_E_CAPACITY, PGX_OK
from photogrammetry_amd.api import _ptr

pytestmark = pytest.mark.gpu

SENT = -7
RAW, NO_LIMIT = 1 << 18, 1 << 20
CAP = 1024                        # the call's capacity of the image batches
W, H = 83, 60                     # the frame of the BRIEF list cases


@pytest.fixture(scope="module")
def eng():
    """Own context: these tests change the table, the threshold, the radius, the map, the source format and the capacities
    all the time; every test sets what it depends on."""
    e = pg.Engine(0)
    e.set_dewarp_map(None)
    yield e
    e.close()


# ==== FAST ============================================================================================================================

def brief_pairs(_made=[]):
    if not _made:
        _made.append(cref.gaussian_pairs(1, 50, 256))
    return _made[0]


def _fast_equals_oracle(eng, g, T):
    eng.set_detect_params(T, 0)
    exp = cref.detect(g, T)
    fc.same_hits(eng.fast(g), exp)
    return exp


# ---- pgx_fast -----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", ["dense", "noise4"])
@pytest.mark.parametrize("w,h", fc.SCAN_SHAPES + fc.SCAN_BEYOND)
def test_scan_passes(eng, w, h, kind):
    exp = _fast_equals_oracle(eng, *fc.fast_scene(kind, w, h))
    assert len(exp) > 1000


@pytest.mark.parametrize("w,h", fc.SATURATED_SHAPES)
def test_saturated_tile(eng, w, h):
    exp = _fast_equals_oracle(eng, fc.dense(w, h), fc.T_DENSE)
    assert len(exp) == (w - 6) * (h - 6)


@pytest.mark.parametrize("w", fc.EDGE_W)
def test_halo_and_tile_edges(eng, w):
    for h in fc.EDGE_H:
        for kind in ("dense", "noise4"):
            _fast_equals_oracle(eng, *fc.fast_scene(kind, w, h))


def test_nonfinite_grey(eng):
    exp = _fast_equals_oracle(eng, fc.nonfinite(), fc.T_NOISE)
    assert np.isnan(exp["value"]).sum() > 50               # the value bits of those are the frame's own NaNs, compared as bits


def _fast_abi(eng, g, capacity, room):
    """pgx_fast itself on a sentinel-filled array of `room` entries -> (return code, *n_out, the array)"""
    out = np.full((room, 4), SENT, dtype=np.int32)
    n = C.c_int(SENT)
    rc = eng._L.pgx_fast(eng._h, _ptr(g), g.shape[1], g.shape[0], _ptr(out) if capacity > 0 else None, capacity, C.byref(n))
    return rc, n.value, out


@pytest.mark.parametrize("scene", ["dense", "noise4"])
def test_raw_capacity(eng, scene):
    g, T, w = (fc.dense(192, 70), fc.T_DENSE, 192) if scene == "dense" else (fc.noise4(129, 65, 1), fc.T_NOISE, 129)
    exp = cref.detect(g, T)
    n = len(exp)
    want = np.ascontiguousarray(exp).view(np.int32).reshape(n, 4)          # KEYPOINT_DTYPE is four 32-bit fields
    eng.set_detect_params(T, 0)
    other = fc.dense(w + 1, g.shape[0])                                    # more hits than n, another pixel at every index past the first row
    for capacity in fc.capacities(exp, w):
        eng.set_detect_params(fc.T_DENSE, 0)                               # the library's raw lists are reused from call to call:
        assert len(eng.fast(other)) > n                                    # fill them with another frame's, so that an entry the
        eng.set_detect_params(T, 0)                                        # call under test leaves out cannot be right by chance
        rc, n_out, out = _fast_abi(eng, g, capacity, n + 8)
        assert n_out == n, capacity                                        # the full count, whatever fits
        assert rc == (PGX_OK if capacity >= n else PGX_E_CAPACITY), capacity
        kept = min(n, capacity)
        assert out[:kept].tobytes() == want[:kept].tobytes(), capacity     # the first entries are the oracle's, bit for bit
        assert (out[kept:] == SENT).all(), capacity                        # nothing behind them is written
        if rc != PGX_OK:
            eng.check_status()                                             # nothing stale: the failing call read the status word
            rc, n_out, out = _fast_abi(eng, g, n + 8, n + 8)
            assert rc == PGX_OK and n_out == n and out[:n].tobytes() == want.tobytes() and (out[n:] == SENT).all()
            eng.check_status()


# ---- FAST and the compaction in a batch -----------------------------------------------------------------------------------------------

def _batch(eng, frames, radius, exp, raw_cap=RAW):
    cap = max(len(e[0]) for e in exp) + 5
    eng.set_brief_pairs(brief_pairs())
    eng.set_detect_params(fc.T_DENSE, radius)
    eng.set_capacity(raw_cap, NO_LIMIT)
    out = run_detect(eng, frames, cap, sentinel=SENT)
    eng.check_status()
    for f, e in enumerate(exp):
        detect_equal(out, f, *e, sentinel=SENT)


@pytest.mark.parametrize("radius", [-1, 0, 12])
def test_batch_of_66_segment_frames(eng, radius):
    """case 1: frames 1 and 2 read their counts at f * 66 segments; r = 12 is the other side of pgx_nms_fills_raw_lists"""
    frames = fc.compact_batch(65, 33)
    exp = [oracle_detect(f, None, brief_pairs(), fc.T_DENSE, radius, NO_LIMIT) for f in frames]
    assert exp[1][2] == 59 * 27
    _batch(eng, frames, radius, exp)


@pytest.fixture(scope="module")
def tall():
    frames = fc.compact_batch(64, 4097)
    return frames, [fc.keep_all_detect(f, brief_pairs(), fc.T_DENSE) for f in frames]


@pytest.mark.parametrize("radius", [-1, 0])
def test_batch_of_two_pass_frames(eng, tall, radius):
    """case 2: a scan of two passes per frame, 237 278 hits in frame 1; the expectation is shared by the two radii"""
    frames, exp = tall
    assert exp[1][2] == 58 * 4091
    _batch(eng, frames, radius, exp)


@pytest.mark.parametrize("radius", [-1, 0])
def test_batch_with_hits_behind_the_first_pass(eng, radius):
    """case 2's other half: 64 x 4103, the hits in the last rows, so most offsets k_fast_compact reads hold the carry"""
    frames = fc.tail_batch(64, 4103)
    exp = [oracle_detect(f, None, brief_pairs(), fc.T_DENSE, radius, NO_LIMIT) for f in frames]
    _batch(eng, frames, radius, exp)


# ==== dewarp-grey ======================================================================================================================

def _source(eng, src8):
    eng.set_source_format(pg.api.PGX_SRC_RGBA8 if src8 else pg.api.PGX_SRC_RGBA64)


# ---- the host forms -------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("src8", [0, 1])
@pytest.mark.parametrize("w,h", [(1024, 513), (1023, 513)])
def test_host_forms_stride(eng, w, h, src8):
    assert fc.dewarp_grid(1, w * h)[3] == 2
    rng = np.random.default_rng(w + src8)
    if src8:
        a = rng.integers(0, 256, (h, w, 4), dtype=np.uint8)
        wide = a.astype(np.uint16) * 257
    else:
        a = wide = rng.integers(0, 65536, (h, w, 4), dtype=np.uint16)
    m = fc.perm_map(w, h, 7)
    try:
        _source(eng, src8)
        assert eng.gray(a).tobytes() == cref.gray(wide).tobytes()
        eng.set_dewarp_map(m)
        got = eng.dewarp(a)
        assert got.dtype == np.uint16 and got.tobytes() == cref.apply_distortion(wide, m).tobytes()
    finally:
        _source(eng, 0)
        eng.set_dewarp_map(None)


# ---- batches through the chain --------------------------------------------------------------------------------------------------------

_scenes, _expected = {}, {}


def _scene(w, h, src8):
    if (w, h, src8) not in _scenes:
        _scenes[w, h, src8] = fc.bad_scene(w, h, src8)
    return _scenes[w, h, src8]


def _expect(w, h, src8, f, entries=None):
    """the oracle chain on frame f, shared by the batch sizes; entries: those output pixels of the dewarp black"""
    key = (w, h, src8, f, entries is not None)
    if key not in _expected:
        frames, dmap, pairs = _scene(w, h, src8)
        if entries is None:
            _expected[key] = oracle_detect(frames[f], dmap, pairs, fc.BAD_T, fc.BAD_RADIUS, CAP)
        else:
            _expected[key] = fc.zeroed_detect(frames[f], dmap, entries, pairs, fc.BAD_T, fc.BAD_RADIUS, CAP)
    return _expected[key]


@pytest.mark.parametrize("src8", [0, 1])
@pytest.mark.parametrize("w,h", fc.BAD_SHAPES)
@pytest.mark.parametrize("F", fc.BAD_F)
def test_batch_with_a_map_and_with_entries_out_of_range(eng, F, w, h, src8):
    frames, dmap, pairs = _scene(w, h, src8)
    frames = frames[:F]
    host = (frames // 257).astype(np.uint8) if src8 else frames
    gx, ny, nf_last, passes, path = fc.dewarp_grid(F, w * h)
    assert (gx, ny, passes) == (32, 16, 2) and nf_last == (1 if F == 61 else 4) and path == ("vector" if w == 200 else "scalar")
    checked = fc.BAD_CHECKED + (F - 1,)
    entries = fc.bad_entries(w, h)
    eng.set_brief_pairs(pairs)
    eng.set_detect_params(fc.BAD_T, fc.BAD_RADIUS)
    eng.set_capacity(1 << 16, 1 << 20)
    try:
        _source(eng, src8)
        eng.set_dewarp_map(dmap)
        out = run_detect(eng, host, CAP, sentinel=SENT)
        eng.check_status()
        for f in checked:
            detect_equal(out, f, *_expect(w, h, src8, f), sentinel=SENT)
        assert not fc.lists_differ(_expect(w, h, src8, 0), fc.zeroed_detect(frames[0], dmap, [], pairs, fc.BAD_T, fc.BAD_RADIUS, CAP))
        # three entries out of range: the error, and black pixels exactly there
        eng.set_dewarp_map(fc.bad_map(dmap, entries))
        out = run_detect(eng, host, CAP, sentinel=SENT)
        with pytest.raises(pg.IndexOutOfRangeException):
            eng.check_status()
        changed = 0
        for f in checked:
            exp = _expect(w, h, src8, f, entries)
            detect_equal(out, f, *exp, sentinel=SENT)
            changed += fc.lists_differ(exp, _expect(w, h, src8, f))
        assert changed >= 3
        # the next call with a good map is clean
        eng.set_dewarp_map(dmap)
        out = run_detect(eng, host, CAP, sentinel=SENT)
        eng.check_status()
        for f in (0, F - 1):
            detect_equal(out, f, *_expect(w, h, src8, f), sentinel=SENT)
    finally:
        _source(eng, 0)
        eng.set_dewarp_map(None)


# ==== BRIEF ============================================================================================================================

def _kps(xy):
    k = np.zeros(len(xy), dtype=pg.KEYPOINT_DTYPE)
    if len(xy):
        k["x"], k["y"] = np.asarray(xy)[:, 0], np.asarray(xy)[:, 1]
    return k


def _brief_equals_oracle(eng, g, xy, pairs):
    got = eng.brief(g, _kps(xy))
    exp = cref.brief(g, xy, pairs)
    assert got.shape == exp.shape and got.dtype == np.uint32 and (got == exp).all()
    return exp


# ---- the list form ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("P", [256, 70])
def test_keypoints_outside_the_image(eng, P):
    g = fc.noise4(W, H, 4)
    pts, far = fc.outside_points(W, H)
    pairs = fc.table(P, seed=fc.OUTSIDE_SEED)
    eng.set_brief_pairs(pairs)
    exp = _brief_equals_oracle(eng, g, pts, pairs)
    assert not exp[far].any() and exp[~far].any(axis=1).sum() >= 8


@pytest.mark.parametrize("P", fc.TABLE_P)
def test_table_sizes(eng, P):
    g = fc.noise4(W, H, 6)
    pairs = fc.table(P)
    eng.set_brief_pairs(pairs)
    exp = _brief_equals_oracle(eng, g, fc.table_points(W, H), pairs)
    assert exp.shape[1] == (P + 31) // 32


def test_a_table_past_the_maximum_is_rejected_and_the_old_one_stays(eng):
    g = fc.noise4(W, H, 6)
    pairs = fc.table(64)
    eng.set_brief_pairs(pairs)
    with pytest.raises(pg.ArgumentException) as e:
        eng.set_brief_pairs(fc.table(fc.P_MAX + 1))
    assert e.value.code == PGX_E_BADARG
    assert eng.P == 64
    _brief_equals_oracle(eng, g, fc.table_points(W, H), pairs)


@pytest.mark.parametrize("P", [256, 70])
def test_list_lengths(eng, P):
    g = fc.noise4(W, H, 8)
    pairs = fc.table(P)
    eng.set_brief_pairs(pairs)
    pts = fc.table_points(W, H)
    for n in fc.LIST_N:
        _brief_equals_oracle(eng, g, pts[:n], pairs)


# ---- the kept form, through the chain -----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("P", [256, 100])
@pytest.mark.parametrize("F", fc.MAP_F)
def test_block_to_frame_map(eng, F, P):
    frames, flat = fc.map_frames(F)
    pairs = cref.gaussian_pairs(3, 8, P)
    words = (P + 31) // 32
    radius, limit = 3, 7
    eng.set_brief_pairs(pairs)
    eng.set_detect_params(fc.T_NOISE, radius)
    eng.set_capacity(1 << 16, limit)
    full = [oracle_detect(f, None, pairs, fc.T_NOISE, radius, 1 << 20) for f in frames]
    assert all((len(e[0]) == 0) == (f in flat) for f, e in enumerate(full)) and min(len(e[0]) for f, e in enumerate(full) if f not in flat) > limit
    try:
        for cap in (7, 9, 5):
            out = run_detect(eng, frames, cap, sentinel=SENT, words=words)
            if cap < limit:                                # the call's own capacity is a hard limit
                with pytest.raises(pg.CapacityError):
                    eng.check_status()
            eng.check_status()
            keep = min(cap, limit)
            for f, (kept, desc, n_raw) in enumerate(full):
                detect_equal(out, f, kept[:keep], desc[:keep], n_raw, sentinel=SENT)
                assert int(out[2][f]) == (0 if f in flat else keep)
    finally:
        eng.set_capacity(1 << 16, 1 << 20)
