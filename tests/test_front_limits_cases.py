"""The scenes of tests/front_limits_cases.py are what tests/test_gpu_front_limits.py takes them for (no GPU): the restated launch rules equal the text of csrc/k_fast.hip,
csrc/k_image.hip, csrc/k_brief.hip and csrc/k_brief_core.inc, and every scene reaches the side of the constant it is named
for -- asserted on the oracle alone, so that a scene that stops exercising its limit fails here first."""
import os
import re

import numpy as np
import pytest

import front_limits_cases as fc
import steered_ref as sr
from oracle import cref
import photogrammetry_amd as pg

CSRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "photogrammetry_amd", "csrc")


def source(name):
    return open(os.path.join(CSRC, name)).read()


# ---- the mirrored launch facts -----------------------------------------------------------------------------------------------------

def test_constants_and_rules_equal_the_kernel_sources():
    fast = source("k_fast.hip")
    assert "constexpr int TW = %d, TH = %d, HALO = %d;" % (fc.TW, fc.TH, fc.HALO) in fast
    assert "__shared__ uint16_t queue[TW * TH];" in fast and "hv[k] = (rowok && lane < 2 * HALO && hx < W) ? grow[hx] : 0.0f;" in fast
    assert "for (int base = 0; base < nseg; base += 1024 * 4) {" in fast and fc.SCAN_PASS == 4096
    assert "if (i0 + 3 < nseg && (nseg & 3) == 0) {" in fast and "if (tid == 1023) carry_s = run;" in fast
    assert "if (pos >= (uint32_t)raw_cap) break;" in fast and "const int code = score - 11; // 1..5" in fast
    assert "size_t pgx_fast_seg_count(int W, int H) { return (size_t)H * ((W + TW - 1) / TW); }" in fast
    img = source("k_image.hip")
    assert "constexpr int FB = %d;" % fc.FB in img and "dim3 grid(gx, (unsigned)((F + FB - 1) / FB)), block(%d);" % fc.DG_NT in img
    assert "const unsigned cap = %du / ny > %du ? %du / ny : %du;" % (fc.DG_WG, fc.DG_MIN_WG, fc.DG_WG, fc.DG_MIN_WG) in img
    assert "const bool vec = (npix & 3) == 0 || F == 1;" in img and "if (vec && i0 + 3 < npix) {" in img
    api = source("pgx_api.hip")
    assert 'if (!pairs || P <= 0 || P > %d) return fail(c, PGX_E_BADARG, "P must be in [1, 4064]");' % fc.P_MAX in api
    assert "const int kp_eff = kp_soft ? c->kp_cap : cap;" in api
    assert "enqueue_from_gray(c, gray, F, W, H, kp_eff, kp_soft, d_kp, d_desc, d_counts, d_nraw, cap, d_bins);" in api
    brief = source("k_brief.hip")
    for line in ("const int nblk = (kp_cap + 3) / 4;", "const int F8 = (nframes / 8) * 8;", "if (Lid < nblk * F8) {", "const int j = Lid >> 3;",
                 "f = (j / nblk) * 8 + (Lid & 7);", "kb = j % nblk;", "const int r = Lid - nblk * F8;", "f = F8 + r / nblk;", "kb = r % nblk;",
                 "if (kb == 0 && threadIdx.x == 0) counts_out[f] = nk;", "const int k = blockIdx.x * 4 + wv;"):
        assert line in brief, line
    assert "P == PGX_PLAN_PAIRS ? k_brief_kept<true> : k_brief_kept<false>" in brief
    core = source("k_brief_core.inc")
    assert "const int nchunk = (P + 63) / 64;" in core and "const int off = P - 64 * (c + 1);" in core
    assert "#define PGX_PLAN_PAIRS %d" % fc.P_PLAN in source("pgx_brief_plan.h") or "PGX_PLAN_PAIRS = %d" % fc.P_PLAN in source("pgx_brief_plan.h")
    # which radii run k_fast_compact in the chain: every one outside the champion rounds
    nms = source("k_nms.hip")
    assert "{ return radius >= 0 && nms_layout(W, H, radius, n_cap, true).champ != 0; }" in nms


# ---- the grey patterns ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("w,h", fc.SCAN_SHAPES + fc.SATURATED_SHAPES + [(70, 2100), (65, 33)])
def test_dense_makes_every_interior_pixel_a_hit_of_score_16(w, h):
    hits = cref.detect(fc.dense(w, h), fc.T_DENSE)
    assert len(hits) == (w - 6) * (h - 6) and set(hits["fast_score"].tolist()) == {16}
    assert hits["x"].min() == 3 and hits["x"].max() == w - 4 and hits["y"].min() == 3 and hits["y"].max() == h - 4
    # the same pattern as a frame: its grey image gives the same hits
    assert fc.same_hits(cref.detect(cref.gray(fc.dense_frame(w, h)), fc.T_DENSE), hits) is None


@pytest.mark.parametrize("w,h", fc.SCAN_SHAPES + [(67, 35), (129, 65)])
def test_noise4_has_all_five_scores(w, h):
    g, T = fc.fast_scene("noise4", w, h)
    hits = cref.detect(g, T)
    assert set(hits["fast_score"].tolist()) == {12, 13, 14, 15, 16}
    assert 0.05 < len(hits) / (w * h) < 0.25
    # the batch's threshold finds the same hits: the levels are 1/3 apart
    fc.same_hits(cref.detect(g, fc.T_DENSE), hits)


def test_scan_shapes_cross_the_pass_and_the_load_switch():
    facts = [(fc.nseg(w, h), fc.scan_passes(w, h), fc.scan_load(w, h)) for w, h in fc.SCAN_SHAPES + fc.SCAN_BEYOND]
    assert facts == [(4096, 1, "vector"), (4097, 2, "scalar"), (8193, 3, "scalar"), (4098, 2, "scalar"), (4100, 2, "vector"),
                     (4103, 2, "scalar"), (4106, 2, "scalar"), (4108, 2, "vector")]
    assert fc.nseg(128, 2049) & 3 == 2
    # what the first parity tests reach: one pass
    assert max(fc.nseg(w, h) for w, h in [(451, 383), (200, 131), (83, 60)]) == 3064 < fc.SCAN_PASS
    for w, h in fc.SCAN_SHAPES + fc.SCAN_BEYOND:
        for kind in ("dense", "noise4"):
            g, T = fc.fast_scene(kind, w, h)
            hits = cref.detect(g, T)
            beyond = (fc.segment_of(hits, w) >= fc.SCAN_PASS).sum()
            # hits behind the first pass get their offsets through the carry; without any, the carry still makes n_raw
            assert (beyond > 0) == ((w, h) in fc.SCAN_BEYOND + [(63, 8193)])
            if (w, h) in fc.SCAN_BEYOND:
                assert beyond > 10
            assert len(hits) - beyond > 1000


def test_saturated_tile():
    w, h = 192, 70
    hits = cref.detect(fc.dense(w, h), fc.T_DENSE)
    tile = (hits["x"] // fc.TW == 1) & (hits["y"] // fc.TH == 1)
    assert tile.sum() == fc.TW * fc.TH == 2048                               # the queue is full to its last entry
    seg, cnt = np.unique(fc.segment_of(hits[tile], w), return_counts=True)
    assert len(seg) == fc.TH and (cnt == 64).all()                           # all 64 bits of each of the 32 segments
    assert np.bincount(fc.segment_of(cref.detect(fc.dense(128, 64), fc.T_DENSE), 128)).max() == 61   # no full segment here


def test_edge_shapes_put_hits_on_both_sides_of_both_tile_edges():
    xs, ys = {"dense": set(), "noise4": set()}, {"dense": set(), "noise4": set()}
    for w in fc.EDGE_W:
        for h in fc.EDGE_H:
            for kind in ("dense", "noise4"):
                g, T = fc.fast_scene(kind, w, h)
                hits = cref.detect(g, T)
                xs[kind] |= set(hits["x"].tolist())
                ys[kind] |= set(hits["y"].tolist())
                if kind == "dense":
                    assert len(hits) == max(w - 6, 0) * max(h - 6, 0)
    for kind in ("dense", "noise4"):
        assert set(range(60, 67)) <= xs[kind] and set(range(28, 35)) <= ys[kind]
        assert set(range(124, 128)) <= xs[kind] and {60, 61} <= ys[kind]     # the second tile edge: x = 128 needs W >= 132
    # widths at which the six halo lanes end inside the image's last three columns, and the second tile's
    assert {66, 67, 69} <= set(fc.EDGE_W) and {127, 128, 129, 131} <= set(fc.EDGE_W)
    assert {fc.TH - 1, fc.TH, fc.TH + 1, fc.TH + fc.HALO, fc.TH + 2 * fc.HALO, 2 * fc.TH, 2 * fc.TH + 1} <= set(fc.EDGE_H)


def test_nonfinite_frame_has_hits_on_nan_centres():
    g = fc.nonfinite()
    assert g.shape == (40, 70)
    for frac in (np.isnan(g).mean(), np.isposinf(g).mean(), np.isneginf(g).mean()):
        assert 0.015 < frac < 0.05
    hits = cref.detect(g, fc.T_NOISE)
    on_nan = np.isnan(hits["value"])
    assert len(hits) > 500 and on_nan.sum() > 50 and np.isinf(hits["value"]).sum() > 50
    assert set(hits["fast_score"].tolist()) == {12, 13, 14, 15, 16}


def test_capacities_cut_inside_a_segment_and_at_a_boundary():
    for g, T, w in ((fc.dense(192, 70), fc.T_DENSE, 192), (fc.noise4(129, 65, 1), fc.T_NOISE, 129)):
        hits = cref.detect(g, T)
        seg = fc.segment_of(hits, w)
        n, n1, b, b1, one, zero = fc.capacities(hits, w)
        assert (n, n1, one, zero) == (len(hits), len(hits) - 1, 1, 0) and 1 < b < n - 1
        assert seg[b - 1] != seg[b]                        # cut at a boundary: the last entry kept ends a segment
        assert seg[b] == seg[b + 1]                        # one more: the cut falls inside the segment that follows
        assert seg[n - 2] == seg[n - 1]                    # n - 1 cuts inside the last segment
    hits = cref.detect(fc.dense(192, 70), fc.T_DENSE)
    assert fc.capacities(hits, 192)[2] == 64 * 93          # 32 rows of 61 + 64 + 61 hits: a segment boundary at a multiple of 64


# ---- the batched FAST cases ----------------------------------------------------------------------------------------------------------

def test_compact_batch_frames():
    pairs = cref.gaussian_pairs(1, 50, 256)
    assert fc.nseg(65, 33) == 66 and (66 * 4) % 16 != 0 and fc.scan_load(65, 33) == "scalar"   # frame 1's offsets: 8 bytes off
    assert fc.scan_passes(64, 4097) == 2
    frames = fc.compact_batch(65, 33)
    for f, frame in enumerate(frames):
        exp = fc.keep_all_detect(frame, pairs, fc.T_DENSE)
        assert exp[2] == len(exp[0]) and (exp[2] == 59 * 27 if f == 1 else exp[2] > 150)
        for radius in (-1, 0):                             # the restated keep-all chain IS the oracle chain at these radii
            ref = fc.oracle_chain(frame, None, pairs, fc.T_DENSE, radius, 1 << 20)
            assert not fc.lists_differ(exp, ref)
    # and on a slice of the tall frames, long enough for every score and thousands of ties
    for frame in fc.compact_batch(64, 4097)[:, 1000:1090]:
        exp = fc.keep_all_detect(frame, pairs, fc.T_DENSE)
        assert exp[2] > 700 and not fc.lists_differ(exp, fc.oracle_chain(frame, None, pairs, fc.T_DENSE, -1, 1 << 20))
    for frame in fc.tail_batch(64, 4103):                  # the cheap tall case: most hits behind the first pass, and some before it
        hits = cref.detect(cref.gray(frame), fc.T_DENSE)
        seg = fc.segment_of(hits, 64)
        assert (seg >= fc.SCAN_PASS).sum() > 30 and 0 < (seg < fc.SCAN_PASS).sum() and len(hits) < 2500
        assert not fc.lists_differ(fc.keep_all_detect(frame, pairs, fc.T_DENSE), fc.oracle_chain(frame, None, pairs, fc.T_DENSE, 0, 1 << 20))
    tall = fc.compact_batch(64, 4097)
    n = [len(cref.detect(cref.gray(f), fc.T_DENSE)) for f in tall]
    assert n[1] == 58 * 4091 and min(n) > 20000 and max(n) < 1 << 18


# ---- dewarp-grey ----------------------------------------------------------------------------------------------------------------------

def test_dewarp_grids():
    # host forms, one frame: the stride loop starts above 512 * 256 * 4 pixels
    assert fc.dewarp_grid(1, 524288)[3] == 1
    assert fc.dewarp_grid(1, 1024 * 513) == (512, 1, 1, 2, "vector") and 1024 * 513 == 525312
    assert fc.dewarp_grid(1, 1023 * 513) == (512, 1, 1, 2, "vector") and (1023 * 513) % 4 == 3   # a scalar tail in pass 2
    assert fc.dewarp_grid(1, 451 * 383)[3] == 1                                                # the largest before: one pass
    # batches: 16 frame groups, 32 workgroups each, two passes; last group of one frame | of four
    assert fc.dewarp_grid(61, 200 * 170) == (32, 16, 1, 2, "vector") and fc.dewarp_grid(64, 200 * 170) == (32, 16, 4, 2, "vector")
    assert fc.dewarp_grid(61, 201 * 171) == (32, 16, 1, 2, "scalar") and fc.dewarp_grid(64, 201 * 171) == (32, 16, 4, 2, "scalar")


@pytest.mark.parametrize("src8", [0, 1])
@pytest.mark.parametrize("w,h", fc.BAD_SHAPES)
def test_every_spoiled_map_entry_changes_a_compared_list(w, h, src8):
    frames, dmap, pairs = fc.bad_scene(w, h, src8)
    assert dmap[..., 0].min() >= 0 and dmap[..., 0].max() < w and dmap[..., 1].min() >= 0 and dmap[..., 1].max() < h
    if src8:
        assert ((frames // 257) * 257 == frames).all()
    entries = fc.bad_entries(w, h)
    assert entries[1] == (w - 1, h - 1) and (entries[1][1] * w + entries[1][0]) // 4 == (w * h - 1) // 4
    bad = fc.bad_map(dmap, entries)
    for x, y in entries:                                   # out of range after the (ushort) cast, each in its own way
        u, v = int(bad[y, x, 0]) & 0xFFFF, int(bad[y, x, 1]) & 0xFFFF
        assert u >= w or v >= h
    with pytest.raises(cref.OracleError):
        cref.apply_distortion(frames[0], bad)
    good = [fc.oracle_chain(frames[f], dmap, pairs, fc.BAD_T, fc.BAD_RADIUS, fc.BAD_CAP) for f in fc.BAD_CHECKED]
    assert all(len(g[0]) > 100 for g in good)
    assert not fc.lists_differ(good[0], fc.zeroed_detect(frames[0], dmap, [], pairs, fc.BAD_T, fc.BAD_RADIUS, fc.BAD_CAP))
    for e in entries:
        assert any(fc.lists_differ(g, fc.zeroed_detect(frames[f], dmap, [e], pairs, fc.BAD_T, fc.BAD_RADIUS, fc.BAD_CAP))
                   for f, g in zip(fc.BAD_CHECKED, good)), e


# ---- BRIEF ----------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("P", [256, 70])
def test_outside_points(P):
    w, h = 83, 60
    g = fc.noise4(w, h, 4)
    pts, far = fc.outside_points(w, h)
    pairs = fc.table(P, seed=fc.OUTSIDE_SEED)
    assert np.abs(pairs).max() == fc.REACH
    assert np.abs(pts.astype(np.int64)).max() + fc.REACH < 2 ** 31      # the oracle's C addition stays defined
    d = cref.brief(g, pts, pairs)
    assert far.sum() >= 6 and (~far).sum() >= 8
    assert not d[far].any()                                            # no sample can land inside
    for p in ((-1, -1), (w, h), (-1, h // 2), (w // 2, h)):            # just outside: some pairs still see the image
        i = np.flatnonzero((pts == p).all(axis=1))[0]
        assert not far[i] and d[i].any(), p
    on_reach = [np.flatnonzero((pts == p).all(axis=1))[0] for p in ((w + fc.REACH - 1, 10), (10, -fc.REACH))]
    assert not far[on_reach].any()                                     # exactly at the reach: a sample on the border column / row


def test_table_sizes():
    assert max(fc.TABLE_P) == fc.P_MAX and {31, 32, 63, 64, 65} <= set(fc.TABLE_P)
    words = {P: (P + 31) // 32 for P in fc.TABLE_P}
    assert words[4064] == 127 and words[4033] == 127 and words[32] == 1 and words[65] == 3
    last_off = {P: P - 64 * ((P + 63) // 64) for P in fc.TABLE_P}
    assert last_off[4064] == -32 and last_off[64] == 0 and last_off[31] == -33 and last_off[65] == -63
    w, h = 83, 60
    g = fc.noise4(w, h, 6)
    pts = fc.table_points(w, h)
    assert len(pts) == 9 and (0, 0) in map(tuple, pts) and (w - 1, h - 1) in map(tuple, pts)
    for P in fc.TABLE_P:
        d = cref.brief(g, pts, fc.table(P))
        assert d.shape == (9, words[P]) and d.any(axis=1).sum() >= 7
        if P % 32:
            assert (d[:, -1] >> (P % 32) == 0).all()       # the bits above P - 1 of the top word stay clear
    assert fc.KP_PER_WG == 4 and {3, 4, 5, 8, 9} <= set(fc.LIST_N)


@pytest.mark.parametrize("F", fc.MAP_F)
def test_block_to_frame_map_scene(F):
    nblk = (7 + 3) // 4
    assert nblk == 2 and (5 + 3) // 4 == 2 and 7 % 4 == 3  # a ragged last block at both survivor limits
    got = [fc.kept_map(lid, nblk, F) for lid in range(nblk * F)]
    assert sorted(got) == [(f, b) for f in range(F) for b in range(nblk)]
    F8 = F // 8 * 8
    assert (F8 > 0) == (F >= 8) and (F8 < F) == (F % 8 != 0)                  # which branches F takes
    # a remainder branch that dealt the frames round-robin, f = F8 + r % (F - F8), would still reach every (frame, block) where
    # the remainder's frame count and nblk are coprime (7 and 2) or the remainder is one frame; 10 is there for it
    wrong = {(F8 + (lid - nblk * F8) % (F - F8), (lid - nblk * F8) % nblk) for lid in range(nblk * F8, nblk * F)}
    assert (len(wrong) < nblk * (F - F8)) == (F == 10)
    frames, flat = fc.map_frames(F)
    assert flat == ([3] if F < 9 else [3, F - 1]) and 3 % 8 == 3               # frame 3: in the middle of a group of eight
    for P in (256, 100):
        pairs = cref.gaussian_pairs(3, 8, P)
        for f in (0, 3, 4, F - 1):
            kept, desc, n_raw = fc.oracle_chain(frames[f], None, pairs, fc.T_NOISE, 3, 1 << 20)
            assert (len(kept) == 0 and n_raw == 0) if f in flat else len(kept) >= 10


# ---- steered BRIEF -----------------------------------------------------------------------------------------------------------------------

def test_half_plane_reaches_the_top_of_the_packed_key():
    w, h, R, B = 161, 140, 31, 64
    _, dirs = pg.make_steering(fc.table(256), B)
    c = np.array([(80, 70)], np.int32)
    top = 0
    for turns in range(4):
        g = fc.half_plane(w, h, 80, 70, turns)
        s = sr.scores(g, c, dirs, R)[0]
        m10, m01 = sr.moments(g, c, R)
        assert abs(int(m10[0])) == abs(int(m01[0])) > 2 ** 29 and abs(int(m10[0])) < 2 ** 31
        assert 2 ** 44 < int(np.abs(s).max()) < 2 ** 46
        assert sr.unique_maximum(s[None])[0]
        top = max(top, int(np.abs(s).max()))
    assert top > 2 ** 44
