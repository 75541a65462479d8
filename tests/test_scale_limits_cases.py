"""The scenes of tests/scale_limits_cases.py are what tests/test_gpu_scale_limits.py takes them for (no GPU): the restated launch
rules equal the text of csrc/k_pyramid.hip, csrc/k_steer.hip and csrc/pgx_api.hip, and every scene reaches the side of the
constant it is named for -- asserted on the restatements (tests/pyramid_ref.py, tests/steered_ref.py) alone, so that a scene
that stops exercising its limit fails here first."""
import os

import numpy as np
import pytest

import front_limits_cases as fc
import pyramid_ref as pr
import scale_limits_cases as sc
import steered_ref as sr
from oracle import cref
import photogrammetry_amd as pg

CSRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "photogrammetry_amd", "csrc")


def source(name):
    return open(os.path.join(CSRC, name)).read()


# ---- the mirrored launch facts -----------------------------------------------------------------------------------------------------

def test_constants_and_rules_equal_the_kernel_sources():
    pyr = source("k_pyramid.hip")
    for line in ("const int f = f0 + (int)blockIdx.z, l = blockIdx.y, k0 = (int)blockIdx.x * %d, tid = threadIdx.x;" % sc.APPEND_WG,
                 "for (int j = 0; j < l; j++) base += lvl_counts[j * F + f];",
                 "int nv = n < cap - base ? n : cap - base;", "nv -= k0;", "if (nv <= 0) return;", "if (nv > %d) nv = %d;" % (sc.APPEND_WG, sc.APPEND_WG),
                 "const int room = cap - total;", "nj < room ? nj : (room > 0 ? room : 0);",
                 "const int nj = j < m.n_run ? lvl_counts[j * F + f] : 0, rj = j < m.n_run ? lvl_nraw[j * F + f] : 0;",
                 "counts[f] = total < cap ? total : cap;", "if (total > cap) atomicOr(status, (int)PGX_ST_KP_CAP);",
                 "dim3((tmp_stride + %d) / %d, n_run, nf), dim3(256)" % (sc.APPEND_WG - 1, sc.APPEND_WG),
                 "const int y = (int)blockIdx.y * %d + wv;" % sc.DOWN_ROWS,
                 "const int x4 = ((int)blockIdx.x * 64 + (int)(threadIdx.x & 63)) * %d;" % sc.DOWN_PX,
                 "dim3((Wd + %d) / %d, (Hd + %d) / %d, nf), dim3(%d)" % (sc.DOWN_NT - 1, sc.DOWN_NT, sc.DOWN_ROWS - 1, sc.DOWN_ROWS, sc.DOWN_NT),
                 "float *o = dst + ((size_t)blockIdx.z * Hd + y) * Wd + x4;",
                 "if (x4 + 3 < Wd && (reinterpret_cast<uintptr_t>(o) & 15) == 0) {",
                 "const long long q = (((long long)(2 * x + 1) * step) - 65536) >> 1;"):
        assert line in pyr, line
    assert sc.DOWN_NT == 64 * sc.DOWN_PX and sc.DOWN_NT // 64 == sc.DOWN_ROWS      # a wave is 256 pixels of one row; four waves
    steer = source("k_steer.hip")
    for line in ("constexpr int ROWS_AHEAD = %d;" % sc.ROWS_AHEAD, "for (int r0 = -R; r0 <= R; r0 += ROWS_AHEAD) {",
                 "const int dx = lane - R, R2 = R * R;", "const bool in = col_in && dy * dy <= rem && ys < (uint32_t)H;",
                 "pgx_xcd_map(blockIdx.x, (kp_cap + 3) / 4, nframes, f, kb);", "if (kb == 0 && threadIdx.x == 0) counts_out[f] = nk;",
                 "pairs_rot + (size_t)bin * P, P, words", "P == PGX_PLAN_PAIRS ? k_steer_list<true> : k_steer_list<false>",
                 "P == PGX_PLAN_PAIRS ? k_steer_kept<true> : k_steer_kept<false>"):
        assert line in steer, line
    api = source("pgx_api.hip")
    for line in ("while (p.n_run < p.n_levels && p.dims[p.n_run][0] > 0) p.n_run++;", "const bool kp_soft = c->kp_cap <= cap;",
                 "const int kp_eff = kp_soft ? c->kp_cap : cap;", "float *dst = (l & 1) ? c->ws_pyr_a.as<float>() : c->ws_pyr_b.as<float>();",
                 "if (pl.n_run > 2) HIPCHK(c, c->ws_pyr_b.ensure((size_t)F * pl.dims[2][0] * pl.dims[2][1] * 4));",
                 "lvl_nraw, F, kp_eff, c->words, pl.n_levels, pl.n_run, W, H, pl.scale, d_kp, d_desc, d_bins,",
                 "lvl_nraw + (size_t)l * F, kp_eff, tmp_bins ? tmp_bins + (l - 1) * lvl_slots : nullptr);"):
        assert line in api, line
    assert "#define PGX_PLAN_PAIRS %d" % fc.P_PLAN in source("pgx_brief_plan.h") or "PGX_PLAN_PAIRS = %d" % fc.P_PLAN in source("pgx_brief_plan.h")
    assert "if (w < %d || h < %d) empty = true;" % (sc.MIN_SIDE, sc.MIN_SIDE) in source("pgx_hostutil.cpp")
    assert pr.dims(32, 31, 2, 131072)[0].tolist() == [[32, 31], [0, 0]] and pr.dims(32, 32, 2, 131072)[0][1].tolist() == [16, 16]


def test_append_map_and_room_clamp_restated():
    counts, cap = [132, 182, 160], 260                       # the cut falls in level 1 at 128: on a 64-entry boundary
    g = sc.append_groups(counts, cap, 256)
    assert len(g) == 3 * 4 and g[0] == (0, 0, 132) and g[2] == (0, 128, 4) and g[3] == (0, 192, -60)
    assert [nv for l, k0, nv in g if l == 1] == [128, 64, 0, -64] and all(nv < 0 for l, k0, nv in g if l == 2)
    st, count, rooms = sc.append_stats(counts, 8, cap)
    assert st == [132, 128, 0, 0, 0, 0, 0, 0] and count == 260 and rooms[:4] == [260, 128, -54, -214]
    assert sc.append_stats(counts, 3, 314) == ([132, 182, 0], 314, [314, 182, 0])
    assert sc.cut_regime(counts, 260) == ("wg_boundary", True) and sc.cut_regime(counts, 314) == ("level_boundary", False)
    assert sc.cut_regime(counts, 131) == ("level0", True) and sc.cut_regime(counts, 132) == ("level_boundary", True)
    assert sc.cut_regime(counts, 473) == ("inside", False) and sc.cut_regime(counts, 474) == ("fits", False)
    assert sc.cut_regime(counts, 200, kp_cap=50) == ("fits", False) and sc.kp_limits(50, 200) == (50, True) and sc.kp_limits(50, 49) == (49, False)
    # the sum of what the workgroups copy is the list's length, whatever the cap
    for cap in (1, 131, 132, 133, 196, 260, 314, 400, 473, 474, 1000):
        eff = sc.level_counts(counts, cap)
        moved = sum(min(max(nv, 0), 64) for _, _, nv in sc.append_groups(eff, cap, min(cap, 256)))
        assert moved == min(sum(counts), cap) == sc.append_stats(eff, 3, cap)[1] == sum(sc.append_stats(eff, 3, cap)[0])


def test_orient_row_groups():
    live = {R: sc.orient_groups(R)[-1][1] for R in (1, 2, 7, 15, 31) + sc.RADII}
    assert [live[R] for R in (1, 2, 7, 15, 31)] == [3, 5, 7, 7, 7]          # what the first tests reach (the issue's 3, 5 or 7)
    assert live[4] == live[8] == live[28] == 1 and live[30] == 5            # R = 4k: a single live row in the last group
    assert sc.idle_lanes(31) == 1 and sc.idle_lanes(30) == 3 and sc.idle_lanes(4) == 55
    for R in range(1, 32):
        g = sc.orient_groups(R)
        assert sum(n for _, n in g) == 2 * R + 1 and all(n == sc.ROWS_AHEAD for _, n in g[:-1]) and (g[-1][1] == 1) == (R % 4 == 0)


# ---- the pyramid's scenes -------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("w,h,n_levels,step,n_run", sc.LADDERS)
def test_partly_empty_ladders(w, h, n_levels, step, n_run):
    assert sc.n_run(w, h, n_levels, step) == n_run and 1 < n_run < n_levels
    assert (n_run > 2) == ((w, h) == (sc.W, sc.H))           # ws_pyr_b is allocated for the first two ladders only
    d, _ = pr.dims(w, h, n_levels, step)
    if step == 131072 and w == sc.W:
        assert d[:4].tolist() == [[161, 140], [80, 70], [40, 35], [20, 17]]
        assert sc.reference("ordinary", 0, n_levels, step, 256)["stats"][:, 0].tolist() == [132, 111, 35, 8, 0, 0, 0, 0]
        assert d[3, 0] < 2 * sc.STEER_R + 1 and d[3, 1] < sc.STEER_R           # the steered disc is larger than the last level
    for P in (256, 33):
        for steer in (None, (sc.STEER_B, sc.STEER_R)):
            for f in range(3):
                r = sc.reference("ordinary", f, n_levels, step, P, steer, w=w, h=h)
                assert (r["stats"][:min(n_run, 3), 0] > 0).all() and (r["stats"][n_run:] == 0).all() and r["count"] == r["total"]
                if steer:
                    assert len(np.unique(r["bins"])) >= (8 if w == sc.W else 3)
    # the store paths of the level images: at step 2.0 every width here is a multiple of 4 (16-byte stores alone); the 104858
    # ladder has rows that start off 16 bytes (62 columns) and a level whose frames do (38 x 33 = 1254 pixels)
    paths = [sc.store_paths(3, *d[l]) for l in range(1, n_run)]
    if step == 131072:
        assert all(p == {"vector"} for p in paths) and (d[1:n_run, 0] % 4 == 0).all()
    else:
        assert d[1:5].tolist() == [[100, 87], [62, 54], [38, 33], [23, 20]]
        assert paths[0] == {"vector"} and all(p == {"vector", "scalar"} for p in paths[1:])
        assert [sc.down_store(f, 0, 0, 38, 33) for f in range(4)] == ["vector", "scalar", "vector", "scalar"]
        assert [sc.down_store(0, y, 0, 62, 54) for y in range(4)] == ["vector", "scalar", "vector", "scalar"]
        assert {sc.down_store(f, 0, 0, 38, 33) for f in (7, 8)} == {"vector", "scalar"}     # and in the nine-frame call's tail


def test_capacity_sweep_hits_every_regime():
    n_levels, step = sc.SWEEP
    r = sc.reference("ordinary", sc.SWEEP_FRAME, n_levels, step, 256)
    surv = r["stats"][:, 0].tolist()
    n0, n1, total = surv[0], surv[1], r["total"]
    assert (surv[:3] > np.int64(0)).all() and n1 > 128 and sum(surv) == total and sc.n_run(sc.W, sc.H, n_levels, step) == 8
    caps = sc.sweep_caps(n0, n1, total)
    assert caps[-1] == 1 and len(set(caps)) == 11 and n0 + 128 < n0 + n1
    regimes = [sc.cut_regime(surv, c) for c in caps]
    assert regimes == [("level0", True), ("level_boundary", True), ("inside", True), ("inside", True), ("wg_boundary", True),
                       ("inside", True), ("wg_boundary", True), ("level_boundary", True), ("inside", False), ("fits", False),
                       ("level0", True)]
    for cap in caps:
        c = sc.reference("ordinary", sc.SWEEP_FRAME, n_levels, step, 256, capacity=cap)
        assert c["count"] == min(total, cap) and c["total"] == total and c["nraw"] == r["nraw"]
        eff = sc.level_counts(surv, sc.kp_limits(1 << 20, cap)[0])
        st, count, rooms = sc.append_stats(eff, n_levels, cap)
        assert st == c["stats"][:, 0].tolist() and count == c["count"]       # the restated clamp is the restatement's rule
        regime, behind = regimes[caps.index(cap)]
        assert {int(np.sign(x)) for x in rooms} == ({1, 0, -1} if regime in ("level0", "level_boundary") else {1, -1} if behind
                                                    else {1}), cap
        if regime == "wg_boundary":                           # the workgroup that starts at the cut has nothing left: nv == 0
            assert (1, cap - n0, 0) in sc.append_groups(eff, cap, cap) and (1, cap - n0 - 64, 64) in sc.append_groups(eff, cap, cap)
    # three frames, one capacity, three regimes
    refs = [sc.reference("ordinary", f, n_levels, step, 256) for f in range(3)]
    cap = sc.three_regime_cap([x["stats"][0, 0] for x in refs])
    got = sorted(sc.cut_regime(x["stats"][:, 0].tolist(), cap)[0] for x in refs)
    assert got == ["inside", "level0", "level_boundary"] and all(x["total"] > cap for x in refs)


def test_one_sided_frames():
    n_levels, step = sc.ONE_SIDED
    at = sc.ONE_SIDED_AT
    assert sc.ONE_SIDED_F == 9 and {at["pixels"], at["flat"]} == {7, 8} and at["bumps"] % 8 not in (0, 7)
    assert sc.one_sided_batch().shape == (9, sc.H, sc.W, 4)
    for steer in (None, (sc.STEER_B, sc.STEER_R)):
        st = {k: sc.reference("one_sided", f, n_levels, step, 256, steer)["stats"] for k, f in at.items()}
        assert st["pixels"][0, 0] > 30 and (st["pixels"][1:] == 0).all()            # n = 0 with base > 0 at every later level
        assert (st["bumps"][0] == 0).all() and (st["bumps"][1:, 0] > 0).sum() >= 2  # base = 0 at l >= 1
        assert (st["flat"] == 0).all()
        for f in set(range(9)) - set(at.values()):
            assert (sc.reference("one_sided", f, n_levels, step, 256, steer)["stats"][:4, 0] > 0).all()
    # the nine frames are the block -> frame map's both branches
    nblk = 2
    assert sorted(fc.kept_map(lid, nblk, 9) for lid in range(nblk * 9)) == [(f, b) for f in range(9) for b in range(nblk)]
    assert fc.kept_map(nblk * 8, nblk, 9) == (8, 0) and fc.kept_map(7, nblk, 9) == (7, 0)
    # at step 2.0 every level is a multiple of 4 wide; the same nine frames at NINE_OTHER reach the scalar stores, by the row
    # and by the frame (asserted in test_partly_empty_ladders), and still hold frames with empty levels
    assert sc.NINE_OTHER == sc.LADDERS[1][2:4]
    st = {k: sc.reference("one_sided", f, *sc.NINE_OTHER, 256)["stats"] for k, f in at.items()}
    assert (st["flat"] == 0).all() and (st["bumps"][0] == 0).all() and st["bumps"][1:, 0].sum() > 0 and st["pixels"][0, 0] > 30


def test_survivor_limits_scene():
    n_levels, step = sc.LIMITS
    refs = [sc.reference("ordinary", f, n_levels, step, 256) for f in range(3)]
    assert all((r["stats"][:, 0] > 65).all() for r in refs) and max(sc.KP_CAPS) == 65
    assert {k % 4 for k in sc.KP_CAPS} >= {1, 2, 3} and min(sc.KP_CAPS) == 1 and {63, 65} <= set(sc.KP_CAPS)
    for kp_cap in sc.KP_CAPS:
        soft = [sc.reference("ordinary", f, n_levels, step, 256, kp_cap=kp_cap, capacity=3 * kp_cap + 5) for f in range(3)]
        assert all((r["stats"][:, 0] == kp_cap).all() and r["count"] == r["total"] == 3 * kp_cap for r in soft)
        assert sc.kp_limits(kp_cap, 3 * kp_cap + 5) == (kp_cap, True)
        over = [sc.reference("ordinary", f, n_levels, step, 256, kp_cap=kp_cap, capacity=2 * kp_cap) for f in range(3)]
        assert all(r["stats"][:, 0].tolist() == [kp_cap, kp_cap, 0] and r["total"] > r["count"] for r in over)   # soft, yet too long
        if kp_cap > 1:
            cap = kp_cap - 1
            hard = [sc.reference("ordinary", f, n_levels, step, 256, kp_cap=kp_cap, capacity=cap) for f in range(3)]
            assert sc.kp_limits(kp_cap, cap) == (cap, False)
            assert all(r["stats"][:, 0].tolist() == [cap, 0, 0] and r["count"] == cap for r in hard)
    assert (65 + sc.APPEND_WG - 1) // sc.APPEND_WG == 2 and (63 + sc.APPEND_WG - 1) // sc.APPEND_WG == 1   # k_pyr_append's grid.x


@pytest.mark.parametrize("step", sc.STRIP_STEPS)
def test_resampler_taps_at_the_size_limit(step):
    """pgx.h rule 3: q >= 0 and x0 <= W_{l-1} - 1 for the two extreme sizes and down every ladder the strips have"""
    for n_src in (16, 17, sc.h16(step), 65534, 65535):
        n = n_src
        while True:
            n_dst = (n * 65536) // step
            if n_dst < 1:
                break
            i0, i1, fr, q = pr.taps(n_dst, n, step)
            assert q.min() >= 0 and i0.max() <= n - 1 and i1.max() <= n - 1 and (i1 >= i0).all()
            assert (2 * (n_dst - 1) + 1) * step < 2 ** 63 and fr.min() >= 0 and fr.max() < 1
            if n_dst < sc.MIN_SIDE:
                break
            n = n_dst
    shapes = sc.strip_shapes(step)
    assert shapes[:3] == [(65535, 17), (17, 65535), (65534, 16)]
    with_level_1 = [s for s in shapes if sc.n_run(s[0], s[1], 8, step) >= 2]
    assert {max(s) for s in with_level_1} == {65535} and len(with_level_1) == 2     # one wide and one tall strip go down a level
    for w, h in with_level_1:
        d = pr.dims(w, h, 8, step)[0]
        assert min(d[1]) == 16 and sc.n_run(w, h, 8, step) == 2
        assert sc.down_grid(d[1, 0], d[1, 1], 1)[:2] in (((d[1, 0] + 255) // 256, 4), (1, (d[1, 1] + 3) // 4))
        assert w * h * 4 < 9 << 20                            # thin strips: under 9 MB each


def test_ingest_scene():
    n_levels, step = sc.INGEST
    frames8, wide, dmap = sc.ingest_scene()
    assert frames8.dtype == np.uint8 and (wide == frames8.astype(np.uint16) * 257).all() and len(frames8) == 3
    assert dmap[..., 0].min() >= 0 and dmap[..., 0].max() < sc.W and dmap[..., 1].min() >= 0 and dmap[..., 1].max() < sc.H
    ident = np.stack(np.meshgrid(np.arange(sc.W), np.arange(sc.H)), axis=2)
    assert (dmap != ident).any(axis=2).mean() > 0.3           # the map moves pixels
    for f in range(3):
        r = sc.ingest_reference(f)
        plain = pr.detect_pyramid(cref.gray(wide[f]), n_levels, step, sc.T, sc.RADIUS, sc.tables(256)[0])
        assert (r["stats"][:, 0] > 20).all() and r["kp"].tobytes() != plain["kp"].tobytes()


# ---- steering's scenes ------------------------------------------------------------------------------------------------------------------

def test_radii_scene():
    g = sc.image()
    for R in sc.RADII:
        xy = sc.points(sc.W, sc.H, R)
        for B in (4, 64):
            _, rot, dirs = sc.steer_tables(256, B)
            b = sr.bins(g, xy, dirs, R)
            assert len(np.unique(b)) >= 3
    # the last live row, dy = R, holds one pixel of the disc, (x, y + R): in last_row_image it alone is bright, and it alone
    # decides the direction -- a quarter turn with it, the flat patch's bin 0 without
    for R in sc.RADII:
        for B in (4, 64):
            _, rot, dirs = sc.steer_tables(256, B)
            g1, c = sc.last_row_image(R)
            assert sr.bins(g1, c, dirs, R).tolist() == [B // 4] and sr.moments(g1, c, R)[0].tolist() == [0]
            g0 = g1.copy()
            g0[c[0, 1] + R, c[0, 0]] = np.float32(0.37)
            assert sr.bins(g0, c, dirs, R).tolist() == [0]


def test_outside_and_small_scenes():
    pts, _ = fc.outside_points(sc.W, sc.H)
    g = sc.image()
    for R, B in [(15, 32), (31, 64)]:
        for P in (256, 70):
            _, rot, dirs = sc.steer_tables(P, B)
            b, d = sr.describe(g, pts, rot, dirs, R)
            dx = np.maximum(np.maximum(-pts[:, 0].astype(np.int64), pts[:, 0].astype(np.int64) - (sc.W - 1)), 0)
            dy = np.maximum(np.maximum(-pts[:, 1].astype(np.int64), pts[:, 1].astype(np.int64) - (sc.H - 1)), 0)
            outside = (dx > 0) | (dy > 0)
            near = outside & (dx <= 1) & (dy <= 1)
            assert near.sum() >= 4 and d[near].any(axis=1).all()            # just outside: some turned pairs still see the image
            assert not d[(dx > fc.REACH + 9) | (dy > fc.REACH + 9)].any()   # a turned offset is at most sqrt 2 * 20 long
            assert len(np.unique(b[~outside])) >= 2
    for w, h in sc.SMALL:
        for R in (31, 15):
            assert w < 2 * R + 1 or h < 2 * R + 1
            _, rot, dirs = sc.steer_tables(256, 64)
            b = sr.bins(sc.image(w, h, 3), sc.every_pixel(w, h), dirs, R)
            assert len(b) == w * h and len(np.unique(b)) >= 8
    assert min(w for w, h in sc.SMALL) == 7 and min(h for w, h in sc.SMALL) == 7 and (16, 16) in sc.SMALL


@pytest.mark.parametrize("P", sc.TABLE_P)
def test_tables_scene(P):
    assert {255, 257} <= set(sc.TABLE_P) and fc.P_PLAN == 256 and max(sc.TABLE_P) == fc.P_MAX and min(sc.TABLE_P) == 1
    _, rot, dirs = sc.steer_tables(P, 64)
    assert rot.shape == (64, P, 4) and (P < 4064 or rot.nbytes >= 4 * 10 ** 6)
    g = sc.rays_image()
    xy, b = sc.direction_points(g, dirs, 15)
    assert len(np.unique(b)) >= 16 and 63 in b and 0 in b
    _, d = sr.describe(g, xy, rot, dirs, 15)
    assert d.shape == (len(xy), (P + 31) // 32) and (P == 1 or d.any(axis=1).sum() >= len(xy) // 2)
    if P > 1:                                                 # the direction's own table matters: bin 63's is not bin 0's
        i = int(np.flatnonzero(b == 63)[0])
        assert (cref.brief(g, xy[i:i + 1], rot[0]) != d[i]).any() or P < 64


def test_fused_scene():
    frames = sc.fused_batch()
    assert frames.shape[0] == 9 and 9 % 8 == 1
    for kp_cap in (3, 50):
        assert kp_cap % 4 != 0
        for P in (256, 33):
            for f in range(9):
                r = sc.fused_reference(f, P, kp_cap)
                full = sc.fused_reference(f, P, None)
                if f in (3, 8):
                    assert r["count"] == 0 and r["nraw"] == 0
                else:
                    assert full["count"] > 50 and r["count"] == kp_cap and len(np.unique(full["bins"])) >= 8
