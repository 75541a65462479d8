"""GPU tests of steered BRIEF and the scale pyramid past their list, level and capacity limits: csrc/k_pyramid.hip (k_pyr_down,
k_pyr_append), csrc/k_steer.hip (orient_bin, k_steer_list, k_orient_list, k_steer_kept) and the pyramid's launch site in
csrc/pgx_api.hip (pyr_plan, pgx_prepare_detect, enqueue_detect_bins, pgx_pyramid_level).  Every comparison is exact and
against the numpy restatements tests/pyramid_ref.py and tests/steered_ref.py (which rest on the C oracle): keypoint fields
by bit pattern, descriptors, bins, origin, stats, counts and nraw, the sentinel rows behind every list, and the status raised
or not raised.  The device is never its own reference, and every scene's precondition is an assert on the restatements alone
(tests/test_scale_limits_cases.py).  The statements below are quoted from the sources; that file holds them to the text.

  branch (file: statement)                            one side (earlier tests, or the case)      other side (the case here)
  --------------------------------------------------  -----------------------------------------  ---------------------------------------
  -- pgx_api.hip
  pyr_plan: `while (p.n_run < p.n_levels &&           test_gpu_pyramid: n_run == n_levels, or    ladder[161 x 140, 8 levels, step 131072]
    p.dims[p.n_run][0] > 0) p.n_run++`                n_run == 1                                 n_run 4; [step 104858] n_run 5;
                                                                                                 [40 x 35, step 131072] n_run 2
  pgx_prepare_detect: `if (pl.n_run > 2) ...          n_run 3 and 8: allocated                   ladder[40 x 35]: n_run 2 of 8, ws_pyr_b
    ws_pyr_b.ensure(...)`                                                                        never needed by a fresh context
  enqueue_detect_bins: `dst = (l & 1) ? ws_pyr_a :    3 levels: a, b                             ladder n_run 4 and 5: a, b, a(, b), every
    ws_pyr_b`, the ping-pong over `l < pl.n_run`                                                 level checked through its keypoints
  enqueue_detect_bins: `kp_soft = c->kp_cap <= cap`,  limit 50 below cap 1024                    limits[1, 3, 50, 63, 65] x cap above (soft:
    `kp_eff = kp_soft ? c->kp_cap : cap`                                                         no error), 2 * limit (soft, list too
                                                                                                 long: error) and limit - 1 (hard: error)
  enqueue_detect_bins: the level chains' out_stride   F = 3                                      nine[F = 9]: pgx_xcd_map's two branches
    = kp_eff, level 0's = cap                                                                    with stride kp_eff != cap; fused[F = 9]
  pgx_launch_dewarp_gray in front of the levels       16-bit sources, no map                     ingest: RGBA8 behind a dewarp map, 3 levels
  -- k_pyramid.hip, k_pyr_append
  totals: `nj = j < m.n_run ? lvl_counts[...] : 0`    j < n_run throughout                       ladder: stats rows j >= n_run are 0, not
                                                                                                 what ws_pyr_cnt held before
  `nv = n < cap - base ? n : cap - base; nv -= k0;    one cut, wherever totals[1] falls          sweep[n0 + 1, n0 + 63, n0 + 65, total - 1]:
    if (nv <= 0) return; if (nv > 64) nv = 64`                                                   0 < nv < 64, the cut inside a workgroup;
                                                                                                 [n0 + 64, n0 + 128]: nv == 0 at k0 = 64,
                                                                                                 128; [n0, n0 + n1]: base == cap; every cap
                                                                                                 below n0 + n1: cap - base < 0 at level 2;
                                                                                                 [n0 - 1, 1]: level 0 alone over the cap;
                                                                                                 [total]: no cut; three: three regimes in
                                                                                                 one call
  stats: `room = cap - total;                         room > 0, one room <= 0                    sweep: room > 0, == 0 ([n0, n0 + n1]: 0
    nj < room ? nj : (room > 0 ? room : 0)`                                                      entries), < 0 (every level behind the cut)
  `if (total > cap) atomicOr(status, KP_CAP)`         raised, and total == cap not               sweep: raised exactly when cap < total
  `n = lvl_counts[l * F + f]`, `base`                 every level of every frame has entries     nine: pixels (n = 0 with base > 0 from level
                                                                                                 1 on), bumps (base = 0 at l >= 1), flat (no
                                                                                                 entry anywhere) among ordinary frames
  `f = f0 + blockIdx.z`, `dst0 = f * cap + base + k0`  F = 3                                     nine: F = 9, special frames at 3, 7 and 8
  `src0 = ((l - 1) * F + f) * tmp_stride + k0`        tmp_stride = cap or 50                     limits: tmp_stride 1, 3, 63, 65 (grid.x 1
                                                                                                 and 2, the second workgroup one entry)
  `if (bins) bins[dst0 + tid] = tmp_bins[...]`        steered, 3 levels                          every pyramid case again steered (R = 31,
                                                                                                 B = 64), bins requested and not
  -- k_pyramid.hip, k_pyr_down
  `if (x4 + 3 < Wd && (o & 15) == 0)` with            F = 1 (pgx_pyramid_level): the row alone   ladder[104858] F = 3 and nine[104858] F = 9:
    `o = dst + (blockIdx.z * Hd + y) * Wd + x4`       decides                                    38 x 33 levels, odd frames start 8 bytes
                                                                                                 off; 62 x 54: odd rows do
  pyr_tap: `q = ((2 * x + 1) * step - 65536) >> 1`,   sizes up to 1030                           strips[65535 x 17, 17 x 65535, 65534 x 16,
    `i0 < n_src - 1`, in long long                                                               65535 x h16, h16 x 65535] at steps 69632,
                                                                                                 100000, 131072: x up to 61679, y likewise
  grid `(Wd + 255) / 256, (Hd + 3) / 4`               up to 5 x 18 workgroups                    strips: 241 workgroups a row; 15420 rows of
                                                                                                 workgroups (grid.y)
  -- k_steer.hip
  orient_bin: `for (r0 = -R; r0 <= R; r0 +=           R in 1, 2, 7, 15, 31: 3, 5 or 7 live rows  radii[4, 8, 28]: ONE live row in the last
    ROWS_AHEAD)`, `dy * dy <= rem`                    in the last group                          group; last_row[R]: that row's one pixel
                                                                                                 alone decides the bin; [30]: 5 live rows
  orient_bin: `dx = lane - R`, `rem >= 0`             R = 31: one idle lane                      radii[30]: three idle lanes; [4]: 55
  orient_bin: `xs < (uint32_t)W`, `ys < (uint32_t)H`  orient alone outside the image; images     outside: the steered DESCRIPTOR at points on,
                                                      larger than the disc                       just outside and 2^30 outside the image;
                                                                                                 small[16 x 16, 7 x 40, 40 x 7] x R 31, 15:
                                                                                                 every pixel, the disc wider or higher than
                                                                                                 the image; ladder steered: the 20 x 17
                                                                                                 level under R = 31
  `P == PGX_PLAN_PAIRS ? k_steer_list<true> : <false>`  P 33, 256, 320                           tables[255, 257]: both sides of the plan
                                                                                                 switch; [1]: one pair
  `pairs_rot + (size_t)bin * P`                       bin * P below 64 * 320                     tables[4064] B = 64: 4 MB of turned pairs,
                                                                                                 bin 63 among the keypoints' (the largest
                                                                                                 offset), >= 16 distinct directions
  k_steer_kept: `pgx_xcd_map(blockIdx.x, (kp_cap + 3)  F = 9 with a limit of 2048, every frame   fused[F = 9, limit 3 and 50]: lists cut by a
    / 4, nframes, f, kb)`, `k >= nk`,                 textured                                   limit that is no multiple of 4 (ragged last
    `if (kb == 0 && threadIdx.x == 0)                                                            block), frames 3 and 8 flat: counts 0
      counts_out[f] = nk`                                                                        written, no row touched; cap above the limit

Not tested: more than 65535 frames in one call.  The slice loops of pgx_launch_pyr_down and pgx_launch_pyr_append
(`for (f0 = 0; f0 < F; f0 += 65535)`) run once in every case here, as everywhere else in the suite.  For kp_cap = 1 there is no
capacity below the limit: a caller's cap of 0 is PGX_E_BADARG, and that is what the case asserts.

Steps 100000 and 131072 turn the 17-pixel side of the first three strips into fewer than 16 pixels, so those strips have
level 0 alone there (asserted: the first empty level is refused); the strips of side h16(step) -- 25 and 32 -- are the thinnest that
still have a level 1, so that the long axis is resampled at every step."""
import numpy as np
import pytest
import torch

import front_limits_cases as fc
import photogrammetry_amd as pg
import pyramid_ref as pr
import scale_limits_cases as sc
import steered_ref as sr
from match_gpu import DEV
from photogrammetry_amd._lib import PGX_E_BADARG
from pyramid_gpu import buffers, host, run

pytestmark = pytest.mark.gpu
STEER = (sc.STEER_B, sc.STEER_R)


@pytest.fixture(scope="module")
def eng():
    e = pg.Engine(0)          # a context of its own: the modes set here stay out of the shared one
    yield e
    e.close()


def _configure(eng, P, steer, n_levels, step, kp_cap=1 << 20):
    """the engine in the state sc.reference(..., P, steer) restates"""
    eng.set_source_format(pg.api.PGX_SRC_RGBA64)
    eng.set_detect_params(sc.T, sc.RADIUS)
    eng.set_capacity(1 << 16, kp_cap)
    eng.set_dewarp_map(None)
    eng.set_brief_pairs(sc.tables(P)[0])                     # turns steering off
    if steer:
        _, rot, dirs = sc.tables(P, steer[0])
        eng.set_brief_steering(rot, dirs, steer[1])
    eng.set_pyramid(n_levels, step)


def _reset(eng):
    eng.set_brief_steering(None)
    eng.set_capacity(1 << 16, 1 << 20)
    eng.set_pyramid(1, pr.STEP_MAX)


def _entries(eng, frames, ref, cap, words, n_levels, steered, expect=None):
    """the merged lists through pgx_detect_batch_pyramid_dev (bins asked for in steered mode), the plain entry and, steered, the
    steered entry"""
    got = run(eng, frames, cap, words, n_levels, bins=steered, expect=expect)
    sc.check_lists(got, ref, cap, bins=steered)
    if not steered:
        assert (got["bins"] == sc.SENT).all()
    plain = run(eng, frames, cap, words, n_levels, entry="plain", expect=expect)
    sc.check_lists(plain, ref, cap, origin=False)
    assert (plain["bins"] == sc.SENT).all() and (plain["origin"] == sc.SENT).all() and (plain["stats"] == sc.SENT).all()
    if steered:
        sc.check_lists(run(eng, frames, cap, words, n_levels, entry="steered", expect=expect), ref, cap, origin=False, bins=True)
        no_bins = run(eng, frames, cap, words, n_levels, expect=expect)      # steered descriptors, d_bins = NULL
        sc.check_lists(no_bins, ref, cap)
        assert (no_bins["bins"] == sc.SENT).all()
    return got


# ---- the pyramid ---------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("steered", [False, True])
@pytest.mark.parametrize("P", [256, 33])
@pytest.mark.parametrize("w,h,n_levels,step,n_run", sc.LADDERS)
def test_partly_empty_ladder(eng, w, h, n_levels, step, n_run, P, steered):
    cap, words = 1024, (P + 31) // 32
    steer = STEER if steered else None
    ref = [sc.reference("ordinary", f, n_levels, step, P, steer, w=w, h=h) for f in range(3)]
    assert all(r["total"] < cap for r in ref)
    _configure(eng, P, steer, n_levels, step)
    got = _entries(eng, sc.frames(3, w, h), ref, cap, words, n_levels, steered)
    assert (got["stats"][:, n_run:] == 0).all() and (got["stats"][:, :min(n_run, 3), 0] > 0).all()
    assert set(np.unique(got["origin"][..., 0])) == set(range(n_run)) | {sc.SENT}
    _reset(eng)


def _sweep(steered):
    n_levels, step = sc.SWEEP
    P, steer = (33, STEER) if steered else (256, None)
    r = sc.reference("ordinary", sc.SWEEP_FRAME, n_levels, step, P, steer)
    return P, steer, r, sc.sweep_caps(int(r["stats"][0, 0]), int(r["stats"][1, 0]), r["total"])


@pytest.mark.parametrize("steered", [False, True])
@pytest.mark.parametrize("which", range(11), ids=["n0-1", "n0", "n0+1", "n0+63", "n0+64", "n0+65", "n0+128", "n0+n1", "total-1",
                                                  "total", "one"])
def test_capacity_sweep(eng, which, steered):
    n_levels, step = sc.SWEEP
    P, steer, full, caps = _sweep(steered)
    cap = caps[which]
    ref = [sc.reference("ordinary", sc.SWEEP_FRAME, n_levels, step, P, steer, capacity=cap)]
    assert ref[0]["count"] == min(cap, full["total"]) and ref[0]["total"] == full["total"]
    _configure(eng, P, steer, n_levels, step)
    frame = sc.frames(3)[sc.SWEEP_FRAME:sc.SWEEP_FRAME + 1]
    _entries(eng, frame, ref, cap, (P + 31) // 32, n_levels, steered, expect=pg.CapacityError if cap < full["total"] else None)
    _reset(eng)


@pytest.mark.parametrize("steered", [False, True])
def test_three_cut_regimes_in_one_call(eng, steered):
    n_levels, step = sc.SWEEP
    P, steer = (33, STEER) if steered else (256, None)
    full = [sc.reference("ordinary", f, n_levels, step, P, steer) for f in range(3)]
    cap = sc.three_regime_cap([r["stats"][0, 0] for r in full])
    assert sorted(sc.cut_regime(r["stats"][:, 0].tolist(), cap)[0] for r in full) == ["inside", "level0", "level_boundary"]
    ref = [sc.reference("ordinary", f, n_levels, step, P, steer, capacity=cap) for f in range(3)]
    _configure(eng, P, steer, n_levels, step)
    got = _entries(eng, sc.frames(3), ref, cap, (P + 31) // 32, n_levels, steered, expect=pg.CapacityError)
    assert got["counts"].tolist() == [cap] * 3
    _reset(eng)


@pytest.mark.parametrize("steered", [False, True])
@pytest.mark.parametrize("n_levels,step", [sc.ONE_SIDED, sc.NINE_OTHER])
def test_one_sided_frames_among_ordinary_ones(eng, n_levels, step, steered):
    cap, P = 512, 256
    steer = STEER if steered else None
    ref = [sc.reference("one_sided", f, n_levels, step, P, steer) for f in range(sc.ONE_SIDED_F)]
    assert all(r["total"] < cap for r in ref)
    _configure(eng, P, steer, n_levels, step)
    got = _entries(eng, sc.one_sided_batch(), ref, cap, 8, n_levels, steered)
    at = sc.ONE_SIDED_AT
    assert got["counts"][at["flat"]] == 0 and got["nraw"][at["flat"]] == 0 and (got["stats"][at["flat"]] == 0).all()
    assert got["stats"][at["bumps"], 0, 0] == 0 and got["counts"][at["bumps"]] > 0
    if (n_levels, step) == sc.ONE_SIDED:
        assert got["counts"][at["pixels"]] == got["stats"][at["pixels"], 0, 0] > 30
    _reset(eng)


@pytest.mark.parametrize("steered", [False, True])
@pytest.mark.parametrize("kp_cap", sc.KP_CAPS)
def test_survivor_limits(eng, kp_cap, steered):
    n_levels, step = sc.LIMITS
    P, steer = (33, STEER) if steered else (256, None)
    words, frames = (P + 31) // 32, sc.frames(3)
    _configure(eng, P, steer, n_levels, step, kp_cap=kp_cap)
    for cap, expect in ((3 * kp_cap + 5, None), (2 * kp_cap, pg.CapacityError), (kp_cap - 1, pg.CapacityError)):
        if cap == 0:                                         # no capacity lies below a limit of 1: 0 is refused, nothing written
            b = buffers(3, 1, words, n_levels)
            d_frames = torch.from_numpy(frames).to(DEV)
            torch.cuda.synchronize()
            with pytest.raises(pg.PgxError) as ex:
                eng.detect_batch_pyramid_dev(d_frames, 3, sc.W, sc.H, b["kp"], b["desc"], b["counts"], b["nraw"], 0, b["origin"],
                                             b["stats"])
            assert ex.value.code == PGX_E_BADARG
            eng.check_status()
            assert all((v == sc.SENT).all() for v in host(b).values())
            continue
        ref = [sc.reference("ordinary", f, n_levels, step, P, steer, kp_cap=kp_cap, capacity=cap) for f in range(3)]
        assert all((r["total"] > cap) == (expect is not None) for r in ref)
        _entries(eng, frames, ref, cap, words, n_levels, steered, expect=expect)
    _reset(eng)


@pytest.mark.parametrize("step", sc.STRIP_STEPS)
def test_resampler_at_the_size_limit(eng, step):
    eng.set_pyramid(8, step)
    went_down = 0
    for i, (w, h) in enumerate(sc.strip_shapes(step)):
        g = sc.strip(w, h, 40 + i)
        for l, e in enumerate(pr.levels(g, 8, step)):
            if e is None:
                with pytest.raises(pg.PgxError) as ex:       # an empty level has no image
                    eng.pyramid_level(g, l)
                assert ex.value.code == PGX_E_BADARG
                break
            got = eng.pyramid_level(g, l)
            assert got.shape == e.shape and got.dtype == np.float32
            assert (got.view(np.uint32) == e.view(np.uint32)).all(), (w, h, step, l)
            went_down += l > 0
    assert went_down == 2                                    # one wide and one tall strip have a level 1
    eng.set_pyramid(1, step)


def test_pyramid_behind_a_dewarp_map_and_an_8_bit_source(eng):
    n_levels, step = sc.INGEST
    frames8, _, dmap = sc.ingest_scene()
    ref = [sc.ingest_reference(f) for f in range(3)]
    cap = 1024
    assert all(r["total"] < cap for r in ref)
    _configure(eng, 256, None, n_levels, step)
    try:
        eng.set_source_format(pg.api.PGX_SRC_RGBA8)
        eng.set_dewarp_map(dmap)
        _entries(eng, frames8, ref, cap, 8, n_levels, False)
    finally:
        eng.set_source_format(pg.api.PGX_SRC_RGBA64)
        eng.set_dewarp_map(None)
        _reset(eng)


# ---- steering ------------------------------------------------------------------------------------------------------------------------------

def _set(eng, P, B, R):
    pairs, rot, dirs = sc.steer_tables(P, B)
    eng.set_pyramid(1, pr.STEP_MAX)
    eng.set_brief_pairs(pairs)
    eng.set_brief_steering(rot, dirs, R)
    return rot, dirs


def _check_list(eng, g, xy, rot, dirs, R):
    eb, ed = sr.describe(g, xy, rot, dirs, R)
    k = sc.kps(xy, pg.KEYPOINT_DTYPE)
    gb, gd = eng.orient(g, k), eng.brief(g, k)
    assert gb.dtype == np.int32 and gb.tolist() == eb.tolist()
    assert gd.shape == ed.shape and (gd == ed).all()
    return eb, ed


@pytest.mark.parametrize("P", [256, 33])
@pytest.mark.parametrize("B", [4, 64])
@pytest.mark.parametrize("R", sc.RADII)
def test_radii_with_a_short_last_row_group(eng, R, B, P):
    rot, dirs = _set(eng, P, B, R)
    eb, ed = _check_list(eng, sc.image(), sc.points(sc.W, sc.H, R), rot, dirs, R)
    assert len(np.unique(eb)) >= 3 and ed.any()
    g, c = sc.last_row_image(R)                              # the one pixel of the row dy = R decides
    eb, _ = _check_list(eng, g, c, rot, dirs, R)
    assert eb.tolist() == [B // 4]
    eng.set_brief_steering(None)


@pytest.mark.parametrize("P", [256, 70])
@pytest.mark.parametrize("R,B", [(15, 32), (31, 64)])
def test_descriptors_of_keypoints_outside_the_image(eng, R, B, P):
    rot, dirs = _set(eng, P, B, R)
    pts, _ = fc.outside_points(sc.W, sc.H)
    _, ed = _check_list(eng, sc.image(), pts, rot, dirs, R)
    assert ed.any(axis=1).sum() >= 8 and (~ed.any(axis=1)).sum() >= 6
    eng.set_brief_steering(None)


@pytest.mark.parametrize("R", [31, 15])
@pytest.mark.parametrize("w,h", sc.SMALL)
def test_images_smaller_than_the_disc(eng, w, h, R):
    rot, dirs = _set(eng, 256, 64, R)
    eb, _ = _check_list(eng, sc.image(w, h, 3), sc.every_pixel(w, h), rot, dirs, R)
    assert len(eb) == w * h and len(np.unique(eb)) >= 8
    eng.set_brief_steering(None)


@pytest.mark.parametrize("P", sc.TABLE_P)
def test_table_sizes_and_the_largest_offset(eng, P):
    rot, dirs = _set(eng, P, 64, 15)
    g = sc.rays_image()
    xy, b = sc.direction_points(g, dirs, 15)
    assert len(np.unique(b)) >= 16 and 63 in b
    eb, _ = _check_list(eng, g, xy, rot, dirs, 15)
    assert eb.tolist() == b.tolist()
    eng.set_brief_steering(None)


@pytest.mark.parametrize("P", [256, 33])
@pytest.mark.parametrize("kp_cap", [3, 50])
def test_fused_form_cut_by_a_survivor_limit(eng, kp_cap, P):
    F, cap, words = 9, kp_cap + 6, (P + 31) // 32
    ref = [sc.fused_reference(f, P, kp_cap) for f in range(F)]
    assert [r["count"] for r in ref] == [0 if f in (3, 8) else kp_cap for f in range(F)]
    _configure(eng, P, (sc.FUSED_B, sc.FUSED_R), 1, pr.STEP_MAX, kp_cap=kp_cap)
    got = run(eng, sc.fused_batch(), cap, words, 1, entry="steered")
    sc.check_lists(got, ref, cap, origin=False, bins=True)
    assert got["counts"].tolist() == [r["count"] for r in ref] and (got["origin"] == sc.SENT).all()
    plain = run(eng, sc.fused_batch(), cap, words, 1, entry="plain")     # the plain call with the mode on: no bins
    sc.check_lists(plain, ref, cap, origin=False)
    assert (plain["bins"] == sc.SENT).all()
    _reset(eng)
