"""Scenes and CPU helpers of tests/test_gpu_scale_limits.py (no torch, no GPU): the launch rules of csrc/k_pyramid.hip
(k_pyr_append's workgroup -> (level, k0, nv) map with its capacity cut and the `room` clamp of its stats, k_pyr_down's grid
and its store path) and of csrc/k_steer.hip (orient_bin's row groups and idle lanes) restated, the frames and keypoint lists
the GPU tests run, and the exact comparisons they make.  tests/test_scale_limits_cases.py holds the restated rules to the
sources' text and asserts, on the restatements tests/pyramid_ref.py and tests/steered_ref.py alone, that every scene lies on
the side of the constant it is made for.  Also home of the keypoint list tests/test_gpu_steered.py shares with it.  A plain
helper module: no test module imports another."""
import functools

import numpy as np

import front_limits_cases as fc
import pyramid_ref as pr
import steered_ref as sr
from oracle import cref

# ---- the launch rules -----------------------------------------------------------------------------------------------------------------
APPEND_WG = 64                                    # k_pyr_append: entries of one level of one frame per workgroup
DOWN_PX, DOWN_NT, DOWN_ROWS = 4, 256, 4           # k_pyr_down: pixels per thread, threads per workgroup, rows (waves) per workgroup
ROWS_AHEAD = 8                                    # orient_bin: rows whose loads are issued together
MIN_SIDE = pr.MIN_SIDE                            # a level narrower or lower than this is empty
W, H, T, RADIUS = 161, 140, np.float32(0.1), 4    # the frame size and detect parameters of every scene but the strips
SENT = -7                                         # what the GPU tests fill their output buffers with


def n_run(w, h, n_levels, step):
    """pyr_plan: the levels that are not empty (level 0 always runs)"""
    d, _ = pr.dims(w, h, n_levels, step)
    n = 1
    while n < n_levels and d[n, 0] > 0:
        n += 1
    assert (d[n:] == 0).all()
    return n


def kp_limits(kp_cap, cap):
    """enqueue_detect_bins -> (kp_eff, kp_soft): the per-level limit and whether exceeding it is silent"""
    soft = kp_cap <= cap
    return (kp_cap if soft else cap), soft


def level_counts(survivors, kp_eff):
    """what the level chains leave in lvl_counts: every level's NMS survivors, cut to kp_eff"""
    return [min(int(n), kp_eff) for n in survivors]


def append_groups(counts, cap, stride):
    """k_pyr_append's grid for one frame -> [(level, k0, nv)] of EVERY workgroup, nv before the `nv <= 0` return and the
    clamp to 64 (so 0 and negative values show which workgroups leave at once).  counts: level_counts of the levels that run."""
    out, base = [], 0
    for l, n in enumerate(counts):
        for bx in range((stride + APPEND_WG - 1) // APPEND_WG):
            k0 = bx * APPEND_WG
            out.append((l, k0, min(n, cap - base) - k0))
        base += n
    return out


def append_stats(counts, n_levels, cap):
    """the `room` clamp of k_pyr_append's totals -> (entries per level IN the list [n_levels], count, rooms [n_levels]); the
    levels behind the ones that run count 0"""
    total, st, rooms = 0, [], []
    for j in range(n_levels):
        nj = counts[j] if j < len(counts) else 0
        room = cap - total
        rooms.append(room)
        st.append(nj if nj < room else max(room, 0))
        total += nj
    return st, min(total, cap), rooms


def cut_regime(survivors, cap, kp_cap=1 << 20):
    """Where the caller's capacity cuts the merged list of one frame -> (regime, a level lies wholly behind the cap):
    "fits" (no cut), "level0" (level 0 alone is over the cap), "level_boundary" (base == cap at a level with entries),
    "wg_boundary" (the cut falls on a 64-entry boundary inside a level: one workgroup gets nv == 0) or "inside" (inside a
    workgroup's 64 entries)."""
    counts = level_counts(survivors, kp_cap)      # the levels as pgx_set_capacity's limit alone leaves them
    if sum(counts) <= cap:
        return "fits", False
    if counts[0] > cap:
        return "level0", any(n > 0 for n in counts[1:])
    base = 0
    for l, n in enumerate(counts):
        if base + n > cap:
            rem = cap - base
            return (("level_boundary" if rem == 0 else "wg_boundary" if rem % APPEND_WG == 0 else "inside"),
                    any(m > 0 for m in counts[l + 1:]))
        base += n
    raise AssertionError("unreachable")


def down_grid(Wd, Hd, F):
    """pgx_launch_pyr_down's grid"""
    return (Wd + DOWN_NT - 1) // DOWN_NT, (Hd + DOWN_ROWS - 1) // DOWN_ROWS, F


def down_store(f, y, x4, Wd, Hd):
    """k_pyr_down's store of the four pixels from column x4 of row y of frame f (the buffer itself starts on a 16-byte
    boundary): "vector" (one 16-byte store) or "scalar" (the row tail, and rows that start off a 16-byte boundary)"""
    return "vector" if x4 + DOWN_PX - 1 < Wd and ((f * Hd + y) * Wd + x4) % 4 == 0 else "scalar"


def store_paths(F, Wd, Hd):
    """the store paths a level of F frames takes, as a set"""
    return {down_store(f, y, x4, Wd, Hd) for f in range(F) for y in range(Hd) for x4 in range(0, Wd, DOWN_PX)}


def orient_groups(R):
    """orient_bin's row groups -> [(r0, live rows)]: a row of the group is live while r0 + j <= R"""
    return [(r0, min(ROWS_AHEAD, R - r0 + 1)) for r0 in range(-R, R + 1, ROWS_AHEAD)]


def idle_lanes(R):
    """lanes of the wave that own no column of the disc"""
    return 64 - (2 * R + 1)


# ---- frames -----------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def frames(n, w=W, h=H):
    """the ordinary frames: the textured synthetic frames of tests/test_gpu_pyramid.py, seeds 1 .. n"""
    from photogrammetry_amd import synth
    return np.stack([synth.make_frame(w, h, seed=1 + i) for i in range(n)])


def frame_of_grey(g):
    """the RGBA64 frame with R = G = B = round(65535 g), A = 65535: its grey image is g to within 2^-17"""
    f = np.empty(g.shape + (4,), dtype=np.uint16)
    f[..., :3] = np.rint(np.clip(g, 0, 1) * 65535).astype(np.uint16)[..., None]
    f[..., 3] = 65535
    return f


def pixels_frame(w=W, h=H, seed=7):
    """isolated bright pixels (0.7) on a flat ground (0.4), one per cell of a 14 x 20 grid and at least 10 px apart: each is a
    FAST hit at level 0, and the 2 x 2 mean of the next level lifts its pixel by 0.075 < T only"""
    rng = np.random.default_rng(seed)
    g = np.full((h, w), 0.4)
    for cy in range(10, h - 10, 20):
        for cx in range(10, w - 10, 14):
            g[cy + rng.integers(-2, 3), cx + rng.integers(-2, 3)] = 0.7
    return frame_of_grey(g)


def bumps_frame(w=W, h=H, sigma=6.0, amp=0.5):
    """broad Gaussian bumps on a grid, far enough apart not to overlap: at level 0 the ring of radius 3 is less than T below the
    summit (amp * (1 - exp(-9 / (2 sigma^2))) = 0.06), at the half-size levels it is not"""
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    g = np.full((h, w), 0.2)
    for cy in range(24, h - 20, 46):
        for cx in range(26, w - 20, 54):
            g += amp * np.exp(-((x - cx) ** 2 + (y - cy) ** 2) / (2 * sigma * sigma))
    return frame_of_grey(g)


def flat_frame(w=W, h=H):
    return fc.flat_frame(w, h)


ONE_SIDED_F = 9
ONE_SIDED_AT = {"bumps": 3, "pixels": 7, "flat": 8}     # frames 7 and 8: the F % 8 tail of the block -> frame map


@functools.lru_cache(maxsize=None)
def one_sided_batch():
    """nine frames: six ordinary ones and the three one-sided ones at ONE_SIDED_AT"""
    special = {"bumps": bumps_frame(), "pixels": pixels_frame(), "flat": flat_frame()}
    at = {i: k for k, i in ONE_SIDED_AT.items()}
    ordinary = iter(frames(ONE_SIDED_F - len(at)))
    return np.stack([special[at[i]] if i in at else next(ordinary) for i in range(ONE_SIDED_F)])


@functools.lru_cache(maxsize=None)
def fused_batch():
    """nine frames for the fused steered form: ordinary ones, frame 3 and the last one flat"""
    b = frames(9).copy()
    b[3], b[8] = flat_frame(), flat_frame()
    return b


# ---- the pyramid's configurations -------------------------------------------------------------------------------------------------------
LADDERS = [(W, H, 8, 131072, 4), (W, H, 8, 104858, 5), (40, 35, 8, 131072, 2)]     # (w, h, n_levels, step, n_run)
ONE_SIDED = (8, 131072)
NINE_OTHER = (8, 104858)                          # the nine frames again where the store path depends on the row and the frame
SWEEP = (8, 78643)                                # at least three contributing levels, more than 128 survivors at level 1
SWEEP_FRAME = 0
LIMITS = (3, 78643)                               # every level of frames 0 .. 2 has more than 65 survivors
KP_CAPS = (1, 3, 50, 63, 65)
INGEST = (3, 92682)
STEER_R, STEER_B = 31, 64                         # the steered pyramid cases: a disc larger than the 20 x 17 level


@functools.lru_cache(maxsize=None)
def tables(P, B=32):
    import photogrammetry_amd as pg
    pairs = pg.make_brief_pairs(3, 8, P)
    rot, dirs = pg.make_steering(pairs, B)
    return pairs, rot, dirs


@functools.lru_cache(maxsize=None)
def grey_of(batch, f, w=W, h=H):
    """grey image of frame f of a named batch ("ordinary", "one_sided", "fused")"""
    src = {"ordinary": lambda: frames(max(f + 1, 3), w, h), "one_sided": one_sided_batch, "fused": fused_batch}[batch]()
    return cref.gray(src[f])


@functools.lru_cache(maxsize=None)
def reference(batch, f, n_levels, step, P, steer=None, capacity=None, kp_cap=None, w=W, h=H):
    """pyramid_ref.detect_pyramid of frame f of a named batch, computed once and left unchanged.  steer: None or (B, R)."""
    st = None
    if steer is not None:
        _, rot, dirs = tables(P, steer[0])
        st = (rot, dirs, steer[1])
    return pr.detect_pyramid(grey_of(batch, f, w, h), n_levels, step, T, RADIUS, tables(P)[0], capacity=capacity, kp_cap=kp_cap,
                             steer=st)


FUSED_B, FUSED_R = 32, 15


@functools.lru_cache(maxsize=None)
def fused_reference(f, P, kp_cap):
    """frame f of fused_batch through the single-scale steered chain, cut to the survivor limit kp_cap (None: none)"""
    return reference("fused", f, 1, pr.STEP_MAX, P, (FUSED_B, FUSED_R), kp_cap=kp_cap)


@functools.lru_cache(maxsize=None)
def ingest_scene():
    """-> (frames8 uint8 [3][H][W][4], the same frames widened x257 as the oracle sees them, a mild dewarp map): the pyramid
    behind an 8-bit source and a dewarp map"""
    frames8 = (frames(3) // 257).astype(np.uint8)
    return frames8, frames8.astype(np.uint16) * 257, cref.build_distortion_matrix(W, H, [3e-4, 1e-7, 0, 0, 0])


@functools.lru_cache(maxsize=None)
def ingest_reference(f):
    _, wide, dmap = ingest_scene()
    return pr.detect_pyramid(cref.gray(cref.apply_distortion(wide[f], dmap)), INGEST[0], INGEST[1], T, RADIUS, tables(256)[0])


def sweep_caps(n0, n1, total):
    """the capacities of the sweep, in the issue's order"""
    return [n0 - 1, n0, n0 + 1, n0 + 63, n0 + 64, n0 + 65, n0 + 128, n0 + n1, total - 1, total, 1]


def three_regime_cap(n0s):
    """a capacity that cuts three frames in three different ways: the median of their level-0 counts (level 0 over it, the
    cut on the level boundary, the cut inside level 1)"""
    return int(sorted(n0s)[1])


# ---- the resampler at the size limit ------------------------------------------------------------------------------------------------------
STRIP_STEPS = (69632, 100000, 131072)


def h16(step):
    """the smallest side whose next level has exactly MIN_SIDE pixels"""
    return -(-MIN_SIDE * step // 65536)


def strip_shapes(step):
    """(w, h) of the thin strips: the three of the issue, and the two at the size limit whose short side is just long enough
    for a level 1 at this step (17 is, at 69632 only)"""
    return [(65535, 17), (17, 65535), (65534, 16)] + ([(65535, h16(step)), (h16(step), 65535)] if h16(step) != 17 else [])


def strip(w, h, seed):
    """random float32 grey made from 16-bit values (no intermediate of rule 3 is subnormal)"""
    return (np.random.default_rng(seed).integers(0, 65536, (h, w)) / 65535).astype(np.float32)


# ---- steering -----------------------------------------------------------------------------------------------------------------------------
RADII = (4, 8, 28, 30)
SMALL = [(16, 16), (7, 40), (40, 7)]              # (w, h): narrower or lower than the disc of R = 15 and of R = 31
TABLE_P = (1, 255, 257, 4064)


@functools.lru_cache(maxsize=None)
def steer_tables(P, B):
    """a random pair table of reach 20 (front_limits_cases.table) and its B turned copies -> (pairs, pairs_rot, dirs)"""
    import photogrammetry_amd as pg
    pairs = fc.table(P)
    rot, dirs = pg.make_steering(pairs, B)
    return pairs, rot, dirs


def points(w, h, R):
    """The four corners, the edge mid-points, points R - 1, R and R + 1 from each border, interior points."""
    pts = [(0, 0), (w - 1, 0), (0, h - 1), (w - 1, h - 1), (w // 2, 0), (w // 2, h - 1), (0, h // 2), (w - 1, h // 2)]
    for d in (R - 1, R, R + 1):
        pts += [(d, h // 2 + 3), (w - 1 - d, h // 2 - 3), (w // 2 + 3, d), (w // 2 - 3, h - 1 - d), (d, d), (w - 1 - d, h - 1 - d)]
    pts += [(w // 2, h // 2), (40, 37), (101, 90), (77, 50), (33, 99)]
    return np.array(pts, np.int32)


def last_row_image(R, w=W, h=H, cx=80, cy=70):
    """-> (noise with a flat disc of radius R around (cx, cy) and ONE bright pixel in the disc's last row, at (cx, cy + R); the
    keypoint int32 [1][2]): m10 = 0 and m01 = R * 65535 * 0.63, so the bin is a quarter turn"""
    g = np.random.default_rng(R).random((h, w)).astype(np.float32)
    y, x = np.mgrid[0:h, 0:w]
    g[(x - cx) ** 2 + (y - cy) ** 2 <= R * R] = np.float32(0.37)
    g[cy + R, cx] = 1.0
    return np.ascontiguousarray(g), np.array([(cx, cy)], np.int32)


def every_pixel(w, h):
    y, x = np.mgrid[0:h, 0:w]
    return np.stack([x.reshape(-1), y.reshape(-1)], axis=1).astype(np.int32)


@functools.lru_cache(maxsize=None)
def image(w=W, h=H, seed=1):
    """Smooth ground (a clear centroid) plus noise (descriptor bits that depend on the exact samples), float32 in [0, 1]."""
    noise = np.random.default_rng(seed).random((h, w)).astype(np.float32)
    return np.ascontiguousarray((np.float32(0.6) * sr.smooth_image(w, h, seed + 1) + np.float32(0.4) * noise).astype(np.float32))


def direction_points(g, dirs, R, step=3):
    """keypoints of a grid over the image, the first one met of every direction bin -> (points int32 [n][2], their bins)"""
    h, w = g.shape
    cand = np.array([(x, y) for y in range(0, h, step) for x in range(0, w, step)], np.int32)
    b = sr.bins(g, cand, dirs, R)
    _, first = np.unique(b, return_index=True)
    first.sort()
    return cand[first], b[first]


def rays_image(w=W, h=H, cx=80, cy=70):
    """brightness falling off linearly from (cx, cy): around that centre the centroid of a disc points at it, so the grid of
    direction_points meets every direction"""
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    g = 1.0 - np.hypot(x - cx, y - cy) / np.hypot(w, h)
    noise = np.random.default_rng(5).random((h, w))
    return np.ascontiguousarray((0.9 * g + 0.1 * noise).astype(np.float32))


def kps(xy, dtype):
    k = np.zeros(len(xy), dtype=dtype)
    if len(xy):
        k["x"], k["y"] = np.asarray(xy)[:, 0], np.asarray(xy)[:, 1]
    return k


# ---- comparisons ----------------------------------------------------------------------------------------------------------------------------
def check_lists(got, ref, cap, origin=True, bins=False, sent=SENT):
    """The merged lists of every frame (host arrays kp [F][cap][4], desc, counts, nraw, origin, stats, bins as int32) against
    the restatement's, every field exact; the rows behind a list untouched."""
    for f, r in enumerate(ref):
        n = r["count"]
        assert int(got["counts"][f]) == n and int(got["nraw"][f]) == r["nraw"], (f, got["counts"][f], n, got["nraw"][f], r["nraw"])
        assert (got["kp"][f, :n] == r["kp"].view(np.int32).reshape(-1, 4)).all(), f   # x, y, fast_score and the bits of value
        assert (got["desc"][f, :n].view(np.uint32) == r["desc"]).all(), f
        assert (got["kp"][f, n:] == sent).all() and (got["desc"][f, n:] == sent).all(), f
        if origin:
            assert (got["origin"][f, :n] == r["origin"]).all() and (got["origin"][f, n:] == sent).all(), f
            assert (got["stats"][f] == r["stats"]).all(), (f, got["stats"][f].tolist(), r["stats"].tolist())
        if bins:
            assert (got["bins"][f, :n] == r["bins"]).all() and (got["bins"][f, n:] == sent).all(), f
