"""Scenes and CPU helpers of tests/test_gpu_front_limits.py (and of two cases of tests/test_gpu_steered.py)
(no torch, no GPU): the launch rules of csrc/k_fast.hip, csrc/k_image.hip and csrc/k_brief.hip restated
(tests/test_front_limits_cases.py holds them to the sources' text), the grey patterns and frames the GPU tests run, and the
comparison with the oracle's lists.  Every scene is made to put one input on each side of one constant of a kernel; that it
does so is asserted in tests/test_front_limits_cases.py, on the oracle alone.  A plain helper module: no test module imports
another."""
import numpy as np

from oracle import cref

# ---- the launch rules ---------------------------------------------------------------------------------------------------------------
TW, TH, HALO = 64, 32, 3                          # k_fast.hip: the LDS tile and its halo
SCAN_PASS = 1024 * 4                              # k_seg_scan: segments per pass (1024 threads, four each)
FB, DG_WG, DG_MIN_WG, DG_NT = 4, 512, 32, 256     # k_image.hip: frames per thread, the two grid caps, the workgroup
P_MAX, P_PLAN, CHUNK, KP_PER_WG = 4064, 256, 64, 4   # pgx_set_brief_pairs' limit, brief_256's P, pairs per ballot, waves per workgroup


def nseg(w, h):
    """pgx_fast_seg_count: 64-pixel row segments of a frame, in (y, tx) order = raster order"""
    return h * ((w + TW - 1) // TW)


def scan_passes(w, h):
    return (nseg(w, h) + SCAN_PASS - 1) // SCAN_PASS


def scan_load(w, h):
    """k_seg_scan's load of a thread's four counts: "vector" (one 16-byte load) where nseg is a multiple of 4"""
    return "vector" if nseg(w, h) % 4 == 0 else "scalar"


def dewarp_grid(F, npix):
    """pgx_launch_dewarp_gray -> (workgroups per frame group, frame groups, frames in the last group, passes of the stride
    loop, path): path "vector" where every frame's base is 16-byte aligned (or there is one frame), else "scalar"; with one
    frame the last partial group of four pixels is scalar on the vector path too"""
    ngroups = (npix + 3) // 4
    ny = (F + FB - 1) // FB
    cap = max(DG_WG // ny, DG_MIN_WG)
    gx = min((ngroups + DG_NT - 1) // DG_NT, cap)
    passes = (ngroups + gx * DG_NT - 1) // (gx * DG_NT)
    return gx, ny, F - (ny - 1) * FB, passes, ("vector" if npix % 4 == 0 or F == 1 else "scalar")


def kept_map(lid, nblk, F):
    """k_brief_kept's block -> (frame, keypoint block) map, its inline copy of pgx_xcd_map"""
    F8 = (F // 8) * 8
    if lid < nblk * F8:
        j = lid >> 3
        return (j // nblk) * 8 + (lid & 7), j % nblk
    r = lid - nblk * F8
    return F8 + r // nblk, r % nblk


# ---- grey patterns ------------------------------------------------------------------------------------------------------------------
T_DENSE, T_NOISE = np.float32(0.05), np.float32(0.1)


def dense_levels(w, h):
    y, x = np.mgrid[0:h, 0:w]
    return (x + 4 * y) % 16


def dense(w, h):
    """((x + 4 y) mod 16) / 15: every one of the sixteen ring offsets changes the residue, so with T = 0.05 every pixel 3 px
    from the border is a hit of score 16 -- (w - 6)(h - 6) of them, 64 in every interior segment"""
    return np.ascontiguousarray((dense_levels(w, h) / 15).astype(np.float32))


def noise4_levels(w, h, seed):
    return np.random.default_rng(seed).integers(0, 4, (h, w))


def noise4(w, h, seed):
    """four grey levels at random: about one pixel in seven is a hit, of every score 12 .. 16 (the three score planes)"""
    return np.ascontiguousarray((noise4_levels(w, h, seed) / 3).astype(np.float32))


def rgba_of_levels(levels, top):
    """the RGBA64 frame whose grey image is levels / top: R = G = B = level * (65535 / top) (top divides 65535), A = 65535"""
    assert 65535 % top == 0
    f = np.empty(levels.shape + (4,), dtype=np.uint16)
    f[..., :3] = (levels * (65535 // top)).astype(np.uint16)[..., None]
    f[..., 3] = 65535
    return f


def dense_frame(w, h):
    return rgba_of_levels(dense_levels(w, h), 15)


def noise4_frame(w, h, seed):
    return rgba_of_levels(noise4_levels(w, h, seed), 3)


def flat_frame(w, h):
    f = np.full((h, w, 4), 16384, dtype=np.uint16)
    f[..., 3] = 65535
    return f


def nonfinite(w=70, h=40, seed=5):
    """random float32 with NaN, +inf and -inf sprinkled in, 3 % each"""
    rng = np.random.default_rng(seed)
    g = rng.random((h, w)).astype(np.float32)
    u = rng.random((h, w))
    g[u < 0.03] = np.nan
    g[(u >= 0.03) & (u < 0.06)] = np.inf
    g[(u >= 0.06) & (u < 0.09)] = -np.inf
    return np.ascontiguousarray(g)


# ---- FAST scenes --------------------------------------------------------------------------------------------------------------------
# the smallest shapes that cross the scan's pass; in all but 63 x 8193 the segments of the later passes lie in the last three
# rows, which hold no hit, so there the carry reaches n_raw alone -- SCAN_BEYOND adds the smallest with hits behind the pass
SCAN_SHAPES = [(64, 4096), (64, 4097), (63, 8193), (128, 2049), (128, 2050)]
SCAN_BEYOND = [(64, 4103), (128, 2053), (128, 2054)]
SATURATED_SHAPES = [(192, 70), (128, 64)]
EDGE_W = (63, 64, 65, 66, 67, 69, 70, 71, 127, 128, 129, 131)
EDGE_H = (6, 7, 31, 32, 33, 35, 38, 64, 65)
EDGE_SEED = 3


def fast_scene(kind, w, h):
    """-> (grey image, threshold) of pattern `kind` ("dense" or "noise4", seeded by the shape)"""
    if kind == "dense":
        return dense(w, h), T_DENSE
    return noise4(w, h, EDGE_SEED + w * 131 + h), T_NOISE


def same_hits(got, exp):
    """two keypoint lists: same length, x, y, score and value BITS in the same (raster) order"""
    assert len(got) == len(exp), (len(got), len(exp))
    for f in ("x", "y", "fast_score"):
        assert (got[f] == exp[f]).all(), f
    assert np.asarray(got["value"]).tobytes() == np.asarray(exp["value"]).tobytes()


def segment_of(hits, w):
    """index of every hit's 64-pixel segment"""
    return hits["y"].astype(np.int64) * ((w + TW - 1) // TW) + hits["x"] // TW


def capacities(hits, w):
    """the capacities of the raw-capacity test on a list of n hits: n, n - 1, a cut at a segment boundary, one behind it
    (inside a segment), 1 and 0"""
    n = len(hits)
    seg = segment_of(hits, w)
    starts = np.flatnonzero(np.diff(seg) != 0) + 1          # indices at which a new segment begins
    boundary = int(starts[len(starts) // 2])
    return [n, n - 1, boundary, boundary + 1, 1, 0]


# ---- the chain: frames of the batched cases -------------------------------------------------------------------------------------------
def compact_batch(w, h):
    """three frames, noise4 / dense / noise4 (one threshold for a batch: T_DENSE, under which noise4's levels, 1/3 apart, give
    the hits they give under T_NOISE)"""
    return np.stack([noise4_frame(w, h, 11), dense_frame(w, h), noise4_frame(w, h, 12)])


def tail_batch(w, h, rows=40):
    """compact_batch with everything above the last `rows` rows flat: few hits, and most of them behind the scan's first pass"""
    frames = compact_batch(w, h)
    frames[:, :h - rows] = flat_frame(w, h - rows)
    return frames


def keep_all_detect(frame, pairs, T):
    """match_gpu.oracle_detect for a suppression radius below 1 and no limit, without the oracle's literal NMS loop, which copies
    the remaining list once per accepted point (n^2 / 2 steps: minutes at the 237 278 hits of the dense 64 x 4097 frame).  Two
    hits never share a pixel, so every distance is >= 1 > radius, nothing is ever dropped, and the loop emits its stable
    descending sort by score -- restated here as a stable argsort.  tests/test_front_limits_cases.py holds this to cref.nms
    at radius -1 and 0 on frames small enough for it."""
    g = cref.gray(frame)
    raw = cref.detect(g, T)
    kept = raw[np.argsort(-raw["fast_score"].astype(np.int64), kind="stable")]
    return kept, cref.brief(g, np.stack([kept["x"], kept["y"]], 1), pairs), len(raw)


def perm_map(w, h, seed):
    """a random in-range map with a few wrapped entries: the unchecked (ushort) casts take u - 65536 and v + 65536 to (u, v)"""
    rng = np.random.default_rng(seed)
    m = np.stack([rng.integers(0, w, (h, w)), rng.integers(0, h, (h, w))], axis=2).astype(np.int32)
    for y, x in ((0, 0), (h // 2, w // 3), (h - 1, w - 1)):
        m[y, x, 0] -= 65536
        m[y, x, 1] += 65536
    return m


BAD_SHAPES = [(200, 170), (201, 171)]
BAD_F = (61, 64)


def bad_entries(w, h):
    """output pixels (x, y) whose map entry the out-of-range run spoils: one mid-frame, one in the frame's last group of four
    pixels (the last pixel), one more; in textured regions (asserted on the oracle: each changes a compared list)"""
    return [(w // 2 + 1, h // 2 - 2), (w - 1, h - 1), (w // 3, 2 * h // 3 + 1)]


def bad_map(dmap, entries):
    """the map with the entries out of range, one by each of the ways a (ushort) cast value can miss the image"""
    m = dmap.copy()
    h, w = m.shape[:2]
    for (x, y), uv in zip(entries, [(w, 0), (0, -1), (w + 7, h)]):
        m[y, x] = uv
    return m


def oracle_chain(frame, dmap, pairs, T, radius, cap, zero=()):
    """match_gpu.oracle_detect restated without torch (that module uploads too): dewarp (dmap or None) -> gray -> detect -> NMS
    -> BRIEF by the oracle -> (kept keypoints, descriptors, raw hits).  zero: output pixels (x, y) of the dewarp made black
    before the grey image -- what the chain owes for a map whose entries there are out of range, which cref.apply_distortion
    refuses."""
    src = cref.apply_distortion(frame, dmap) if dmap is not None else np.array(frame)
    for x, y in zero:
        src[y, x] = 0
    g = cref.gray(src)
    raw = cref.detect(g, T)
    kept = raw[cref.nms(raw, radius)][:cap]
    return kept, cref.brief(g, np.stack([kept["x"], kept["y"]], 1), pairs), len(raw)


def zeroed_detect(frame, dmap, entries, pairs, T, radius, cap):
    return oracle_chain(frame, dmap, pairs, T, radius, cap, zero=entries)


BAD_T, BAD_RADIUS, BAD_CAP = np.float32(0.1), 4, 4096
BAD_CHECKED = (0, 1, 20, 33)                      # and the last frame of the batch


def bad_scene(w, h, src8, F=max(BAD_F)):
    """-> (frames [F][h][w][4] uint16 as the oracle sees them, dmap, pairs): textured frames under the shipped-coefficient
    table, the source pixel behind the frame's last output pixel white in every frame, and a short-reach pair table (sigma 6),
    so that the keypoints near the corner sample that pixel.  src8: the frames are 8-bit frames widened x257 (frames // 257 is
    what the device gets)."""
    from photogrammetry_amd import synth
    dmap = cref.build_distortion_matrix(w, h, [3e-4, 1e-7, 0, 0, 0])
    u, v = dmap[h - 1, w - 1]
    own = set(BAD_CHECKED) | {f - 1 for f in BAD_F}   # the frames a test compares; the others are shifted copies of frame 0
    first = synth.make_frame(w, h, seed=500, n_shapes=400)
    frames = np.stack([synth.make_frame(w, h, seed=500 + i, n_shapes=400) if i in own else np.roll(first, 3 * i, axis=1)
                       for i in range(F)])
    frames[:, v, u, :3] = 65535
    if src8:
        frames = (frames // 257).astype(np.uint16) * 257
    return frames, dmap, cref.gaussian_pairs(1, 6, 256)


def lists_differ(a, b):
    """two (kept, descriptors, n_raw) triples of the oracle chain differ somewhere"""
    return len(a[0]) != len(b[0]) or a[0].tobytes() != b[0].tobytes() or bool((a[1] != b[1]).any()) or a[2] != b[2]


# ---- BRIEF scenes -------------------------------------------------------------------------------------------------------------------
REACH = 20
OUTSIDE_SEED = 22                                 # a table under which the points just outside the image keep some set bit
TABLE_P = (31, 32, 63, 64, 65, 127, 128, 4033, 4063, 4064)
LIST_N = (0, 1, 3, 4, 5, 8, 9)
MAP_F = (7, 8, 9, 10, 16, 17)                     # 10: a remainder of two frames, see test_block_to_frame_map_scene
BIG = 1 << 30


def table(P, seed=21, reach=REACH):
    return np.random.default_rng(seed + P).integers(-reach, reach + 1, (P, 4)).astype(np.int32)


def outside_points(w, h):
    """-> (points int32 [n][2], far bool [n]): keypoints on, just outside and far outside the image, mixed with inside ones; far:
    farther than the table's reach from the image, so no sample can land inside.  Every x + offset stays inside int32."""
    pts = [(5, 7), (-1, -1), (w // 2, h // 2), (w, h), (w + 50, 3), (3, -50), (w - 1, h - 1), (BIG, 5), (-BIG, 5), (5, BIG),
           (5, -BIG), (0, 0), (-1, h // 2), (w // 2, h), (w + REACH, 10), (w + REACH - 1, 10), (10, -REACH - 1), (10, -REACH)]
    p = np.array(pts, dtype=np.int32)
    dx = np.maximum(np.maximum(-p[:, 0].astype(np.int64), p[:, 0].astype(np.int64) - (w - 1)), 0)
    dy = np.maximum(np.maximum(-p[:, 1].astype(np.int64), p[:, 1].astype(np.int64) - (h - 1)), 0)
    return p, (dx > REACH) | (dy > REACH)


def table_points(w, h):
    """nine keypoints, both corners among them"""
    return np.array([(0, 0), (w - 1, h - 1), (w // 2, h // 2), (3, h - 4), (w - 4, 3), (17, 23), (w - 1, 0), (40, 31), (61, 9)],
                    dtype=np.int32)


def map_frames(F, w=96, h=64):
    """F textured frames; frame 3 is flat, and with F >= 9 the last one too"""
    from photogrammetry_amd import synth
    frames = np.stack([synth.make_frame(w, h, seed=300 + i, n_shapes=60) for i in range(F)])
    flat = [3] + ([F - 1] if F >= 9 else [])
    for f in flat:
        frames[f] = flat_frame(w, h)
    return frames, flat


# ---- steered BRIEF ------------------------------------------------------------------------------------------------------------------
def half_plane(w, h, cx, cy, turns):
    """1.0 where dx + dy > 0 around (cx, cy), 0 elsewhere, turned by `turns` quarter turns about the point"""
    y, x = np.mgrid[0:h, 0:w]
    dx, dy = x - cx, y - cy
    for _ in range(turns % 4):
        dx, dy = dy, -dx
    return np.ascontiguousarray((dx + dy > 0).astype(np.float32))
