"""Scenes and CPU helpers of tests/test_gpu_front_fused.py (no torch, no GPU): the batch path's level 0 runs dewarp, grey and
FAST in one tile kernel (csrc/k_fast.hip: k_dewarp_fast) off the gather plan of the installed map (csrc/k_image.hip:
k_dewarp_plan).  Here: the frame sizes, the batches, the maps and what the oracle owes for each -- cref.apply_distortion ->
cref.gray -> cref.detect -> cref.nms -> cref.brief, with the pixels black whose map entry lies outside the image after the
(ushort) wrap, which cref.apply_distortion itself refuses.  That every scene does what it is named for is asserted in
tests/test_front_fused_cases.py on the oracle alone.  A plain helper module: no test module imports another."""
import functools

import numpy as np

import front_limits_cases as fc
from oracle import cref

TW, TH, HALO = fc.TW, fc.TH, fc.HALO
FG = 8                                            # k_dewarp_fast: frames of a tile that run back to back (its block -> frame map)

# 6 x 6: no interior pixel; 7 x 7: one candidate; 64 x 32: exactly one tile; 65 x 33: one pixel into the next tile each way;
# the last two ragged both ways (2 x 2 and 4 x 5 tiles)
SIZES = [(6, 6), (7, 7), (64, 32), (65, 33), (83, 60), (200, 131)]
# batch sizes: 1, 3, 5, 9 frames, and 7 | 8 | 9 on the two sides of the frame group
BATCHES = (1, 3, 5, 7, 8, 9)
F_MAX = max(BATCHES)
FLAT = (4,)                                       # the flat frame of a batch
DENSE = (1,)                                      # the dense frame of a batch
MAPS = ("none", "identity", "shift", "wrap", "flip", "halo")
# one threshold for a batch: noise4's levels are 1/3 apart (front_limits_cases).  Radius 10: the mask rounds of the default path;
# at radius 3 the 24 000 tied hits of the dense 200 x 131 frame took the device's NMS 1.5 s per call, none of it this kernel's
T, RADIUS, CAP, RAW = fc.T_DENSE, 10, 4096, 1 << 16


def frames_of(w, h):
    """F_MAX frames [h][w][4] uint16: dense at 1, flat at 4, noise4 (a seed each) elsewhere.  Every channel value is a multiple of
    257 (levels of 65535 / 15 = 17 * 257 and 65535 / 3 = 85 * 257), so frames // 257 is the same batch as 8-bit RGBA."""
    out = []
    for i in range(F_MAX):
        if i in FLAT:
            f = fc.flat_frame(w, h)
            f[..., :3] = 64 * 257
        elif i in DENSE:
            f = fc.dense_frame(w, h)
        else:
            f = fc.noise4_frame(w, h, 40 + i + w)
        out.append(f)
    frames = np.stack(out)
    assert ((frames // 257) * 257 == frames).all()
    return frames


def halo_pixel(w, h):
    """the output pixel the "halo" map sends outside: in the three-pixel halo of tile (0, 0) where the frame reaches that far
    (right of column 63, below row 31), the frame's last pixel otherwise"""
    return (TW + 1 if w > TW + 1 else w - 1, TH + 1 if h > TH + 1 else h - 1)


def make_map(kind, w, h):
    """[h][w][2] int32 (u, v) entries, or None"""
    if kind == "none":
        return None
    y, x = np.mgrid[0:h, 0:w]
    if kind == "identity":
        u, v = x, y
    elif kind == "shift":                         # the last five columns and the first two rows come from outside the image
        u, v = x + 5, y - 2
    elif kind == "flip":                          # 180 degrees: a tile's sources are far away and descending
        u, v = w - 1 - x, h - 1 - y
    elif kind == "wrap":                          # mirrored columns; entries below 0 and above 65535 that wrap back inside
        u, v = (w - 1 - x).copy(), y.copy()
        u[(x + y) % 3 == 0] -= 65536
        v[(x + 2 * y) % 5 == 0] += 2 * 65536
    else:
        assert kind == "halo"
        u, v = x.copy(), y.copy()
        hx, hy = halo_pixel(w, h)
        u[hy, hx] = w                             # one column past the image
    return np.ascontiguousarray(np.stack([u, v], axis=2).astype(np.int32))


def outside(dmap):
    """bool [h][w]: the entries whose source lies outside the image after the unchecked (ushort) casts"""
    h, w = dmap.shape[:2]
    return ((dmap[..., 0] & 0xFFFF) >= w) | ((dmap[..., 1] & 0xFFFF) >= h)


def dewarp(frame, dmap):
    """cref.apply_distortion with the wrapped entries; the pixels of `outside` black (the oracle refuses their entries)"""
    if dmap is None:
        return np.array(frame)
    bad = outside(dmap)
    safe = (dmap & 0xFFFF).astype(np.int32)
    safe[bad] = 0
    out = cref.apply_distortion(frame, np.ascontiguousarray(safe))
    out[bad] = 0
    return out


def chain(frame, dmap, pairs, T=T, radius=RADIUS, cap=CAP):
    """-> (kept keypoints, descriptors, raw hits) as match_gpu.oracle_detect gives them, on the frame dewarped by `dewarp`"""
    g = cref.gray(dewarp(frame, dmap))
    raw = cref.detect(g, T)
    kept = raw[cref.nms(raw, radius)][:cap]
    return kept, cref.brief(g, np.stack([kept["x"], kept["y"]], 1), pairs), len(raw)


@functools.lru_cache(maxsize=None)
def brief_pairs():
    return cref.gaussian_pairs(1, 6, 256)


@functools.lru_cache(maxsize=None)
def scene(w, h, kind):
    """-> (frames, dmap, [the oracle's triple per frame]) of one size and map, computed once and left unchanged; the 8-bit
    batch is frames // 257 and owes the same lists"""
    frames = frames_of(w, h)
    dmap = make_map(kind, w, h)
    return frames, dmap, [chain(f, dmap, brief_pairs()) for f in frames]
