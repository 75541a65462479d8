"""numpy restatement of the scale pyramid (include/pgx.h, "Scale pyramid"; the kernels are csrc/k_pyramid.hip), for the tests
that hold the library to it bit for bit.  Rules 1, 2 and 5 are integer arithmetic; rule 3 is nine single float32 operations
per pixel, which numpy's float32 ufuncs perform one by one (no fused multiply-add), so there is no tolerance anywhere.  Rule 4,
the chain on a level image, is the oracle's (oracle.cref.detect / nms / brief), or tests/steered_ref.py in steered mode.
A plain helper module, next to steered_ref.py and knn_ref.py."""
import numpy as np

import knn_ref
import steered_ref
from oracle import cref

KP_DTYPE = np.dtype([("x", "<i4"), ("y", "<i4"), ("fast_score", "<i4"), ("value", "<f4")])
STEP_MIN, STEP_MAX, MIN_SIDE = 69632, 131072, 16


def dims(W, H, n_levels, step):
    """Rules 1 and 2 -> (dims int64 [n_levels][2] = (W_l, H_l), (0, 0) for an empty level; scale int64 [n_levels] = S_l)."""
    assert 1 <= n_levels <= 8 and STEP_MIN <= step <= STEP_MAX
    d, s = np.zeros((n_levels, 2), np.int64), np.zeros(n_levels, np.int64)
    w, h, S, empty = int(W), int(H), 65536, False
    for l in range(n_levels):
        if l:
            w, h = (w * 65536) // step, (h * 65536) // step
            S = (S * step + 32768) >> 16
            empty = empty or w < MIN_SIDE or h < MIN_SIDE
        d[l] = (0, 0) if empty else (w, h)
        s[l] = S
    return d, s


def taps(n_dst, n_src, step):
    """Rule 3 along one axis -> (i0 int64 [n_dst], i1, fraction float32 [n_dst], q int64 [n_dst])."""
    x = np.arange(n_dst, dtype=np.int64)
    q = ((2 * x + 1) * np.int64(step) - 65536) >> 1
    i0 = q >> 16
    i1 = np.minimum(i0 + 1, n_src - 1)
    fr = (q & 65535).astype(np.float32) * np.float32(2.0 ** -16)
    return i0, i1, fr, q


def down(src, step):
    """Rule 3: the next level of a float32 image."""
    src = np.ascontiguousarray(src, dtype=np.float32)
    Hs, Ws = src.shape
    Wd, Hd = (Ws * 65536) // step, (Hs * 65536) // step
    x0, x1, fx, _ = taps(Wd, Ws, step)
    y0, y1, fy, _ = taps(Hd, Hs, step)
    fx, fy = fx[None, :], fy[:, None]
    a, b = src[y0][:, x0], src[y0][:, x1]
    c, d = src[y1][:, x0], src[y1][:, x1]
    t = a + fx * (b - a)
    u = c + fx * (d - c)
    out = t + fy * (u - t)
    assert out.dtype == np.float32
    return np.ascontiguousarray(out)


def levels(gray0, n_levels, step):
    """The level images of a grey image: a list of n_levels entries, None for an empty level."""
    g = np.ascontiguousarray(gray0, dtype=np.float32)
    d, _ = dims(g.shape[1], g.shape[0], n_levels, step)
    out = [g]
    for l in range(1, n_levels):
        out.append(None if d[l, 0] == 0 else down(out[-1], step))
        assert out[-1] is None or out[-1].shape == (d[l, 1], d[l, 0])
    return out


def to_level0(v, S, n0):
    """Rule 5: a level coordinate on level 0's pixel grid."""
    return np.minimum(((2 * np.asarray(v, np.int64) + 1) * np.int64(S)) >> 17, n0 - 1)


def detect_pyramid(gray0, n_levels, step, T, radius, pairs, capacity=None, raw_cap=None, kp_cap=None, steer=None):
    """Rules 4 and 5 for one frame.  raw_cap / kp_cap: pgx_set_capacity's limits, per level (None: none); capacity: the caller's
    list size (None: unbounded); steer = (pairs_rot, dirs, R) for steered descriptors.
    -> dict(kp KP_DTYPE [n], desc uint32 [n][words], origin int32 [n][3], bins int32 [n] or None, stats int32 [n_levels][2],
    count, nraw, total (before the capacity cut), raw_over (a level exceeded raw_cap))."""
    g0 = np.ascontiguousarray(gray0, dtype=np.float32)
    H, W = g0.shape
    _, scale = dims(W, H, n_levels, step)
    kps, descs, origins, bins = [], [], [], []
    stats = np.zeros((n_levels, 2), np.int32)
    raw_over = False
    words = (len(pairs) + 31) // 32
    for l, g in enumerate(levels(g0, n_levels, step)):
        if g is None:
            continue
        raw = cref.detect(g, np.float32(T))
        stats[l, 1] = len(raw)
        if raw_cap is not None and len(raw) > raw_cap:
            raw, raw_over = raw[:raw_cap], True
        kept = raw[cref.nms(raw, radius)] if len(raw) else raw
        if kp_cap is not None:
            kept = kept[:kp_cap]
        xy = np.stack([kept["x"], kept["y"]], axis=1).astype(np.int64).reshape(-1, 2)
        if steer is not None:
            b, d = steered_ref.describe(g, xy, *steer)
        else:
            b, d = np.zeros(len(xy), np.int32), (cref.brief(g, xy, pairs) if len(xy) else np.zeros((0, words), np.uint32))
        out = np.zeros(len(kept), KP_DTYPE)
        out["x"], out["y"] = to_level0(xy[:, 0], scale[l], W), to_level0(xy[:, 1], scale[l], H)
        out["fast_score"], out["value"] = kept["fast_score"], g[xy[:, 1], xy[:, 0]]
        kps.append(out)
        descs.append(d)
        bins.append(b)
        origins.append(np.concatenate([np.full((len(xy), 1), l, np.int64), xy], axis=1).astype(np.int32))
        stats[l, 0] = len(kept)
    kp, desc = np.concatenate(kps), np.concatenate(descs)
    total = len(kp)
    n = total if capacity is None else min(total, capacity)
    left = n
    for l in range(n_levels):                      # entries of each level IN the list
        stats[l, 0] = min(int(stats[l, 0]), left)
        left -= stats[l, 0]
    return dict(kp=kp[:n], desc=desc[:n], origin=np.concatenate(origins)[:n], bins=np.concatenate(bins)[:n] if steer else None,
                stats=stats, count=n, nraw=int(stats[:, 1].sum()), total=total, raw_over=raw_over)


def shrink2(gray):
    """An image shrunk by 2 with a float64 2 x 2 box mean -> float32 (the zoomed-out partner of the quality case)."""
    g = np.asarray(gray, dtype=np.float64)
    H, W = g.shape[0] // 2 * 2, g.shape[1] // 2 * 2
    g = g[:H, :W]
    return np.ascontiguousarray(((g[0::2, 0::2] + g[0::2, 1::2] + g[1::2, 0::2] + g[1::2, 1::2]) / 4).astype(np.float32))


def nn_accept(desc_a, desc_b, max_dist=64, ratio=0.8):
    """pgx_match_nn_batch_dev's list (distance gate, ratio test, cross-check) of A's rows against B -> int32 [n_a][3]."""
    idx, dist, col = knn_ref.ref_knn(desc_a, desc_b)
    return knn_ref.ref_select(idx, dist, col, max_dist, ratio, True)


def correct_matches(kp_a, kp_b, sel, tol=2.0):
    """(accepted, correct) of a list from nn_accept for A = the full image and B = shrink2(A): pixel i of B covers pixels 2i
    and 2i + 1 of A, so A's (x, y) lies at ((x - 0.5) / 2, (y - 0.5) / 2) in B; correct = within tol px of it."""
    ok = sel[:, 1] >= 0
    a, b = kp_a[sel[ok, 0]], kp_b[sel[ok, 1]]
    dx = (a["x"].astype(np.float64) - 0.5) / 2 - b["x"]
    dy = (a["y"].astype(np.float64) - 0.5) / 2 - b["y"]
    return int(ok.sum()), int((np.hypot(dx, dy) <= tol).sum())


def quality_case(seed, n_levels=4, step=92682, W=640, H=480, T=0.1, radius=6):
    """The zoom case of DESIGN.md section 19 on the reference alone: A = a synthetic frame, B = A shrunk by 2, B described at one
    scale, A at one scale and with the pyramid -> dict(A, B, pairs, single=(accepted, correct), pyramid=(accepted, correct),
    ref_a (detect_pyramid of A), kp_b, desc_b, sel (the pyramid's accepted list))."""
    from photogrammetry_amd import synth
    frame = synth.make_frame(W, H, seed)
    A = cref.gray(frame)
    B = shrink2(A)
    pairs = cref.gaussian_pairs(0, 8, 256)
    one_a = detect_pyramid(A, 1, step, T, radius, pairs)
    one_b = detect_pyramid(B, 1, step, T, radius, pairs)
    pyr_a = detect_pyramid(A, n_levels, step, T, radius, pairs)
    single = correct_matches(one_a["kp"], one_b["kp"], nn_accept(one_a["desc"], one_b["desc"]))
    sel = nn_accept(pyr_a["desc"], one_b["desc"])
    return dict(frame=frame, A=A, B=B, pairs=pairs, single=single, pyramid=correct_matches(pyr_a["kp"], one_b["kp"], sel),
                ref_a=pyr_a, ref_b=one_b, sel=sel)
