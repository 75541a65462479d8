"""numpy restatement of steered BRIEF (include/pgx.h, "Steered BRIEF"; the kernels are csrc/k_steer.hip), for the tests that hold
the device to it bit for bit.  Everything is integer arithmetic after q(g), so there is no tolerance anywhere.  Step 4, the
descriptor itself, is the oracle's Keypoint.GetBriefDescriptor (oracle.cref.brief) with the table of the keypoint's bin.
A plain helper module, next to knn_ref.py and guided_ref.py."""
import numpy as np

from oracle import cref


def quantise(gray):
    """Step 1, q(g): NaN -> 0, clamp to [0, 1], ONE float32 multiplication by 65535, round to nearest even -> int64 [H][W]."""
    g = np.asarray(gray, dtype=np.float32)
    c = np.clip(np.where(np.isnan(g), np.float32(0), g), np.float32(0), np.float32(1)).astype(np.float32)
    return np.rint(c * np.float32(65535)).astype(np.int64)


def disc(R):
    """(dx, dy) int64 [n] of every integer offset with dx^2 + dy^2 <= R^2."""
    d = np.arange(-R, R + 1, dtype=np.int64)
    dx, dy = np.meshgrid(d, d)
    keep = dx * dx + dy * dy <= R * R
    return dx[keep], dy[keep]


def moments(gray, xy, R):
    """Step 2: (m10, m01) int64 [N] of the disc of radius R around every (x, y); a pixel outside the image contributes 0."""
    q = quantise(gray)
    H, W = q.shape
    dx, dy = disc(R)
    xy = np.asarray(xy, dtype=np.int64).reshape(-1, 2)
    m10, m01 = np.zeros(len(xy), np.int64), np.zeros(len(xy), np.int64)
    for i, (x, y) in enumerate(xy):
        xs, ys = x + dx, y + dy
        ok = (xs >= 0) & (xs < W) & (ys >= 0) & (ys < H)
        v = q[ys[ok], xs[ok]]
        m10[i], m01[i] = (dx[ok] * v).sum(), (dy[ok] * v).sum()
    return m10, m01


def scores(gray, xy, dirs, R):
    """Step 3's s_k, int64 [N][B]."""
    m10, m01 = moments(gray, xy, R)
    d = np.asarray(dirs, dtype=np.int64).reshape(-1, 2)
    return m10[:, None] * d[None, :, 0] + m01[:, None] * d[None, :, 1]


def bins(gray, xy, dirs, R):
    """Step 3: the smallest k with the largest s_k, int32 [N] (argmax returns the first maximum)."""
    return scores(gray, xy, dirs, R).argmax(axis=1).astype(np.int32)


def describe(gray, xy, pairs_rot, dirs, R):
    """Steps 1-4 -> (bins int32 [N], descriptors uint32 [N][ceil(P/32)])."""
    xy = np.asarray(xy, dtype=np.int64).reshape(-1, 2)
    t = np.asarray(pairs_rot, dtype=np.int32)
    b = bins(gray, xy, dirs, R)
    out = np.zeros((len(xy), (t.shape[1] + 31) // 32), dtype=np.uint32)
    for k in np.unique(b):
        out[b == k] = cref.brief(gray, xy[b == k], t[k])
    return b, out


def rot90_points(xy, W, H, j):
    """Where the pixels (x, y) of a [H][W] image lie in np.rot90(image, j): one turn takes (x, y) to (y, W - 1 - x)."""
    xy = np.asarray(xy, dtype=np.int64).reshape(-1, 2).copy()
    for _ in range(j % 4):
        xy = np.stack([xy[:, 1], W - 1 - xy[:, 0]], axis=1)
        W, H = H, W
    return xy


def all_inside(shape, xy, R, pairs_rot, b):
    """bool [N]: the disc of radius R and every sample of the table pairs_rot[b[i]] around (x, y) lie inside the image."""
    H, W = shape
    xy = np.asarray(xy, dtype=np.int64).reshape(-1, 2)
    t = np.asarray(pairs_rot, dtype=np.int64)[np.asarray(b)]          # [N][P][4]
    xs = np.concatenate([xy[:, :1] + t[:, :, 0], xy[:, :1] + t[:, :, 2], xy[:, :1] - R, xy[:, :1] + R], axis=1)
    ys = np.concatenate([xy[:, 1:] + t[:, :, 1], xy[:, 1:] + t[:, :, 3], xy[:, 1:] - R, xy[:, 1:] + R], axis=1)
    return ((xs >= 0) & (xs < W) & (ys >= 0) & (ys < H)).all(axis=1)


def unique_maximum(s):
    """bool [N]: the two largest s_k of every row differ (the bin does not hang on the tie rule)."""
    top = np.sort(np.asarray(s), axis=1)[:, -2:]
    return top[:, 1] > top[:, 0]


def quarter_turn_case(gray, xy, pairs_rot, dirs, R, j):
    """An image, its np.rot90 by j turns and the same physical points in both.
    -> dict(turned, xy_turned, bins, desc, bins_turned, desc_turned, qualifies): a keypoint qualifies when its disc and all
    samples lie inside both images and its two largest s_k differ in both."""
    g = np.ascontiguousarray(gray, dtype=np.float32)
    H, W = g.shape
    turned = np.ascontiguousarray(np.rot90(g, j))
    xy2 = rot90_points(xy, W, H, j)
    b1, d1 = describe(g, xy, pairs_rot, dirs, R)
    b2, d2 = describe(turned, xy2, pairs_rot, dirs, R)
    ok = all_inside(g.shape, xy, R, pairs_rot, b1) & all_inside(turned.shape, xy2, R, pairs_rot, b2)
    ok &= unique_maximum(scores(g, xy, dirs, R)) & unique_maximum(scores(turned, xy2, dirs, R))
    return dict(turned=turned, xy_turned=xy2, bins=b1, desc=d1, bins_turned=b2, desc_turned=d2, qualifies=ok)


def smooth_image(W, H, seed):
    """A smooth seeded float32 image in (0, 1): a sum of low-frequency waves, so that every disc has a clear centroid."""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:H, 0:W].astype(np.float64)
    img = np.zeros((H, W))
    for _ in range(12):
        fx, fy = rng.uniform(-0.12, 0.12, 2)
        img += rng.uniform(0.3, 1.0) * np.sin(fx * x + fy * y + rng.uniform(0, 2 * np.pi))
    img = (img - img.min()) / (img.max() - img.min())
    return np.ascontiguousarray((0.05 + 0.9 * img).astype(np.float32))


def hamming(d1, d2):
    """Bits that differ, per row."""
    return np.unpackbits((np.asarray(d1) ^ np.asarray(d2)).view(np.uint8), axis=1).sum(axis=1)
