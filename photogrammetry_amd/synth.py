"""Synthetic inputs for tests, tools and bench.py: corner-rich RGBA64 frames, descriptor sets, the two-view scene
with its fundamental matrix, and multi-view scenes with tracks.  Pure data generation on the host, seeded; no reference code
or data.  device_tracks alone uploads what it made, and imports torch when called."""
import numpy as np


def make_frame(W, H, seed, n_shapes=None, background=0.5):
    """Seeded field of filled rectangles (axis-aligned and rotated) and 4-point stars of random
    grey on a mid-grey ground -> uint16 [H][W][4] (R=G=B, A=65535)."""
    rng = np.random.default_rng(seed)
    if n_shapes is None:
        n_shapes = max(8, (W * H) // 300)
    img = np.full((H, W), background, dtype=np.float32)
    for _ in range(n_shapes):
        cx, cy = rng.integers(0, W), rng.integers(0, H)
        hw, hh = rng.integers(3, 14), rng.integers(3, 14)
        grey = rng.choice([0.0, 0.15, 0.3, 0.7, 0.85, 1.0])
        kind = rng.integers(0, 3)
        r = int(max(hw, hh) * 1.5) + 1
        x0, x1 = max(0, cx - r), min(W, cx + r + 1)
        y0, y1 = max(0, cy - r), min(H, cy + r + 1)
        if x0 >= x1 or y0 >= y1:
            continue
        yy, xx = np.mgrid[y0:y1, x0:x1]
        dx, dy = (xx - cx).astype(np.float32), (yy - cy).astype(np.float32)
        if kind == 0:
            m = (np.abs(dx) <= hw) & (np.abs(dy) <= hh)
        elif kind == 1:
            a = rng.uniform(0, np.pi)
            u, v = dx * np.cos(a) + dy * np.sin(a), -dx * np.sin(a) + dy * np.cos(a)
            m = (np.abs(u) <= hw) & (np.abs(v) <= hh)
        else:
            m = (np.abs(dx) * hh + np.abs(dy) * hw <= hw * hh) | ((np.abs(dx) <= 1) & (np.abs(dy) <= hh * 1.4)) \
                | ((np.abs(dy) <= 1) & (np.abs(dx) <= hw * 1.4))
        img[y0:y1, x0:x1][m] = grey
    v = np.round(img * 65535.0).astype(np.uint16)
    out = np.empty((H, W, 4), dtype=np.uint16)
    out[..., 0] = v
    out[..., 1] = v
    out[..., 2] = v
    out[..., 3] = 65535
    return out


def shift_frame(frame, dx, dy, background=0.5):
    """Translate by (+dx, +dy) pixels, filling with the ground grey (how the reference made
    15pt_star_shifted_150.png: python_src/scripts/image_editing.py:4-15)."""
    H, W = frame.shape[:2]
    out = np.empty_like(frame)
    out[..., :3] = np.uint16(round(background * 65535.0))
    out[..., 3] = 65535
    sx0, sx1 = max(0, -dx), min(W, W - dx)
    sy0, sy1 = max(0, -dy), min(H, H - dy)
    if sx0 < sx1 and sy0 < sy1:
        out[sy0 + dy:sy1 + dy, sx0 + dx:sx1 + dx] = frame[sy0:sy1, sx0:sx1]
    return out


def random_descriptors(n, words, seed):
    """Uniform random descriptors: worst case for greedy rounds (distances ~ Binomial(P, 1/2))."""
    rng = np.random.default_rng(seed)
    return rng.integers(0, 2**32, size=(n, words), dtype=np.uint32)


def true_match_descriptors(n, words, seed, flip=0.15):
    """(set1, set2, perm): set2 = permuted set1 with `flip` of the bits flipped."""
    rng = np.random.default_rng(seed)
    d1 = rng.integers(0, 2**32, size=(n, words), dtype=np.uint32)
    bits = np.unpackbits(d1.view(np.uint8), axis=1)
    noise = (rng.random(bits.shape) < flip).astype(np.uint8)
    perm = rng.permutation(n)
    d2 = np.packbits(bits ^ noise, axis=1).view(np.uint32)[perm]
    return d1, np.ascontiguousarray(d2), perm


def flip_bits(rng, d, k):
    """d (uint32 [n][words]) with k (an int, or [n] ints) distinct random bits of every row flipped"""
    bits = np.unpackbits(np.ascontiguousarray(d).view(np.uint8), axis=1)
    rank = rng.random(bits.shape).argsort(1).argsort(1)
    mask = rank < np.broadcast_to(np.asarray(k), (len(d),))[:, None]
    return np.ascontiguousarray(np.packbits(bits ^ mask.astype(np.uint8), axis=1).view(np.uint32))


def far_descriptors(n1, n2, lo, hi, seed):
    """(set1, set2) of 256-bit descriptors in which every row's nearest column and every column's nearest row is FAR: rows are
    one prototype with every bit flipped at rate q, column j is the bit-complement of row perm[j] with 1..3 more bits
    flipped, so distance(i, j) = 256 - hamming(row i, copy j) and the nearest column is the least similar copy.  q is chosen
    so that the expected largest of n hamming distances (mean + sqrt(2 ln n) sd) is 256 - (lo + hi) / 2; callers check the
    range they need.  lo == hi pins EVERY distance at that value (255, 256, ...): identical rows, columns their complement
    with 256 - lo random bits flipped back, so every distance ties as well."""
    rng = np.random.default_rng(seed)
    proto = rng.integers(0, 2**32, size=(1, 8), dtype=np.uint32)
    if lo == hi:
        cols = ~np.repeat(proto, n2, axis=0)
        return np.repeat(proto, n1, axis=0), (flip_bits(rng, cols, 256 - lo) if lo < 256 else cols)
    n, want = max(n1, n2), 256.0 - (lo + hi) / 2.0
    qs = np.linspace(0.005, 0.5, 400)
    p = 2 * qs * (1 - qs)
    q = qs[np.argmin(np.abs(256 * p + np.sqrt(2 * np.log(n) * 256 * p * (1 - p)) - want))]
    bits = np.unpackbits(np.repeat(proto, n, axis=0).view(np.uint8), axis=1) ^ (rng.random((n, 256)) < q).astype(np.uint8)
    rows = np.ascontiguousarray(np.packbits(bits, axis=1).view(np.uint32))
    perm = rng.permutation(n)[:n2]
    return rows[:n1].copy(), ~flip_bits(rng, rows[perm], rng.integers(1, 4, n2))


def repeat_blocks(d, period):
    """In place: entry j + period holds the descriptor of entry j, for j in every other block of `period` entries (blocks
    0, 2, 4, ... are copied over blocks 1, 3, 5, ...; the last copy is cut at the end of the set)."""
    for b in range(0, len(d) - period, 2 * period):
        m = min(period, len(d) - b - period)
        d[b + period:b + period + m] = d[b:b + m]
    return d


def tiled_ties(n1, n2, period, seed, row_period=96):
    """(set1, set2) whose minima tie across the blockings of a matcher: column j + period repeats column j (repeat_blocks),
    every row is a copy of a random column with 0..2 bits flipped -- its minimum is attained at that column and at its repeat
    -- and row i + row_period repeats row i in the same way, so a column's minimum ties between rows as well.  Half of the
    columns stay distinct, so mutual-nearest rounds still take most rows."""
    rng = np.random.default_rng(seed)
    cols = repeat_blocks(rng.integers(0, 2**32, size=(n2, 8), dtype=np.uint32), period)
    rows = flip_bits(rng, cols[rng.integers(0, n2, n1)], rng.integers(0, 3, n1))
    return repeat_blocks(rows, row_period), cols


def rot_y(a):
    return np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]])


def skew(t):
    return np.array([[0, -t[2], t[1]], [t[2], 0, -t[0]], [-t[1], t[0], 0]])


def fundamental_from_pose(K, R, t):
    """F with h_a^T F h_b = 0 (include/pgx.h) for x_a ~ K X, x_b ~ K (R X + t); unit Frobenius norm, float32 [3][3]."""
    Ki = np.linalg.inv(K)
    F = (Ki.T @ skew(t) @ R @ Ki).T
    return (F / np.linalg.norm(F)).astype(np.float32)


def two_view_pixels(rng, n, K, R, t, W=3000, H=4000):
    """The two-view scene of the matcher and pose tests: n points drawn from rng in [-3, 3] x [-4, 4] x [4, 9], seen as
    x1 ~ K X and x2 ~ K (R X + t); kept are those whose rounded pixels are inside the W x H window in both views.
    -> (p1, p2) int32 [kept][2], in the order drawn"""
    X = np.stack([rng.uniform(-3, 3, n), rng.uniform(-4, 4, n), rng.uniform(4, 9, n)], 1)
    x1 = (K @ X.T).T
    x2 = (K @ (R @ X.T + t[:, None])).T
    p1 = np.rint(x1[:, :2] / x1[:, 2:3]).astype(np.int32)
    p2 = np.rint(x2[:, :2] / x2[:, 2:3]).astype(np.int32)
    ok = (p1 >= 0).all(1) & (p2 >= 0).all(1) & (p1[:, 0] < W) & (p2[:, 0] < W) & (p1[:, 1] < H) & (p2[:, 1] < H)
    return p1[ok], p2[ok]


def look_at_camera(centre, target, f=1200.0, W=1920, H=1080):
    """P = K [R | -R C] (float64 [3][4]) of a pinhole camera at `centre` looking at `target`; principal point at the image
    centre, image x along the camera's x axis and image y along its y axis (world +y projects downwards)."""
    R, t = look_at_pose(centre, target)
    K = np.array([[f, 0.0, W / 2.0], [0.0, f, H / 2.0], [0.0, 0.0, 1.0]])
    return K @ np.concatenate([R, t[:, None]], axis=1)


def look_at_pose(centre, target):
    """(R [3][3], t [3]) of look_at_camera: world -> camera is X -> R X + t, t = -R C."""
    c, t = np.asarray(centre, dtype=np.float64), np.asarray(target, dtype=np.float64)
    z = (t - c) / np.linalg.norm(t - c)
    x = np.cross([0.0, 1.0, 0.0], z)
    x /= np.linalg.norm(x)
    R = np.stack([x, np.cross(z, x), z])
    return R, -R @ c


def make_scene(n_points, n_frames, seed=0, box=1.5, radius=5.0, arc_deg=60.0, f=1200.0, W=1920, H=1080, pairs=None,
               wrong_rate=0.0, offset=(0.0, 0.0, 0.0)):
    """A synthetic multi-view scene with known truth, for the track graph and triangulation.
    n_points uniform in the box [-box, box]^3; n_frames pinhole cameras (W x H, focal f) on an arc of arc_deg degrees at `radius`
    around the box (heights alternate slightly), all looking at its centre.  A point is seen in a frame if it is in front of
    the camera and its rounded projection lies in the image; the keypoints of a frame are those rounded projections
    (x = column, y = row), shuffled.  `offset` translates the whole scene (points and cameras): the keypoints do not change.
    pairs: image pairs (a, b) for which match lists in the pgx_pair layout are made: for every keypoint k1 of frame a
    (k1, k2, 0) if its point is seen in b as keypoint k2, else (k1, -1, PGX_DIST_NONE); a fraction wrong_rate of the rows with
    a true link instead link a random other keypoint of b (dist 0).
    -> dict(points [N][3], P [F][12], K [F][4] (fx, fy, cx, cy), Rt [F][12] (R row-major, then t; P = K [R | t]),
            centres [F][3], kps [F] of KEYPOINT_DTYPE, point_id [F] (point of each keypoint), uv [F] ([n][2] unrounded
            projections in keypoint order), counts [F], pairs [(a, b)], lists [M] of PAIR_DTYPE, wrong [M] (bool per row: a
            planted wrong link))"""
    from .api import KEYPOINT_DTYPE, PAIR_DTYPE
    from ._lib import PGX_DIST_NONE
    rng = np.random.default_rng(seed)
    off = np.asarray(offset, dtype=np.float64)
    pts = rng.uniform(-box, box, size=(n_points, 3))
    ang = np.radians(np.linspace(-arc_deg / 2.0, arc_deg / 2.0, n_frames)) if n_frames > 1 else np.zeros(1)
    centres = np.stack([radius * np.sin(ang), 0.15 * radius * ((np.arange(n_frames) % 3) - 1) / 3.0, -radius * np.cos(ang)], 1)
    kps, pid, uvs, Ps = [], [], [], []
    for j in range(n_frames):
        P0 = look_at_camera(centres[j], np.zeros(3), f, W, H)
        h = pts @ P0[:, :3].T + P0[:, 3]
        with np.errstate(divide="ignore", invalid="ignore"):
            uv = h[:, :2] / h[:, 2:3]
        r = np.round(uv)
        vis = np.flatnonzero((h[:, 2] > 0) & (r[:, 0] >= 0) & (r[:, 0] < W) & (r[:, 1] >= 0) & (r[:, 1] < H))
        vis = vis[rng.permutation(len(vis))]
        k = np.zeros(len(vis), dtype=KEYPOINT_DTYPE)
        k["x"], k["y"] = r[vis, 0].astype(np.int32), r[vis, 1].astype(np.int32)
        kps.append(k)
        pid.append(vis.astype(np.int64))
        uvs.append(uv[vis])
        Ps.append(look_at_camera(centres[j] + off, off, f, W, H).reshape(12))
    lists, wrong = [], []
    for a, b in (pairs or []):
        where = np.full(n_points, -1, dtype=np.int64)
        where[pid[b]] = np.arange(len(pid[b]))
        k2 = where[pid[a]]
        m = np.zeros(len(pid[a]), dtype=PAIR_DTYPE)
        m["k1"] = np.arange(len(pid[a]))
        bad = (k2 >= 0) & (rng.random(len(k2)) < wrong_rate) & (len(pid[b]) > 1)
        if bad.any():
            alt = rng.integers(0, len(pid[b]) - 1, size=int(bad.sum()))
            k2[bad] = alt + (alt >= k2[bad])      # any keypoint of b but the true one
        m["k2"] = k2
        m["dist"] = np.where(k2 >= 0, 0, PGX_DIST_NONE)
        lists.append(m)
        wrong.append(bad)
    Rts = []
    for j in range(n_frames):
        R, t = look_at_pose(centres[j] + off, off)
        Rts.append(np.concatenate([R.reshape(9), t]))
    Ks = np.tile([f, f, W / 2.0, H / 2.0], (n_frames, 1))
    return dict(points=pts + off, P=np.array(Ps).reshape(n_frames, 12), K=Ks, Rt=np.array(Rts).reshape(n_frames, 12),
                centres=centres + off, kps=kps, point_id=pid, uv=uvs, counts=np.array([len(k) for k in kps], dtype=np.int32),
                pairs=list(pairs or []), lists=lists, wrong=wrong)


def scene_tracks(scene, min_len=2):
    """The true tracks of a make_scene scene: one per point seen in >= min_len frames, nodes in frame order.
    -> (offsets [n + 1] int32, nodes [n_nodes][2] int32, point [n] (the point of each track))"""
    seen = {}
    for f, pid in enumerate(scene["point_id"]):
        for k, p in enumerate(pid):
            seen.setdefault(int(p), []).append((f, k))
    pts = [p for p in sorted(seen) if len(seen[p]) >= min_len]
    off = np.concatenate([[0], np.cumsum([len(seen[p]) for p in pts])]).astype(np.int32)
    nodes = np.array([n for p in pts for n in seen[p]], dtype=np.int32).reshape(-1, 2)
    return off, nodes, np.array(pts, dtype=np.int64)


def cut_tracks(scene, lengths, seed=0):
    """Tracks of chosen lengths from a make_scene scene: point p's views, in frame order, cut to one contiguous run of
    min(lengths[p], views of p) nodes at a seeded random start; points left with fewer than 2 nodes give no track.
    lengths: [n_points] ints (tests/test_gpu_geometry_limits.py), or a pair (lo, hi): every seen point's length is then
    drawn from the same generator as integers(lo, hi), length first, then start -- the scenes of tools/geom_bench.py, whose
    recorded shapes depend on that order.  seed: an int, or the generator to draw from.
    -> (offsets [n + 1] int32, nodes [n_nodes][2] int32, point [n] (the point of each track))"""
    rng = np.random.default_rng(seed)
    seen = {}
    for f, pid in enumerate(scene["point_id"]):
        for k, p in enumerate(pid):
            seen.setdefault(int(p), []).append((f, k))
    tracks, pts = [], []
    for p in sorted(seen):
        v = seen[p]
        L = min(len(v), int(rng.integers(*lengths)) if isinstance(lengths, tuple) else int(lengths[p]))
        if L < 2:
            continue
        a = int(rng.integers(0, len(v) - L + 1))
        tracks.append(v[a:a + L])
        pts.append(p)
    off = np.concatenate([[0], np.cumsum([len(t) for t in tracks])]).astype(np.int32)
    nodes = np.array([n for t in tracks for n in t], dtype=np.int32).reshape(-1, 2)
    return off, nodes, np.array(pts, dtype=np.int64)


def slot_layout(kps, slots=None, n_slots=None):
    """The keypoint buffer of a track-graph consumer on the host.  kps: [nf] of KEYPOINT_DTYPE or of [n][2] (x, y);
    slots[f] = the slot frame f sits in (default: f) among n_slots (default: nf); other slots are padding: frame id -1, no
    keypoints.  -> dict(kp [F][stride] KEYPOINT_DTYPE, counts [F], ids [F], slots, F, nf, stride, identity)"""
    from .api import KEYPOINT_DTYPE
    nf = len(kps)
    slots = list(range(nf)) if slots is None else list(slots)
    F = nf if n_slots is None else n_slots
    stride = max(1, max(len(k) for k in kps))
    kp = np.zeros((F, stride), dtype=KEYPOINT_DTYPE)
    counts = np.zeros(F, np.int32)
    ids = np.full(F, -1, np.int32)
    for f, k in enumerate(kps):
        k = np.asarray(k)
        if k.dtype == KEYPOINT_DTYPE:
            kp[slots[f], :len(k)] = k
        elif len(k):
            kp["x"][slots[f], :len(k)], kp["y"][slots[f], :len(k)] = k[:, 0], k[:, 1]
        counts[slots[f]] = len(k)
        ids[slots[f]] = f
    return dict(kp=kp, counts=counts, ids=ids, slots=slots, F=F, nf=nf, stride=stride,
                identity=n_slots is None and slots == list(range(nf)))


def device_tracks(kps, off, nodes, slots=None, n_slots=None, device="cuda:0"):
    """Device buffers of a track-graph consumer's input (triangulation, bundle adjustment, registration; the GPU tests and
    tools/geom_bench.py): slot_layout's keypoints and frame ids, offsets, nodes and a track summary with n_tracks and
    n_nodes.  -> dict(kp [F][stride][4] int32, ids, off, nodes, tsum [8] (torch tensors), F, nf, stride, identity, n_tracks,
    n_nodes)"""
    import torch
    lay = slot_layout(kps, slots, n_slots)
    F, stride, n = lay["F"], lay["stride"], len(off) - 1
    return dict(kp=torch.from_numpy(lay["kp"].view(np.int32).reshape(F, stride, 4)).to(device),
                ids=torch.from_numpy(lay["ids"]).to(device), F=F, nf=lay["nf"], stride=stride, identity=lay["identity"],
                off=torch.from_numpy(np.asarray(off, np.int32)).to(device),
                nodes=torch.from_numpy(np.ascontiguousarray(nodes, np.int32).reshape(-1, 2)).to(device),
                tsum=torch.tensor([n, len(nodes), 0, 0, 0, 0, 0, 0], dtype=torch.int32, device=device), n_tracks=n,
                n_nodes=len(nodes))


def perturb(Rt, xyz, seed, rot_deg=0.3, centre_sigma=0.05, point_sigma=0.015, fixed=None):
    """Cameras and points moved by a seeded random amount, for bundle adjustment: each camera's R turned by rot_deg degrees
    about a random axis (R' = Exp(w) R) and its centre C = -R^T t moved by a random vector of length centre_sigma; each point
    moved by N(0, point_sigma^2) per coordinate.  Frames with fixed[f] != 0 are returned unchanged.
    -> (Rt [F][12], xyz [n][3])"""
    rng = np.random.default_rng(seed)
    Rt = np.array(Rt, dtype=np.float64).reshape(-1, 12)
    out = Rt.copy()
    for f in range(len(Rt)):
        axis = rng.normal(size=3)
        dirn = rng.normal(size=3)
        if fixed is not None and fixed[f]:
            continue
        axis *= np.radians(rot_deg) / np.linalg.norm(axis)
        R, t = Rt[f, :9].reshape(3, 3), Rt[f, 9:]
        C = -R.T @ t + dirn * (centre_sigma / np.linalg.norm(dirn))
        th = np.linalg.norm(axis)
        k = axis / th
        Kx = np.array([[0.0, -k[2], k[1]], [k[2], 0.0, -k[0]], [-k[1], k[0], 0.0]])
        R2 = (np.eye(3) + np.sin(th) * Kx + (1.0 - np.cos(th)) * (Kx @ Kx)) @ R
        out[f, :9] = R2.reshape(9)
        out[f, 9:] = -R2 @ C
    X = np.array(xyz, dtype=np.float64).reshape(-1, 3)
    return out, X + rng.normal(scale=point_sigma, size=X.shape)
