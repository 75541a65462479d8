"""numpy float64 restatement of the dense stage's plan (include/pgx.h, "the plan of the dense stage"): the yardstick of
tests/test_gpu_dense_views.py.  Every value is a float64 and every operation one IEEE operation in the order the header writes
it (sums of three as ((a + b) + c), no dot products from a library), so every integer and every bit of the range can be held
to this file.  Two forms that share no line of arithmetic: plan() vectorised over all nodes and over the pairs of the tracks of
one length, plan_loop() track by track in Python floats with its own camera algebra.  Both take the order statistics from
numpy.sort.  A plain helper module."""
import math

import numpy as np

from consensus_ref import frames as consensus_frames

NOCAMERA, FEWPOINTS, FEWVIEWS, NARROW = 1, 2, 4, 8
DEFAULTS = dict(min_angle_deg=2.0, max_angle_deg=45.0, min_shared=8, min_points=8, q_near_pm=10, q_far_pm=990, grow=1.25)
PAIR_CHUNK = 1 << 22      # pairs per vectorised step of plan()


def cos2_of(deg):
    """the square of the host C library's cos(deg * M_PI / 180.0)"""
    c = math.cos(deg * math.pi / 180.0)
    return c * c


def _inputs(offsets, nodes, xyz, flags, P, refs, max_tracks):
    off = np.asarray(offsets, dtype=np.int64).reshape(-1)
    nd = np.asarray(nodes, dtype=np.int64).reshape(-1, 2)
    n = len(off) - 1
    X = np.asarray(xyz, dtype=np.float64).reshape(-1, 3)
    fl = None if flags is None else np.asarray(flags, dtype=np.int64).reshape(-1)
    P = np.asarray(P, dtype=np.float64).reshape(-1, 12)
    rf = np.arange(len(P), dtype=np.int64) if refs is None else np.asarray(refs, dtype=np.int64).reshape(-1)
    nt = n if max_tracks is None else min(n, max_tracks)
    return off, nd, n, X, fl, P, rf, nt


def _finish(rf, nf, S, known, shared, good, zs, n_used, report, status, p):
    """rows from the counts and the per-frame depths, shared by neither form's arithmetic: integers and numpy.sort only.
    shared, good: callables row frame -> [nf]; zs: frame -> its depths; n_used: frame -> n_a"""
    R = len(rf)
    views = np.full((R, 1 + S), -1, dtype=np.int32)
    rng = np.full((R, 2), np.nan)
    pc = np.zeros((R, nf, 2), dtype=np.int32)
    st = np.zeros((R, 4), dtype=np.int32)
    for r, a in enumerate(rf):
        views[r, 0] = a
        if not (0 <= a < nf and known[a]):
            st[r, 3] = NOCAMERA
            continue
        sh, gd = shared(a), good(a)
        pc[r, :, 0], pc[r, :, 1] = sh, gd
        cand = [b for b in range(nf) if b != a and known[b] and sh[b] >= p["min_shared"]]
        cand.sort(key=lambda b: (-int(gd[b]), -int(sh[b]), b))
        src = cand[:S]
        views[r, 1:1 + len(src)] = src
        na = n_used(a)
        bitsv = 0
        if na < p["min_points"]:
            bitsv |= FEWPOINTS
        else:
            z = np.sort(np.asarray(zs(a), dtype=np.float64))
            i_near, i_far = ((na - 1) * p["q_near_pm"]) // 1000, ((na - 1) * p["q_far_pm"] + 999) // 1000
            with np.errstate(all="ignore"):
                rng[r] = z[i_near] / np.float64(p["grow"]), z[i_far] * np.float64(p["grow"])
            if np.isfinite(rng[r]).all():
                report[4] += 1
                if not rng[r, 0] < rng[r, 1]:
                    bitsv |= NARROW
        if len(src) < S:
            bitsv |= FEWVIEWS
        st[r] = na, len(cand), len(src), bitsv
        report[5] += len(src) == S
        report[6] += len(src) > 0
    return dict(views=views, range=rng, pair_counts=pc, ref_stats=st, report=np.array(report, dtype=np.int32), status=status)


def plan(offsets, nodes, xyz, flags, P, refs, S, max_tracks=None, max_nodes=None, **kw):
    """-> dict(views [R][1 + S], range [R][2], pair_counts [R][nf][2], ref_stats [R][4], report [8], status: the set of
    'cap' and 'node')"""
    p = dict(DEFAULTS, **kw)
    off, nd, n, X, fl, P, rf, nt = _inputs(offsets, nodes, xyz, flags, P, refs, max_tracks)
    nf = len(P)
    cap = len(nd) if max_nodes is None else max_nodes
    cmin2, cmax2 = cos2_of(p["min_angle_deg"]), cos2_of(p["max_angle_deg"])
    status = set(["cap"] if n > nt else [])
    known, _, _, C, sgn = consensus_frames(P)
    with np.errstate(all="ignore"):
        nrm = np.sqrt((P[:, 8] * P[:, 8] + P[:, 9] * P[:, 9]) + P[:, 10] * P[:, 10])
    o0, o1 = off[:nt], off[1:nt + 1]
    bad = (o0 < 0) | (o1 < o0) | (o1 > cap)
    if bad.any():
        status.add("node")
    lens = np.where(bad, 0, o1 - o0)
    used_t = np.isfinite(X[:nt]).all(1) & (True if fl is None else fl[:nt] == 0)
    # all nodes of the used tracks
    tid = np.repeat(np.arange(nt), np.where(used_t, lens, 0))
    start = np.cumsum(np.where(used_t, lens, 0)) - np.where(used_t, lens, 0)
    pos = np.arange(len(tid)) - start[tid]                      # position in the track
    f = nd[o0[tid] + pos, 0] if len(tid) else np.zeros(0, np.int64)
    inr = (f >= 0) & (f < nf)
    if (~inr).any():
        status.add("node")
    fc = np.where(inr, f, 0)
    Xn = X[tid]
    with np.errstate(all="ignore"):
        z = (sgn[fc] * (((P[fc, 8] * Xn[:, 0] + P[fc, 9] * Xn[:, 1]) + P[fc, 10] * Xn[:, 2]) + P[fc, 11])) / nrm[fc]
        used = inr & known[fc] & (z > 0)
    report = [nt, int(used_t.sum()), int(used.sum()), 0, 0, 0, 0, 0]
    # pairs, the tracks of one length at a time; counted in the rows that the references name
    rows_of = np.unique(rf[(rf >= 0) & (rf < nf)])
    ridx = np.full(nf, -1, dtype=np.int64)
    ridx[rows_of] = np.arange(len(rows_of))
    shared, good = np.zeros(len(rows_of) * nf, dtype=np.int64), np.zeros(len(rows_of) * nf, dtype=np.int64)
    first = start[used_t.nonzero()[0]]                          # a used track's first node in the lists above
    tl = lens[used_t]
    for L in np.unique(tl[tl >= 2]):
        L = int(L)
        iu, ju = np.triu_indices(L, 1)
        rows = first[tl == L]
        step = max(1, PAIR_CHUNK // len(iu))
        for c0 in range(0, len(rows), step):
            base = rows[c0:c0 + step, None]
            i, j = base + iu[None], base + ju[None]
            ok = used[i] & used[j] & (fc[i] != fc[j])
            i, j = i[ok], j[ok]
            a, b, Xp = fc[i], fc[j], Xn[i]
            with np.errstate(all="ignore"):
                ri, rj = C[a] - Xp, C[b] - Xp
                d = (ri[:, 0] * rj[:, 0] + ri[:, 1] * rj[:, 1]) + ri[:, 2] * rj[:, 2]
                na = (ri[:, 0] * ri[:, 0] + ri[:, 1] * ri[:, 1]) + ri[:, 2] * ri[:, 2]
                nb = (rj[:, 0] * rj[:, 0] + rj[:, 1] * rj[:, 1]) + rj[:, 2] * rj[:, 2]
                g = (d > 0) & (d * d <= cmin2 * (na * nb)) & (d * d >= cmax2 * (na * nb))
            report[3] += len(i)
            for tab, sel in ((shared, np.ones(len(i), bool)), (good, g)):
                for x, y in ((a, b), (b, a)):
                    m = sel & (ridx[x] >= 0)
                    k, c = np.unique(ridx[x[m]] * nf + y[m], return_counts=True)
                    tab[k] += c
    shared, good = shared.reshape(len(rows_of), nf), good.reshape(len(rows_of), nf)
    uf, uz = fc[used], z[used]
    return _finish(rf, nf, S, known, lambda a: shared[ridx[a]], lambda a: good[ridx[a]], lambda a: uz[uf == a],
                   lambda a: int((uf == a).sum()), report, status, p)


def _frame_loop(row):
    """one camera in Python floats -> (known, C (3), sgn, nrm)"""
    p = [float(x) for x in row]
    m00, m01, m02, m10, m11, m12, m20, m21, m22 = p[0], p[1], p[2], p[4], p[5], p[6], p[8], p[9], p[10]
    fin = all(math.isfinite(x) for x in p)
    if not fin:
        return False, None, 0.0, 0.0
    try:
        k = [[m11 * m22 - m12 * m21, m12 * m20 - m10 * m22, m10 * m21 - m11 * m20],
             [m02 * m21 - m01 * m22, m00 * m22 - m02 * m20, m01 * m20 - m00 * m21],
             [m01 * m12 - m02 * m11, m02 * m10 - m00 * m12, m00 * m11 - m01 * m10]]
        det = (m00 * k[0][0] + m01 * k[0][1]) + m02 * k[0][2]
    except OverflowError:          # Python raises where IEEE gives inf; no test camera comes here
        return False, None, 0.0, 0.0
    if det == 0.0:
        return False, None, 0.0, 0.0
    inv = [[k[c][r] / det for c in range(3)] for r in range(3)]
    C = [-((inv[r][0] * p[3] + inv[r][1] * p[7]) + inv[r][2] * p[11]) for r in range(3)]
    return True, C, (1.0 if det > 0.0 else -1.0), math.sqrt((m20 * m20 + m21 * m21) + m22 * m22)


def plan_loop(offsets, nodes, xyz, flags, P, refs, S, max_tracks=None, max_nodes=None, **kw):
    """plan() restated track by track; finite cameras whose products do not overflow"""
    p = dict(DEFAULTS, **kw)
    off, nd, n, X, fl, P, rf, nt = _inputs(offsets, nodes, xyz, flags, P, refs, max_tracks)
    nf = len(P)
    cap = len(nd) if max_nodes is None else max_nodes
    cmin2, cmax2 = cos2_of(p["min_angle_deg"]), cos2_of(p["max_angle_deg"])
    status = set(["cap"] if n > nt else [])
    cams = [_frame_loop(P[f]) for f in range(nf)]
    known = [c[0] for c in cams]
    shared = [[0] * nf for _ in range(nf)]
    good = [[0] * nf for _ in range(nf)]
    zs = [[] for _ in range(nf)]
    report = [nt, 0, 0, 0, 0, 0, 0, 0]
    for t in range(nt):
        o0, o1 = int(off[t]), int(off[t + 1])
        if o0 < 0 or o1 < o0 or o1 > cap:
            status.add("node")
            o1 = o0 = 0
        if fl is not None and fl[t] != 0:
            continue
        x = [float(v) for v in X[t]]
        if not all(math.isfinite(v) for v in x):
            continue
        report[1] += 1
        obs = []                                  # the used nodes: (frame, r, r . r)
        for o in range(o0, o1):
            f = int(nd[o, 0])
            if f < 0 or f >= nf:
                status.add("node")
                continue
            if not known[f]:
                continue
            _, C, sg, nrm = cams[f]
            q = [float(v) for v in P[f, 8:12]]
            z = (sg * (((q[0] * x[0] + q[1] * x[1]) + q[2] * x[2]) + q[3])) / nrm
            if not z > 0.0:
                continue
            zs[f].append(z)
            r = [C[0] - x[0], C[1] - x[1], C[2] - x[2]]
            obs.append((f, r, (r[0] * r[0] + r[1] * r[1]) + r[2] * r[2]))
        report[2] += len(obs)
        for i in range(len(obs)):
            for j in range(i + 1, len(obs)):
                (a, ri, na), (b, rj, nb) = obs[i], obs[j]
                if a == b:
                    continue
                d = (ri[0] * rj[0] + ri[1] * rj[1]) + ri[2] * rj[2]
                report[3] += 1
                shared[a][b] += 1
                shared[b][a] += 1
                if d > 0.0 and d * d <= cmin2 * (na * nb) and d * d >= cmax2 * (na * nb):
                    good[a][b] += 1
                    good[b][a] += 1
    return _finish(rf, nf, S, known, lambda a: shared[a], lambda a: good[a], lambda a: zs[a], lambda a: len(zs[a]), report, status, p)


def assert_equal(got, want, keys=("views", "range", "pair_counts", "ref_stats", "report")):
    """every integer and every bit"""
    for k in keys:
        g, w = np.ascontiguousarray(got[k]), np.ascontiguousarray(want[k])
        assert g.dtype == w.dtype and g.shape == w.shape, (k, g.dtype, w.dtype, g.shape, w.shape)
        assert g.view(np.uint8).tobytes() == w.view(np.uint8).tobytes(), (k, g, w)


# ---- scenes --------------------------------------------------------------------------------------------------------------

def look_at_camera(C, target, f=500.0, cx=320.0, cy=240.0):
    """K [R | -R C] [3][4] of a camera at C whose axis points at target"""
    C, target = np.asarray(C, dtype=np.float64), np.asarray(target, dtype=np.float64)
    z = (target - C) / np.linalg.norm(target - C)
    x = np.cross([0.0, 1.0, 0.0], z)
    x /= np.linalg.norm(x)
    R = np.stack([x, np.cross(z, x), z])
    K = np.array([[f, 0.0, cx], [0.0, f, cy], [0.0, 0.0, 1.0]])
    return K @ np.hstack([R, -(R @ C)[:, None]])


def random_graph(rng, nf, n_tracks, max_len, P, spread=1.0, centre=(0.0, 0.0, 5.0)):
    """tracks of 2 .. max_len nodes in distinct random frames, points around `centre` -> (offsets, nodes, xyz)"""
    lens = rng.integers(2, min(max_len, nf) + 1, n_tracks)
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    nd = np.zeros((off[-1], 2), dtype=np.int32)
    for t, L in enumerate(lens):
        nd[off[t]:off[t + 1], 0] = rng.permutation(nf)[:L]
    nd[:, 1] = rng.integers(0, 1000, len(nd))
    xyz = np.asarray(centre) + spread * rng.standard_normal((n_tracks, 3))
    return off, nd, xyz


def arc_cameras(angles_deg, radius=5.0, target=(0.0, 0.0, 0.0)):
    """cameras on a circle of `radius` around `target` in the x-z plane, at these angles, looking at it -> P [n][12]"""
    t = np.asarray(target, dtype=np.float64)
    return np.stack([look_at_camera(t + radius * np.array([math.sin(math.radians(a)), 0.0, -math.cos(math.radians(a))]), t).reshape(12)
                     for a in angles_deg])


def sparse_from_scene(sc, X, step=8):
    """A sparse model sampled from a rendered scene of depth_ref (sc: its dict; X [n][H][W][3] the world point of every pixel):
    every step-th pixel of every frame gives one track, whose nodes are the frames that see the point: it projects into the
    image and the depth rendered at that pixel is the point's to 1 % (it is not hidden).  A node's keypoint is the nearest
    pixel of the projection.  -> (offsets, nodes, xyz, kps: per frame [count][2] int (x, y))"""
    P = np.asarray(sc["P"], dtype=np.float64).reshape(-1, 3, 4)
    n, H, W = sc["ztrue"].shape
    off, nd, xyz, kps = [0], [], [], [[] for _ in range(n)]
    for r in range(n):
        for v in range(step // 2, H, step):
            for u in range(step // 2, W, step):
                x = X[r, v, u]
                seen = []
                for f in range(n):
                    q = P[f, :, :3] @ x + P[f, :, 3]
                    if q[2] <= 0:
                        continue
                    uu, vv = int(math.floor(q[0] / q[2] + 0.5)), int(math.floor(q[1] / q[2] + 0.5))
                    zt = q[2] / math.sqrt(P[f, 2, :3] @ P[f, 2, :3])
                    if 0 <= uu < W and 0 <= vv < H and abs(sc["ztrue"][f, vv, uu] - zt) <= 0.01 * zt:
                        seen.append((f, uu, vv))
                if len(seen) >= 2:
                    for f, uu, vv in seen:
                        nd.append((f, len(kps[f])))
                        kps[f].append((uu, vv))
                    off.append(len(nd))
                    xyz.append(x)
    return np.array(off, dtype=np.int32), np.array(nd, dtype=np.int32), np.array(xyz), [np.array(k, dtype=np.int64).reshape(-1, 2) for k in kps]


def scene_points(sc, centres, W, H, f):
    """the world point of every pixel of depth_ref.scene()'s frames (R = I, K = [f, f, W / 2, H / 2])"""
    v, u = np.mgrid[0:H, 0:W].astype(np.float64)
    d = np.stack([(u - W / 2) / f, (v - H / 2) / f, np.ones_like(u)], -1)
    return np.stack([np.asarray(C, dtype=np.float64) + sc["ztrue"][i][..., None] * d for i, C in enumerate(centres)])


def planes_of(z, zn, zf, D):
    """the plane coordinate of depth z in a sweep of D planes over 1/z in [1/zf, 1/zn]"""
    return (1.0 / z - 1.0 / zf) / (1.0 / zn - 1.0 / zf) * (D - 1)


def kernel_constants():
    """the launch constants of photogrammetry_amd/csrc/k_denseviews.hip, read from its source: name -> int"""
    import os
    import re
    import photogrammetry_amd._lib as L
    src = open(os.path.join(L.CSRC, "k_denseviews.hip")).read()
    return {m.group(1): int(m.group(2), 0) for m in re.finditer(r"constexpr int (DVW_\w+) = (\w+);", src)}


def mixed_graph(seed=5):
    """cameras on a rough ring around points near the origin, one of them unknown (NaN), one negated; tracks of 2 .. 9 nodes;
    flagged tracks, tracks with NaN points, a node in the unknown frame, a track that names one frame twice"""
    rng = np.random.default_rng(seed)
    nf = 9
    ang = np.linspace(-40, 40, nf) + rng.uniform(-2, 2, nf)
    P = arc_cameras(ang, radius=6.0)
    P[3] = -P[3]
    P[6] = np.nan
    off, nd, xyz = random_graph(rng, nf, 160, 9, P, spread=0.5, centre=(0.0, 0.0, 0.0))
    flags = (rng.random(160) < 0.1).astype(np.int32) * 2
    xyz[rng.random(160) < 0.05, 1] = np.nan
    xyz[7] = [0.0, 0.0, -50.0]                      # behind every camera
    t = int(np.flatnonzero((np.diff(off) >= 4) & (flags == 0) & np.isfinite(xyz).all(1))[0])
    nd[off[t] + 1, 0] = nd[off[t], 0]               # one frame twice
    return off, nd, xyz, flags, P
