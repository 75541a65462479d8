"""float64 restatement of the start of a reconstruction (include/pgx.h, "relative pose per image pair and the choice of the
initial pair"): the yardstick of tests/test_gpu_init_pair.py.  Candidates (verify_ref's), E = K_a^T F K_b in the header's order
of operations, the decomposition with numpy's SVD in place of the kernel's Jacobi solve (the four candidates agree as a set:
U W V^T does not change when a singular pair changes sign, and t only changes sign), the score in exactly the header's order
(numpy float64 reproduces the device's bits from the same R and t), the winner, the flags, the choice over the pairs and the
per-frame outputs.  tests/test_init_pair_ref.py ties this file to the truth."""
import math

import numpy as np

from verify_ref import DIST_NONE, candidates  # noqa: F401

SKIPPED, BADINPUT, DEGENERATE, FEWFRONT, FEWPOINTS = 1, 2, 4, 8, 16
NAN12 = np.full(12, np.nan)


def cos2_of(min_angle_deg):
    c = math.cos(min_angle_deg * (math.pi / 180))
    return c * c


def bearings(p, K):
    """p [n][2] pixels (x, y), K = (fx, fy, cx, cy) -> (g [n][3] = ((x - cx) fy, (y - cy) fx, fx fy), s = fx fy); no division"""
    fx, fy, cx, cy = (np.float64(v) for v in K)
    p = np.asarray(p, np.float64).reshape(-1, 2)
    s = fx * fy
    return np.stack([(p[:, 0] - cx) * fy, (p[:, 1] - cy) * fx, np.full(len(p), s)], 1), s


def essential(F, Ka, Kb):
    """Gh = G / |G|, G = (K_a^T F K_b)^T, in the header's order [3][3]"""
    F = np.asarray(F, np.float64).reshape(3, 3)
    fxa, fya, cxa, cya = (np.float64(v) for v in Ka)
    fxb, fyb, cxb, cyb = (np.float64(v) for v in Kb)
    with np.errstate(all="ignore"):
        A = np.stack([fxa * F[0], fya * F[1], (cxa * F[0] + cya * F[1]) + F[2]])
        E = np.stack([A[:, 0] * fxb, A[:, 1] * fyb, (A[:, 0] * cxb + A[:, 1] * cyb) + A[:, 2]], 1)
        G = E.T
        nn = np.float64(0.0)
        for v in G.reshape(9):
            nn = nn + v * v
        return G / np.sqrt(nn)


def decompose(Gh):
    """-> (cands [4][12] = (R1, t), (R1, -t), (R2, t), (R2, -t), sigma_2 / sigma_1, sigma [3]); cands None when DEGENERATE"""
    if not np.isfinite(Gh).all():
        return None, np.nan, None
    U, S, Vt = np.linalg.svd(Gh)
    sig = S[1] / S[0]
    if not S[1] > 1e-6 * S[0]:
        return None, sig, S
    u1, u2, v1, v2 = U[:, 0], U[:, 1], Vt[0], Vt[1]
    u3, v3 = np.cross(u1, u2), np.cross(v1, v2)
    R1 = np.outer(u2, v1) - np.outer(u1, v2) + np.outer(u3, v3)
    R2 = np.outer(u1, v2) - np.outer(u2, v1) + np.outer(u3, v3)
    c = np.stack([np.r_[R1.reshape(9), u3], np.r_[R1.reshape(9), -u3], np.r_[R2.reshape(9), u3], np.r_[R2.reshape(9), -u3]])
    return (c if np.isfinite(c).all() else None), sig, S


def _dot(a, b):
    return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]


def score(Rt, ga, gb, sa, sb, cos2):
    """One candidate on n matches, in the header's order -> (front [n] bool, wide [n] bool)"""
    Rt = np.asarray(Rt, np.float64).reshape(12)
    R, t = Rt[:9], Rt[9:]
    a, b = (ga[:, 0], ga[:, 1], ga[:, 2]), (gb[:, 0], gb[:, 1], gb[:, 2])
    with np.errstate(all="ignore"):
        p = (_dot(R[0:3], a), _dot(R[3:6], a), _dot(R[6:9], a))
        a11 = _dot(p, p)
        c = _dot(p, b)
        a12 = -c
        a22 = _dot(b, b)
        r1 = -_dot(p, t)
        r2 = _dot(b, t)
        det = a11 * a22 - a12 * a12
        na = r1 * a22 - a12 * r2
        nb = a11 * r2 - a12 * r1
        front = (det > 0) & (na * sa > 0) & (nb * sb > 0)
        wide = front & (((c * sa) * sb <= 0) | (c * c <= np.float64(cos2) * (a11 * a22)))
    return front, wide


def relative_pose(kpa, kpb, ca, cb, ml, stride, max_dist, F, Ka, Kb, min_angle_deg, min_front_frac, min_points, cands=None):
    """One pair that is not SKIPPED.  cands [4][12]: score these (the device's) instead of this file's decomposition; a
    non-finite cands means DEGENERATE.  -> dict(Rt [12], stats [8], sigma, cand_Rt [4][12], front [4][n], wide [4][n])"""
    F, Ka, Kb = np.asarray(F, np.float64).reshape(9), np.asarray(Ka, np.float64), np.asarray(Kb, np.float64)
    e, pa, pb, _ = candidates(kpa, kpb, ca, cb, ml, stride, max_dist)
    n = len(e)
    nan = dict(Rt=NAN12.copy(), sigma=np.nan, cand_Rt=np.full((4, 12), np.nan), front=None, wide=None)
    if not (np.isfinite(F).all() and np.isfinite(Ka).all() and np.isfinite(Kb).all() and Ka[0] != 0 and Ka[1] != 0 and Kb[0] != 0
            and Kb[1] != 0):
        return dict(nan, stats=np.array([n, 0, 0, 0, 0, 0, -1, BADINPUT], np.int64))
    sig = np.nan
    if cands is None:
        cands, sig, _ = decompose(essential(F, Ka, Kb))
    elif not np.isfinite(cands).all():
        cands = None
    if cands is None:
        return dict(nan, sigma=sig, stats=np.array([n, 0, 0, 0, 0, 0, -1, DEGENERATE], np.int64))
    cands = np.asarray(cands, np.float64).reshape(4, 12)
    ga, sa = bearings(pa, Ka)
    gb, sb = bearings(pb, Kb)
    fw = [score(c, ga, gb, sa, sb, cos2_of(min_angle_deg)) for c in cands]
    front = np.array([int(f.sum()) for f, _ in fw])
    win = int(np.argmax(front))                       # the first maximum
    wide = int(fw[win][1].sum())
    flags = 0
    if float(front[win]) < np.float64(min_front_frac) * np.float64(n):
        flags |= FEWFRONT
    if wide < min_points:
        flags |= FEWPOINTS
    return dict(Rt=cands[win].copy(), sigma=sig, cand_Rt=cands, stats=np.array([n, *front, wide, win, flags], np.int64),
                front=np.stack([f for f, _ in fw]), wide=np.stack([w for _, w in fw]))


def frame_of(frame_ids, slot, F, n_frames):
    """the frame number of a slot, -1 when the slot or its frame is outside the call"""
    if not 0 <= slot < F:
        return -1
    f = slot if frame_ids is None else int(frame_ids[slot])
    return f if 0 <= f < n_frames else -1


def choose(stats, fa, fb):
    """stats [M][8], fa / fb [M] frame numbers -> m* or -1: flags 0, the most wide points, then the smaller frame of a, of b,
    the smaller m"""
    best, key = -1, None
    for m, st in enumerate(np.asarray(stats).reshape(-1, 8)):
        if st[7] != 0:
            continue
        k = (-int(st[5]), int(fa[m]), int(fb[m]), m)
        if key is None or k < key:
            best, key = m, k
    return best


def report(stats, ms):
    st = np.asarray(stats, np.int64).reshape(-1, 8)
    fl = st[:, 7]
    return np.array([len(st), (fl == 0).sum(), ((fl & (SKIPPED | BADINPUT)) != 0).sum(), ((fl & DEGENERATE) != 0).sum(),
                     ((fl & FEWFRONT) != 0).sum(), ((fl & FEWPOINTS) != 0).sum(), ms, st[ms, 5] if ms >= 0 else 0], np.int64)


def make_P(k, rt):
    """K [R | t] with the rows bundle adjustment writes"""
    r = np.asarray(rt, np.float64)
    M = np.concatenate([r[:9].reshape(3, 3), r[9:, None]], 1)
    return np.stack([k[0] * M[0] + k[2] * M[2], k[1] * M[1] + k[3] * M[2], M[2]]).reshape(12)


def frame_outputs(ms, fa, fb, Rt_pair, K, frame_ids, F, n_frames):
    """-> (Rt_out [n_frames][12], P_out, fixed_out [n_frames], register_out [n_frames]) for the chosen pair ms (or -1)"""
    K = np.asarray(K, np.float64).reshape(n_frames, 4)
    Rt, P = np.full((n_frames, 12), np.nan), np.full((n_frames, 12), np.nan)
    fixed, reg = np.zeros(n_frames, np.int64), np.zeros(n_frames, np.int64)
    if ms < 0:
        return Rt, P, fixed, reg
    a, b = int(fa[ms]), int(fb[ms])
    Rt[a] = np.r_[np.eye(3).reshape(9), np.zeros(3)]
    Rt[b] = np.asarray(Rt_pair)[ms]
    P[a], P[b] = make_P(K[a], Rt[a]), make_P(K[b], Rt[b])
    fixed[a] = 1
    for s in range(F):
        f = frame_of(frame_ids, s, F, n_frames)
        if f >= 0 and f != a and f != b:
            reg[f] = 1
    return Rt, P, fixed, reg


def init_pair(kps, counts, pairlist, matches, stride, max_dist, Fs, K, min_angle_deg, min_front_frac, min_points, frame_ids=None,
              n_frames=None, cands=None):
    """kps: per slot [n][2] (x, y); counts [F] by slot; pairlist [M][2] slots; matches [M][stride][3]; Fs [M][9]; K
    [n_frames][4] by frame number; cands [M][4][12] or None (relative_pose).
    -> dict(Rt_pair [M][12], stats [M][8], sigma [M], cand_Rt [M][4][12], fa, fb [M], ms, Rt_out, P_out, fixed_out,
    register_out, report [8], pairs: relative_pose's results (None for a SKIPPED pair))"""
    F = len(counts)
    nf = F if n_frames is None else n_frames
    K = np.asarray(K, np.float64).reshape(nf, 4)
    M = len(pairlist)
    Rt_pair, stats, sigma = np.full((M, 12), np.nan), np.zeros((M, 8), np.int64), np.full(M, np.nan)
    cand_Rt = np.full((M, 4, 12), np.nan)
    fa, fb, res = np.full(M, -1), np.full(M, -1), []
    for m, (a, b) in enumerate(pairlist):
        a, b = int(a), int(b)
        fa[m], fb[m] = frame_of(frame_ids, a, F, nf), frame_of(frame_ids, b, F, nf)
        if fa[m] < 0 or fb[m] < 0 or a == b:
            fa[m] = fb[m] = -1
            stats[m] = [0, 0, 0, 0, 0, 0, -1, SKIPPED]
            res.append(None)
            continue
        r = relative_pose(kps[a], kps[b], counts[a], counts[b], matches[m], stride, max_dist, Fs[m], K[fa[m]], K[fb[m]],
                          min_angle_deg, min_front_frac, min_points, None if cands is None else cands[m])
        Rt_pair[m], stats[m], sigma[m], cand_Rt[m] = r["Rt"], r["stats"], r["sigma"], r["cand_Rt"]
        res.append(r)
    ms = choose(stats, fa, fb)
    Rt_out, P_out, fixed, reg = frame_outputs(ms, fa, fb, Rt_pair, K, frame_ids, F, nf)
    return dict(Rt_pair=Rt_pair, stats=stats, sigma=sigma, cand_Rt=cand_Rt, fa=fa, fb=fb, ms=ms, Rt_out=Rt_out, P_out=P_out,
                fixed_out=fixed, register_out=reg, report=report(stats, ms), pairs=res)


def same_set(ca, cb):
    """the largest entry difference between two sets of four candidates under the best assignment"""
    ca, cb = np.asarray(ca).reshape(4, 12), np.asarray(cb).reshape(4, 12)
    d = np.abs(ca[:, None, :] - cb[None, :, :]).max(2)
    import itertools
    return min(max(d[i, p[i]] for i in range(4)) for p in itertools.permutations(range(4)))


def pose_errors(Rt, R_true, t_true):
    """(rotation error, translation-direction error) in degrees of Rt [12] against the truth"""
    Rt = np.asarray(Rt, np.float64)
    R, t = Rt[:9].reshape(3, 3), Rt[9:]
    cr = (np.trace(R @ np.asarray(R_true).T) - 1.0) / 2.0
    ct = float(t @ t_true) / (np.linalg.norm(t) * np.linalg.norm(t_true))
    return math.degrees(math.acos(min(1.0, max(-1.0, cr)))), math.degrees(math.acos(min(1.0, max(-1.0, ct))))


# ---- cases that tests/test_init_pair_ref.py and tests/test_gpu_init_pair.py share ----------------------------------------------

VER = dict(max_dist=64, n_samples=256, inlier_px=1.5, min_inliers=24, refit_iters=2, seed=7)    # verification ahead of the stage


def rotation_pair(seed=1, n=500, deg=10.0):
    """Two views from ONE centre, the second turned by `deg` about the y axis: pinhole (1200, 1200, 960, 540), points in
    [-3, 3] x [-2, 2] x [4, 9], integer-rounded keypoints seen in both 1920 x 1080 images, an identity match list (dist 5).
    -> (pa [m][2], pb [m][2], ml [m][3], K [4])"""
    from photogrammetry_amd import synth
    rng = np.random.default_rng(seed)
    K = np.array([1200.0, 1200.0, 960.0, 540.0])
    X = np.c_[rng.uniform(-3, 3, n), rng.uniform(-2, 2, n), rng.uniform(4, 9, n)]

    def proj(Y):
        return np.round(np.stack([K[0] * Y[:, 0] / Y[:, 2] + K[2], K[1] * Y[:, 1] / Y[:, 2] + K[3]], 1))
    pa, pb = proj(X), proj(X @ synth.rot_y(np.radians(deg)).T)
    ok = ((pa >= 0) & (pa < [1920, 1080]) & (pb >= 0) & (pb < [1920, 1080])).all(1)
    pa, pb = pa[ok], pb[ok]
    m = len(pa)
    return pa, pb, np.stack([np.arange(m), np.arange(m), np.full(m, 5)], 1).astype(np.int32), K


def scene6():
    """synth.make_scene(600, 6, seed=2) with the lists of all 15 pairs a < b, a fifth of the true rows relinked, and the
    yardstick's verification of them (computed once per process).
    -> dict(scene, pairs, stride, kps [6] of [n][2] float64, counts, ml [15][stride][3], out (verified lists), F [15][9])"""
    if "s6" not in _cache:
        import verify_ref
        from photogrammetry_amd import synth
        pairs = [(a, b) for a in range(6) for b in range(a + 1, 6)]
        s = synth.make_scene(600, 6, seed=2, pairs=pairs, wrong_rate=0.2)
        stride = int(s["counts"].max())
        ml = np.zeros((len(pairs), stride, 3), np.int32)
        ml[:, :, 2] = DIST_NONE
        for m, l in enumerate(s["lists"]):
            ml[m, :len(l)] = np.stack([l["k1"], l["k2"], l["dist"]], 1)
        kps = [np.stack([k["x"], k["y"]], 1).astype(np.float64) for k in s["kps"]]
        res, _ = verify_ref.verify(kps, s["counts"], pairs, ml, stride, VER["max_dist"], VER["n_samples"], VER["inlier_px"],
                                   VER["min_inliers"], VER["refit_iters"], VER["seed"])
        out = ml.copy()
        for m, r in enumerate(res):
            out[m, :len(r["out"])] = r["out"]
        _cache["s6"] = dict(scene=s, pairs=pairs, stride=stride, kps=kps, counts=s["counts"].astype(np.int32), ml=ml, out=out,
                            F=np.stack([r["F"] for r in res]))
    return _cache["s6"]


_cache = {}

# the chain after the stage: triangulation gates, bundle adjustment and registration settings shared by the device chain of
# tests/test_gpu_init_pair.py and the yardstick chain below
CHAIN = dict(min_parallax_deg=1.0, max_reproj_px=2.0, tri_iters=10, ba_iters=20, huber_px=float("inf"), lambda0=1e-3,
             reg_samples=256, reg_inlier_px=2.0, reg_min_inliers=12, reg_iters=10, reg_seed=7)


def chain(kps, K, offsets, nodes, Rt0, P0, fixed, reg):
    """The yardstick chain from the stage's per-frame outputs: triangulate on P0 -> bundle adjustment with `fixed` ->
    triangulate -> register the frames of `reg` -> triangulate -> bundle adjustment of all frames.
    -> dict(Rt [F][12], node_err, flags: the last triangulation's, xyz)"""
    import bundle_ref
    import register_ref
    import triangulate_ref
    c = CHAIN

    def tri(P):
        return triangulate_ref.triangulate(kps, P, offsets, nodes, c["min_parallax_deg"], c["max_reproj_px"], c["tri_iters"])

    def ba(Rt, fx, t):
        return bundle_ref.bundle_adjust(kps, K, Rt, fx, offsets, nodes, t["xyz"], t["flags"], c["ba_iters"], c["huber_px"], c["lambda0"])
    t1 = tri(P0)
    b1 = ba(Rt0, fixed, t1)
    t2 = tri(b1["P"])
    r = register_ref.register(kps, K, b1["Rt"], reg, offsets, nodes, t2["xyz"], t2["flags"], c["reg_samples"], c["reg_inlier_px"],
                              c["reg_min_inliers"], c["reg_iters"], c["reg_seed"])
    t3 = tri(r["P"])
    b2 = ba(r["Rt"], fixed, t3)
    return dict(Rt=b2["Rt"], node_err=b2["node_err"], flags=t3["flags"], xyz=b2["xyz"], steps=(t1, b1, t2, r, t3, b2))


def centre_error(Rt, centres):
    """the largest distance between the camera centres of Rt [F][12] and `centres` after the least-squares similarity
    (Umeyama) that maps the former onto the latter"""
    Rt = np.asarray(Rt, np.float64).reshape(-1, 12)
    C = np.stack([-r[:9].reshape(3, 3).T @ r[9:] for r in Rt])
    D = np.asarray(centres, np.float64)
    mc, md = C.mean(0), D.mean(0)
    Cc, Dc = C - mc, D - md
    U, S, Vt = np.linalg.svd(Dc.T @ Cc / len(C))
    d = np.diag([1.0, 1.0, np.sign(np.linalg.det(U) * np.linalg.det(Vt))])
    R = U @ d @ Vt
    s = np.trace(np.diag(S) @ d) / (Cc ** 2).sum() * len(C)
    return float(np.linalg.norm(s * Cc @ R.T - Dc, axis=1).max())
