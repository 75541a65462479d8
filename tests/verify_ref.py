"""float64 restatement of two-view verification by epipolar RANSAC (include/pgx.h, "two-view geometric verification"): the
yardstick of tests/test_gpu_verify.py.  Candidates, the sampler (ransac_ref), the normalised 8-point fit with
rank 2 enforced (numpy's eigh in place of the kernel's Jacobi solver, the same sign rule), the inlier predicate in exactly
the header's order of operations (numpy float64 reproduces the device's bits from the same F), winner, refit and outputs.
tests/test_verify_ref.py ties this file to the truth."""
import numpy as np

from ransac_ref import M64, draw, splitmix64, stream_seed

FEWMATCHES, NOMODEL, FEWINLIERS = 1, 2, 4
DIST_NONE = 2**31 - 1


def candidates(kpa, kpb, ca, cb, ml, stride, max_dist):
    """ml: [stride][3] (k1, k2, dist) of one pair; kpa, kpb: [>= count][2] (x, y); ca, cb the raw counts
    -> (entries [n] in list order, pa [n][2], pb [n][2], rows: the number of entries the stage looks at)"""
    ca, cb = min(max(int(ca), 0), stride), min(max(int(cb), 0), stride)
    m = np.asarray(ml)[:ca].astype(np.int64)
    ok = (m[:, 0] >= 0) & (m[:, 0] < ca) & (m[:, 1] >= 0) & (m[:, 1] < cb) & (m[:, 2] <= max_dist) & (m[:, 2] != DIST_NONE)
    e = np.flatnonzero(ok)
    pa = np.asarray(kpa, np.float64).reshape(-1, 2)[m[e, 0]] if len(e) else np.zeros((0, 2))
    pb = np.asarray(kpb, np.float64).reshape(-1, 2)[m[e, 1]] if len(e) else np.zeros((0, 2))
    return e, pa, pb, ca


def sample(seed, a, b, s, n):
    """the 8 distinct positions of sample s of the pair in slots (a, b) with n candidates"""
    return draw(stream_seed(seed, a, s) ^ (((b & 0xFFFFFFFF) * 0x9E3779B97F4A7C15) & M64), n, 8)


def _smallest(A, gaps=None):
    """eigenvector of the smallest eigenvalue, largest component positive; gaps (a list) receives the distance of the two
    smallest eigenvalues over the largest: what the vector's conditioning depends on"""
    w, V = np.linalg.eigh(A)
    if gaps is not None:
        gaps.append((w[1] - w[0]) / w[-1])
    v = V[:, 0]
    return -v if v[np.argmax(np.abs(v))] < 0 else v


def _norm(p):
    c = p.mean(0)
    d = np.sqrt(((p - c) ** 2).sum(1)).mean()
    if not d > 0:
        return None
    sc = np.sqrt(2.0) / d
    return np.array([[sc, 0.0, -sc * c[0]], [0.0, sc, -sc * c[1]], [0.0, 0.0, 1.0]])


def fit(pa, pb, gaps=None):
    """the normalised 8-point fit with rank 2 enforced on the correspondences pa[i] <-> pb[i] -> F [3][3] with unit Frobenius
    norm, h_a^T F h_b = 0; None when the set is invalid.  gaps (a list) receives the relative eigenvalue gaps of the two
    eigen-solves (_smallest)"""
    pa, pb = np.asarray(pa, np.float64), np.asarray(pb, np.float64)
    Ta, Tb = _norm(pa), _norm(pb)
    if Ta is None or Tb is None:
        return None
    ha = np.c_[pa, np.ones(len(pa))] @ Ta.T
    hb = np.c_[pb, np.ones(len(pb))] @ Tb.T
    A = np.einsum("ni,nj->nij", ha, hb).reshape(-1, 9)
    with np.errstate(all="ignore"):
        G = A.T @ A
        if not np.isfinite(G).all():
            return None
        Fh = _smallest(G, gaps).reshape(3, 3)
        v3 = _smallest(Fh.T @ Fh, gaps)
        Fh = Fh - np.outer(Fh @ v3, v3)
        F = Ta.T @ Fh @ Tb
        F = F / np.sqrt((F * F).sum())
    return F if np.isfinite(F).all() else None


def predicate(F, pa, pb, inlier_px):
    """the inlier predicate in the header's order -> bool [n]"""
    F = np.asarray(F, np.float64).reshape(3, 3)
    x, y, u, v = pa[:, 0], pa[:, 1], pb[:, 0], pb[:, 1]
    with np.errstate(all="ignore"):
        m0 = (F[0, 0] * u + F[0, 1] * v) + F[0, 2]
        m1 = (F[1, 0] * u + F[1, 1] * v) + F[1, 2]
        m2 = (F[2, 0] * u + F[2, 1] * v) + F[2, 2]
        e = (x * m0 + y * m1) + m2
        l0 = (F[0, 0] * x + F[1, 0] * y) + F[2, 0]
        l1 = (F[0, 1] * x + F[1, 1] * y) + F[2, 1]
        d = ((l0 * l0 + l1 * l1) + m0 * m0) + m1 * m1
        T = np.float64(inlier_px) * np.float64(inlier_px)
        return (d > 0) & (e * e <= T * d)


def refit(F, cur, pa, pb, inlier_px, refit_iters):
    """the refit loop from the F whose inlier count is cur -> (F, count, refits kept)"""
    kept = 0
    for _ in range(refit_iters):
        if cur < 8:
            break
        I = predicate(F, pa, pb, inlier_px)
        Fn = fit(pa[I], pb[I])
        if Fn is None:
            break
        c = int(predicate(Fn, pa, pb, inlier_px).sum())
        if c <= cur:
            break
        F, cur, kept = Fn, c, kept + 1
    return F, cur, kept


def verify_pair(kpa, kpb, ca, cb, ml, a, b, stride, max_dist, n_samples, inlier_px, min_inliers, refit_iters, seed):
    """One pair -> dict(out [rows][3], F [9], stats [8], inlier [rows], sample_F [n_samples][9], sample_count [n_samples])"""
    ml = np.asarray(ml).astype(np.int64)
    e, pa, pb, rows = candidates(kpa, kpb, ca, cb, ml, stride, max_dist)
    n = len(e)
    sF = np.full((n_samples, 9), np.nan)
    sc = np.full(n_samples, -1, np.int64)
    flags, win, wcount, fin, kept = 0, -1, 0, 0, 0
    F = np.full(9, np.nan)
    if n < 8:
        flags = FEWMATCHES
    else:
        for s in range(n_samples):
            ids = sample(seed, a, b, s, n)
            Fs = fit(pa[ids], pb[ids])
            if Fs is None:
                continue
            sF[s] = Fs.reshape(9)
            sc[s] = int(predicate(Fs, pa, pb, inlier_px).sum())
        if (sc >= 0).any():
            win = int(np.argmax(sc))          # the first maximum
            wcount = int(sc[win])
            Ff, fin, kept = refit(sF[win].reshape(3, 3), wcount, pa, pb, inlier_px, refit_iters)
            F = np.asarray(Ff).reshape(9)
            if fin < min_inliers:
                flags |= FEWINLIERS
        else:
            flags = NOMODEL
    inl = np.full(rows, -1, np.int64)
    if n:
        inl[e] = predicate(F, pa, pb, inlier_px).astype(np.int64) if win >= 0 else 0
    out = ml[:rows].copy()
    rej = ~((inl == 1) & (flags == 0))
    out[rej, 1] = -1
    out[rej, 2] = DIST_NONE
    stats = np.array([n, wcount, fin, win, flags, kept, int((sc >= 0).sum()), 0], np.int64)
    return dict(out=out, F=F, stats=stats, inlier=inl, sample_F=sF, sample_count=sc, entries=e, pa=pa, pb=pb)


def verify(kps, counts, pairlist, matches, stride, max_dist, n_samples, inlier_px, min_inliers, refit_iters, seed):
    """kps: per slot [n][2] (x, y); matches [M][stride][3] -> (list of verify_pair results, report [8])"""
    res = []
    for m, (a, b) in enumerate(pairlist):
        res.append(verify_pair(kps[a], kps[b], counts[a], counts[b], matches[m], a, b, stride, max_dist, n_samples, inlier_px,
                               min_inliers, refit_iters, seed))
    return res, report([r["stats"] for r in res])


def report(stats):
    st = np.asarray(stats, np.int64).reshape(-1, 8)
    ok = st[:, 4] == 0
    return np.array([len(st), ok.sum(), ((st[:, 4] & 1) != 0).sum(), ((st[:, 4] & 2) != 0).sum(), ((st[:, 4] & 4) != 0).sum(),
                     st[:, 0].sum(), st[ok, 2].sum(), 0], np.int64)


def epipolar_distance(F, pa, pb):
    """distance in pixels of pa from the line F h_b, and of pb from the line F^T h_a -> ([n], [n])"""
    F = np.asarray(F, np.float64).reshape(3, 3)
    ha, hb = np.c_[pa, np.ones(len(pa))], np.c_[pb, np.ones(len(pb))]
    la, lb = hb @ F.T, ha @ F
    e = (ha * la).sum(1)
    return np.abs(e) / np.hypot(la[:, 0], la[:, 1]), np.abs(e) / np.hypot(lb[:, 0], lb[:, 1])


def scene_pair(seed, n_true, n_junk, n_points=900, frames=(1, 3)):
    """A two-view case from synth.make_scene (pinhole f = 1200, 1920 x 1080, integer-rounded keypoints, 6 cameras on an arc):
    the match list of frames (a, b) holds n_true true correspondences (dist 10) and n_junk junk ones (dist 20: keypoints of a
    with no true row, each linked to a random keypoint of b that is not its own point's), shuffled and
    followed by the (0, 0, PGX_DIST_NONE) tail up to stride = the largest count.
    -> dict(kps [6] of [n][2] float64, counts [6], a, b, stride, ml [stride][3], true [stride] bool, junk [stride] bool, uv_a, uv_b (unrounded, per row of the
    true matches in list order), K [3][3], R, t (x_b ~ K (R X + t) for x_a ~ K X))"""
    from photogrammetry_amd import synth
    rng = np.random.default_rng(seed)
    s = synth.make_scene(n_points, 6, seed=seed)
    a, b = frames
    pa, pb = s["point_id"][a], s["point_id"][b]
    where = np.full(n_points, -1, np.int64)
    where[pb] = np.arange(len(pb))
    common = np.flatnonzero(where[pa] >= 0)
    assert len(common) >= n_true and len(pa) >= n_true + n_junk, (len(common), len(pa))
    tk1 = common[rng.permutation(len(common))[:n_true]]
    rest = np.setdiff1d(np.arange(len(pa)), tk1)
    jk1 = rest[rng.permutation(len(rest))[:n_junk]]
    jk2 = rng.integers(0, len(pb) - 1, n_junk)
    own = where[pa[jk1]]
    jk2 = jk2 + ((own >= 0) & (jk2 >= own))
    ml = np.concatenate([np.stack([tk1, where[pa[tk1]], np.full(n_true, 10)], 1), np.stack([jk1, jk2, np.full(n_junk, 20)], 1)])
    true = np.arange(len(ml)) < n_true
    order = rng.permutation(len(ml))
    stride = int(s["counts"].max())
    pad = stride - len(ml)
    ml = np.concatenate([ml[order], np.tile([0, 0, DIST_NONE], (pad, 1))]).astype(np.int32)
    true = np.concatenate([true[order], np.zeros(pad, bool)])
    kps = [np.stack([k["x"], k["y"]], 1).astype(np.float64) for k in s["kps"]]
    Ra, ta = s["Rt"][a, :9].reshape(3, 3), s["Rt"][a, 9:]
    Rb, tb = s["Rt"][b, :9].reshape(3, 3), s["Rt"][b, 9:]
    R = Rb @ Ra.T
    Kf = s["K"][a]
    K = np.array([[Kf[0], 0.0, Kf[2]], [0.0, Kf[1], Kf[3]], [0.0, 0.0, 1.0]])
    return dict(kps=kps, counts=s["counts"].copy(), a=a, b=b, stride=stride, ml=ml, true=true, junk=~true & (ml[:, 2] == 20), uv_a=s["uv"][a][ml[true, 0]],
                uv_b=s["uv"][b][ml[true, 1]], K=K, R=R, t=tb - R @ ta, scene=s)
