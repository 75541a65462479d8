"""float64 restatement of frame registration by P3P RANSAC (include/pgx.h, "frame registration"): the yardstick of
tests/test_gpu_register.py.  P3P and the sampler are scalar Python floats in the kernel's order of operations (IEEE
doubles, no fused multiply-add), the inlier predicate and the Gauss-Newton sums are numpy over the correspondences;
tests/test_register_ref.py ties this file to the truth.  Besides the outputs it returns every correspondence's predicate
margin at the final pose, so that a test can leave out correspondences that lie within rounding of the threshold."""
import math

import numpy as np

from ransac_ref import M64, draw, splitmix64, stream_seed

BADK, FEWPOINTS, NOSOLUTION, FEWINLIERS = 1, 2, 4, 8


def sample(seed, frame, s, n):
    """the three distinct positions of sample s of a frame with n correspondences"""
    return draw(stream_seed(seed, frame, s), n, 3)


def _det3c(a, b, c):
    return (a[0] * (b[1] * c[2] - b[2] * c[1]) - b[0] * (a[1] * c[2] - a[2] * c[1])) + c[0] * (a[1] * b[2] - a[2] * b[1])


def _cubic_root(b, c, d):
    disc = b * b - 3.0 * c
    m = -b / 3.0
    if disc >= 0.0:
        m = (-b + math.sqrt(disc)) / 3.0
    fm = ((m + b) * m + c) * m + d
    bound = 1.0 + max(abs(b), max(abs(c), abs(d)))
    right = fm <= 0.0
    x = bound if right else -bound
    for _ in range(200):
        f = ((x + b) * x + c) * x + d
        fp = (3.0 * x + 2.0 * b) * x + c
        try:
            xn = x - f / fp
        except ZeroDivisionError:
            break
        if not (xn < x if right else xn > x):
            break
        x = xn
    return x


def _div(a, b):
    """IEEE division (inf / NaN where Python raises)"""
    with np.errstate(all="ignore"):
        return float(np.float64(a) / np.float64(b))


def _sqrt(x):
    return math.sqrt(x) if x >= 0.0 else float("nan")


def _cross(a, b):
    return [a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]]


def _null_vec(M, sig):
    r0 = [M[0][0] - sig, M[0][1], M[0][2]]
    r1 = [M[1][0], M[1][1] - sig, M[1][2]]
    r2 = [M[2][0], M[2][1], M[2][2] - sig]
    best, n = None, None
    for c in (_cross(r0, r1), _cross(r0, r2), _cross(r1, r2)):
        nc = (c[0] * c[0] + c[1] * c[1]) + c[2] * c[2]
        if best is None or nc > n:
            best, n = c, nc
    s = _sqrt(n)
    return [_div(v, s) for v in best]


def _lam_res(l, a12, a13, a23, b12, b13, b23):
    F = [((l[0] * l[0] + l[1] * l[1]) + b12 * (l[0] * l[1])) - a12,
         ((l[0] * l[0] + l[2] * l[2]) + b13 * (l[0] * l[2])) - a13,
         ((l[1] * l[1] + l[2] * l[2]) + b23 * (l[1] * l[2])) - a23]
    return (F[0] * F[0] + F[1] * F[1]) + F[2] * F[2], F


def p3p(y, X):
    """Lambda Twist on unit bearings y[3][3] and points X[3][3] -> list of 4 slots, each (R [9], t [3]) or None"""
    y = [[float(v) for v in r] for r in y]
    X = [[float(v) for v in r] for r in X]
    dot = lambda p, q: (p[0] * q[0] + p[1] * q[1]) + p[2] * q[2]  # noqa: E731
    b12, b13, b23 = -2.0 * dot(y[0], y[1]), -2.0 * dot(y[0], y[2]), -2.0 * dot(y[1], y[2])
    d12 = [X[0][k] - X[1][k] for k in range(3)]
    d13 = [X[0][k] - X[2][k] for k in range(3)]
    d23 = [X[1][k] - X[2][k] for k in range(3)]
    a12, a13, a23 = dot(d12, d12), dot(d13, d13), dot(d23, d23)
    A = [[a23, a23 * (0.5 * b12), 0.0], [a23 * (0.5 * b12), a23 - a12, -(a12 * (0.5 * b23))], [0.0, -(a12 * (0.5 * b23)), -a12]]
    B = [[a23, 0.0, a23 * (0.5 * b13)], [0.0, -a13, -(a13 * (0.5 * b23))], [a23 * (0.5 * b13), -(a13 * (0.5 * b23)), a23 - a13]]
    col = lambda M, j: [M[0][j], M[1][j], M[2][j]]  # noqa: E731
    A0, A1, A2, B0, B1, B2 = col(A, 0), col(A, 1), col(A, 2), col(B, 0), col(B, 1), col(B, 2)
    p0 = _det3c(A0, A1, A2)
    p3 = _det3c(B0, B1, B2)
    p1 = (_det3c(B0, A1, A2) + _det3c(A0, B1, A2)) + _det3c(A0, A1, B2)
    p2 = (_det3c(A0, B1, B2) + _det3c(B0, A1, B2)) + _det3c(B0, B1, A2)
    if abs(p3) >= abs(p0):
        g = _cubic_root(_div(p2, p3), _div(p1, p3), _div(p0, p3))
    else:
        g = _div(1.0, _cubic_root(_div(p1, p0), _div(p2, p0), _div(p3, p0)))
    D = [[A[i][j] + g * B[i][j] for j in range(3)] for i in range(3)]
    tr = (D[0][0] + D[1][1]) + D[2][2]
    mn = ((D[0][0] * D[1][1] - D[0][1] * D[1][0]) + (D[0][0] * D[2][2] - D[0][2] * D[2][0])) + (D[1][1] * D[2][2] - D[1][2] * D[2][1])
    h = 0.5 * tr
    hv = h * h - mn
    q = math.sqrt(hv) if hv > 0.0 else 0.0   # fmax(hv, 0): NaN and negatives give 0
    sa, sb = h + q, h - q
    sig1, sig2 = (sa, sb) if abs(sa) >= abs(sb) else (sb, sa)
    e2 = _null_vec(D, 0.0)
    e0 = _null_vec(D, sig1)
    e1 = [e2[1] * e0[2] - e2[2] * e0[1], e2[2] * e0[0] - e2[0] * e0[2], e2[0] * e0[1] - e2[1] * e0[0]]
    n1 = _sqrt(dot(e1, e1))
    e1 = [_div(v, n1) for v in e1]
    s = _sqrt(_div(-sig2, sig1))
    dc = _cross(d12, d13)
    dX = _det3c(d12, d13, dc)
    Xi = [[_div(d13[1] * dc[2] - d13[2] * dc[1], dX), _div(d13[2] * dc[0] - d13[0] * dc[2], dX), _div(d13[0] * dc[1] - d13[1] * dc[0], dX)],
          [_div(dc[1] * d12[2] - dc[2] * d12[1], dX), _div(dc[2] * d12[0] - dc[0] * d12[2], dX), _div(dc[0] * d12[1] - dc[1] * d12[0], dX)],
          [_div(d12[1] * d13[2] - d12[2] * d13[1], dX), _div(d12[2] * d13[0] - d12[0] * d13[2], dX), _div(d12[0] * d13[1] - d12[1] * d13[0], dX)]]
    out = [None] * 4
    for sg in range(2):
        ss = s if sg == 0 else -s
        nv = [e0[k] - ss * e1[k] for k in range(3)]
        w0, w1 = _div(-nv[1], nv[0]), _div(-nv[2], nv[0])
        dd = a13 - a12
        qa = (dd * (w1 * w1) - a12) - (a12 * b13) * w1
        qb = ((2.0 * dd) * (w0 * w1) + (a13 * b12) * w1) - (a12 * b13) * w0
        qc = (dd * (w0 * w0) + a13) + (a13 * b12) * w0
        disc = qb * qb - 4.0 * (qa * qc)
        sq = _sqrt(disc)
        qq = -0.5 * (qb + (sq if qb >= 0.0 else -sq))
        for r, tau in enumerate((_div(qq, qa), _div(qc, qq))):
            den = (tau * tau + b23 * tau) + 1.0
            l1 = _sqrt(_div(a23, den))
            l = [(w0 + w1 * tau) * l1, l1, tau * l1]
            res, Fr = _lam_res(l, a12, a13, a23, b12, b13, b23)
            for _ in range(3):
                J00, J01 = 2.0 * l[0] + b12 * l[1], 2.0 * l[1] + b12 * l[0]
                J10, J12 = 2.0 * l[0] + b13 * l[2], 2.0 * l[2] + b13 * l[0]
                J21, J22 = 2.0 * l[1] + b23 * l[2], 2.0 * l[2] + b23 * l[1]
                dj = (J00 * (0.0 - J12 * J21) - J01 * (J10 * J22)) + 0.0
                x0 = _div(Fr[0] * (0.0 - J12 * J21) - J01 * (Fr[1] * J22 - J12 * Fr[2]), dj)
                x1 = _div(J00 * (Fr[1] * J22 - J12 * Fr[2]) - Fr[0] * (J10 * J22), dj)
                x2 = _div(J00 * (0.0 * Fr[2] - Fr[1] * J21) - J01 * (J10 * Fr[2]) + Fr[0] * (J10 * J21), dj)
                ln = [l[0] - x0, l[1] - x1, l[2] - x2]
                rn, Fn = _lam_res(ln, a12, a13, a23, b12, b13, b23)
                if not rn < res:
                    break
                res, l, Fr = rn, ln, Fn
            ok = tau > 0.0 and den > 0.0 and l[0] > 0.0 and l[1] > 0.0 and l[2] > 0.0
            Y = [[l[i] * y[i][k] for k in range(3)] for i in range(3)]
            y12 = [Y[0][k] - Y[1][k] for k in range(3)]
            y13 = [Y[0][k] - Y[2][k] for k in range(3)]
            yc = _cross(y12, y13)
            R = [(y12[i] * Xi[0][j] + y13[i] * Xi[1][j]) + yc[i] * Xi[2][j] for i in range(3) for j in range(3)]
            t = [Y[0][i] - ((R[3 * i] * X[0][0] + R[3 * i + 1] * X[0][1]) + R[3 * i + 2] * X[0][2]) for i in range(3)]
            ok = ok and all(math.isfinite(v) for v in R + t)
            out[2 * sg + r] = (R, t) if ok else None
    return out


def ranked(slots):
    """the valid solutions by ascending |t|^2 (ties: slot order)"""
    keyed = []
    for i, sl in enumerate(slots):
        if sl is None:
            continue
        t = sl[1]
        k2 = (t[0] * t[0] + t[1] * t[1]) + t[2] * t[2]
        if math.isfinite(k2):
            keyed.append((k2, i, sl))
    keyed.sort(key=lambda e: (e[0], e[1]))
    return [e[2] for e in keyed]


def bearings(cu, cv, fx, fy):
    """unit bearings of ((u - cx) / fx, (v - cy) / fy, 1) from cu = cx - u, cv = cy - v (scalars)"""
    bx, by = _div(-cu, fx), _div(-cv, fy)
    nr = math.sqrt((bx * bx + by * by) + 1.0)
    return [_div(bx, nr), _div(by, nr), _div(1.0, nr)]


def hypotheses(Xs, cu, cv, fx, fy, seed, frame, s):
    n = len(cu)
    ids = sample(seed, frame, s, n)
    y = [bearings(float(cu[i]), float(cv[i]), fx, fy) for i in ids]
    X = [[float(v) for v in Xs[i]] for i in ids]
    return ranked(p3p(y, X))


def predicate_terms(R, t, Xs, cu, cv, fx, fy, ip):
    """(lhs = a^2 + b^2, rhs = (inlier_px z)^2, z) per correspondence, in the kernel's order"""
    R = np.asarray(R, np.float64)
    t = np.asarray(t, np.float64)
    X0, X1, X2 = Xs[:, 0], Xs[:, 1], Xs[:, 2]
    x = ((R[0] * X0 + R[1] * X1) + R[2] * X2) + t[0]
    y = ((R[3] * X0 + R[4] * X1) + R[5] * X2) + t[1]
    z = ((R[6] * X0 + R[7] * X1) + R[8] * X2) + t[2]
    a = fx * x + cu * z
    b = fy * y + cv * z
    e = ip * z
    return a * a + b * b, e * e, z


def inliers(R, t, Xs, cu, cv, fx, fy, ip):
    with np.errstate(all="ignore"):
        lhs, rhs, z = predicate_terms(R, t, Xs, cu, cv, fx, fy, ip)
        return (z > 0) & (lhs <= rhs)


def residuals(R, t, Xs, cu, cv, fx, fy):
    """pixel residuals (division form) [n][2]"""
    R = np.asarray(R, np.float64)
    q = Xs @ R.reshape(3, 3).T
    p = q + np.asarray(t, np.float64)
    return np.stack([fx * (p[:, 0] / p[:, 2]) + cu, fy * (p[:, 1] / p[:, 2]) + cv], 1)


def jacobian(R, t, Xs, fx, fy):
    """d residual / d (omega, tau) for R' = Exp(omega) R, t' = t + tau: [n][2][6]"""
    q = Xs @ np.asarray(R, np.float64).reshape(3, 3).T
    p = q + np.asarray(t, np.float64)
    z = p[:, 2]
    pu, pv = p[:, 0] / z, p[:, 1] / z
    zero = np.zeros_like(z)
    a = np.stack([np.stack([fx / z, zero, -(fx * pu) / z], 1), np.stack([zero, fy / z, -(fy * pv) / z], 1)], 1)   # [n][2][3]
    J = np.zeros((len(z), 2, 6))
    for r in range(2):
        J[:, r, 0] = q[:, 1] * a[:, r, 2] - q[:, 2] * a[:, r, 1]
        J[:, r, 1] = q[:, 2] * a[:, r, 0] - q[:, 0] * a[:, r, 2]
        J[:, r, 2] = q[:, 0] * a[:, r, 1] - q[:, 1] * a[:, r, 0]
        J[:, r, 3:] = a[:, r, :]
    return J


def rotate_left(om, R):
    om = np.asarray(om, np.float64)
    th2 = float(om @ om)
    if th2 < 1e-8:
        A, B = 1.0 - th2 / 6.0, 0.5 - th2 / 24.0
    else:
        th = math.sqrt(th2)
        A, B = math.sin(th) / th, (1.0 - math.cos(th)) / th2
    W = np.array([[0.0, -om[2], om[1]], [om[2], 0.0, -om[0]], [-om[1], om[0], 0.0]])
    E = np.eye(3) + A * W + B * (np.outer(om, om) - th2 * np.eye(3))
    return (E @ np.asarray(R, np.float64).reshape(3, 3)).reshape(9)


def refine(R, t, Xs, cu, cv, fx, fy, ip, iters):
    """Gauss-Newton on the inliers of (R, t) -> (R, t, steps kept)"""
    R, t = np.array(R, np.float64), np.array(t, np.float64)
    m = inliers(R, t, Xs, cu, cv, fx, fy, ip)
    X, u, v = Xs[m], cu[m], cv[m]
    C = float((residuals(R, t, X, u, v, fx, fy) ** 2).sum())
    kept = 0
    for _ in range(iters):
        r = residuals(R, t, X, u, v, fx, fy).reshape(-1)
        J = jacobian(R, t, X, fx, fy).reshape(-1, 6)
        A, g = J.T @ J, J.T @ r
        try:
            L = np.linalg.cholesky(A)
        except np.linalg.LinAlgError:
            break
        d = -np.linalg.solve(L.T, np.linalg.solve(L, g))
        if not np.linalg.norm(d) > 1e-12 * (1.0 + np.linalg.norm(t)):
            break
        Rn, tn = rotate_left(d[:3], R), t + d[3:]
        Cn = float((residuals(Rn, tn, X, u, v, fx, fy) ** 2).sum())
        if not Cn < C:
            break
        R, t, C = Rn, tn, Cn
        kept += 1
    return R, t, kept


def correspondences(kps, reg, K, offsets, nodes, xyz, track_flags=None):
    """per target frame: (node indices, track indices, X [n][3], u [n], v [n]) in the contract's order; the nodes of a
    track with two nodes in one target frame are left out (and counted in 'twice')"""
    nf = len(kps)
    offsets, nodes = np.asarray(offsets), np.asarray(nodes).reshape(-1, 2)
    xyz = np.asarray(xyz, np.float64).reshape(-1, 3)
    K = np.asarray(K, np.float64).reshape(nf, 4)
    kok = np.isfinite(K).all(1) & (K[:, 0] != 0) & (K[:, 1] != 0)
    tgt = (np.asarray(reg) != 0) & kok
    out = {f: ([], []) for f in range(nf) if tgt[f]}
    twice = 0
    for t in range(len(offsets) - 1):
        o = range(offsets[t], offsets[t + 1])
        if (track_flags is not None and track_flags[t] != 0) or not np.isfinite(xyz[t]).all():
            continue
        fr = [int(nodes[i, 0]) for i in o]
        for i in o:
            f = int(nodes[i, 0])
            if not tgt[f]:
                continue
            if fr.count(f) > 1:
                twice += 1
                continue
            out[f][0].append(i)
            out[f][1].append(t)
    res = {}
    for f, (nd, tr) in out.items():
        nd, tr = np.array(nd, np.int64), np.array(tr, np.int64)
        k = kps[f]
        ks = nodes[nd, 1] if len(nd) else np.zeros(0, np.int64)
        kx, ky = (k["x"], k["y"]) if getattr(k, "dtype", None) is not None and k.dtype.names else (np.asarray(k)[:, 0], np.asarray(k)[:, 1])
        u = np.asarray(kx, np.float64)[ks] if len(nd) else np.zeros(0)
        v = np.asarray(ky, np.float64)[ks] if len(nd) else np.zeros(0)
        res[f] = (nd, tr, xyz[tr] if len(tr) else np.zeros((0, 3)), u, v)
    return res, twice


def register(kps, K, Rt, reg, offsets, nodes, xyz, track_flags=None, n_samples=1024, inlier_px=2.0, min_inliers=12,
             refine_iters=10, seed=0):
    """-> dict(Rt, P, frame_stats, frame_err, node_inlier, report, and per target: margin [n] (|lhs - rhs| / rhs at the
    final pose), winner pose before refinement, S)"""
    nf = len(kps)
    K = np.asarray(K, np.float64).reshape(nf, 4)
    Rt = np.asarray(Rt, np.float64).reshape(nf, 12)
    reg = np.asarray(reg)
    nan = float("nan")
    Rt_out, P_out = Rt.copy(), np.full((nf, 12), nan)
    stats = np.full((nf, 4), -1, np.int32)
    ferr = np.full((nf, 2), nan)
    node_inlier = np.full(len(np.asarray(nodes).reshape(-1, 2)), -1, np.int32)
    corr, twice = correspondences(kps, reg, K, offsets, nodes, xyz, track_flags)
    extra = {}
    for f in range(nf):
        kf = K[f]
        kok = np.isfinite(kf).all() and kf[0] != 0 and kf[1] != 0
        if reg[f] == 0:
            if kok and np.isfinite(Rt[f]).all():
                P_out[f] = make_P(kf, Rt[f])
            continue
        if not kok:
            Rt_out[f] = nan
            stats[f] = (0, 0, -1, BADK)
            continue
        nd, tr, X, u, v = corr[f]
        n = len(nd)
        fx, fy, cx, cy = (float(x) for x in kf)
        S = X.mean(axis=0) if n else np.zeros(3)
        Xs = X - S
        cu, cv = cx - u, cy - v
        flags, win, fin = 0, -1, 0
        R = t = None
        if n < 3:
            flags = FEWPOINTS
        else:
            best = (-1, 0)
            for s in range(n_samples):
                for rank, (Rh, th) in enumerate(hypotheses(Xs, cu, cv, fx, fy, seed, f, s)):
                    c = int(inliers(Rh, th, Xs, cu, cv, fx, fy, inlier_px).sum())
                    h = 4 * s + rank
                    if c > best[0]:
                        best = (c, h)
                        R, t = Rh, th
            if best[0] < 0:
                flags = NOSOLUTION
            else:
                win = best[1] // 4
                extra[f] = dict(R0=np.array(R), t0=np.array(t), S=S, h=best[1], winner_inliers=best[0])
                R, t, kept = refine(R, t, Xs, cu, cv, fx, fy, inlier_px, refine_iters)
                with np.errstate(all="ignore"):
                    lhs, rhs, z = predicate_terms(R, t, Xs, cu, cv, fx, fy, inlier_px)
                m = (z > 0) & (lhs <= rhs)
                fin = int(m.sum())
                node_inlier[nd] = m.astype(np.int32)
                if fin:
                    e = np.sqrt((residuals(R, t, Xs[m], cu[m], cv[m], fx, fy) ** 2).sum(1))
                    ferr[f] = (math.sqrt(float((e ** 2).sum()) / fin), float(e.max()))
                extra[f].update(margin=np.abs(lhs - rhs) / rhs, kept=kept, R=R, t=t, nodes=nd)
                if fin < min_inliers:
                    flags |= FEWINLIERS
        if n and win < 0:
            node_inlier[nd] = 0
        stats[f] = (n, fin, win, flags)
        if flags == 0:
            Rr = np.asarray(R).reshape(3, 3)
            Rt_out[f] = np.concatenate([Rr.reshape(9), np.asarray(t) - Rr @ S])
            P_out[f] = make_P(kf, Rt_out[f])
        else:
            Rt_out[f] = nan
    tg = reg != 0
    report = np.array([tg.sum(), (tg & (stats[:, 3] == 0)).sum()] + [(tg & ((stats[:, 3] >> b) & 1 == 1)).sum() for b in range(4)] +
                      [stats[tg, 0].sum(), stats[tg, 1].sum()], np.int32)
    return dict(Rt=Rt_out, P=P_out, frame_stats=stats, frame_err=ferr, node_inlier=node_inlier, report=report, extra=extra,
                twice=twice)


def make_P(k, rt):
    r = np.asarray(rt, np.float64)
    M = np.concatenate([r[:9].reshape(3, 3), r[9:, None]], 1)
    return np.stack([k[0] * M[0] + k[2] * M[2], k[1] * M[1] + k[3] * M[2], M[2]]).reshape(12)


def centre(rt):
    r = np.asarray(rt, np.float64)
    return -r[:9].reshape(3, 3).T @ r[9:]
