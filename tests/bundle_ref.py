"""numpy float64 restatement of bundle adjustment (include/pgx.h, "bundle adjustment of cameras and track points"): the
yardstick of tests/test_gpu_bundle.py.  The point blocks are eliminated (Schur complement) and the reduced camera system is
solved by np.linalg.cholesky; tests/test_bundle_ref.py ties this file to the full normal equations solved densely, with the
Jacobian checked against central differences.  Besides the outputs it returns the accept / reject sequence."""
import numpy as np

UNKNOWN, FIXED = -1, -2
MAX_FREE = 128


class NotPD(Exception):
    pass


def frame_states(K, Rt, fixed):
    """-> (state [F]: UNKNOWN, FIXED or the free number, n_free (uncapped), bad_rotation [F] bool)"""
    K, Rt = np.asarray(K, np.float64).reshape(-1, 4), np.asarray(Rt, np.float64).reshape(-1, 12)
    st = np.full(len(K), UNKNOWN)
    bad_rot = np.zeros(len(K), bool)
    n_free = 0
    for f in range(len(K)):
        if not (np.isfinite(K[f]).all() and np.isfinite(Rt[f]).all() and K[f, 0] != 0 and K[f, 1] != 0):
            continue
        R = Rt[f, :9].reshape(3, 3)
        if not (np.abs(R @ R.T - np.eye(3)).max() <= 1e-9 and np.linalg.det(R) > 0):
            bad_rot[f] = True
            continue
        if fixed[f]:
            st[f] = FIXED
        else:
            st[f] = n_free if n_free < MAX_FREE else UNKNOWN
            n_free += 1
    return st, n_free, bad_rot


def exp_so3(w):
    th2 = float(w @ w)
    if th2 < 1e-8:
        A, B = 1.0 - th2 / 6.0, 0.5 - th2 / 24.0
    else:
        th = np.sqrt(th2)
        A, B = np.sin(th) / th, (1.0 - np.cos(th)) / th2
    Wx = np.array([[0.0, -w[2], w[1]], [w[2], 0.0, -w[0]], [-w[1], w[0], 0.0]])
    return np.eye(3) + A * Wx + B * (Wx @ Wx)


def huber(s, delta):
    """-> (rho, w)"""
    s = np.asarray(s, np.float64)
    inside = s <= delta * delta
    rs = np.sqrt(s)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(inside, s, 2.0 * delta * rs - delta * delta), np.where(inside, 1.0, delta / rs)


def project(R, t, K, X):
    """R [m][3][3], t [m][3], K [m][4], X [m][3] -> (uv [m][2], z [m], q = R X [m][3], p = q + t)"""
    q = np.einsum("mij,mj->mi", R, X)
    p = q + t
    uv = np.stack([K[:, 0] * (p[:, 0] / p[:, 2]) + K[:, 2], K[:, 1] * (p[:, 1] / p[:, 2]) + K[:, 3]], 1)
    return uv, p[:, 2], q, p


def jacobians(R, K, q, p):
    """-> (Jc [m][2][6] wrt (omega, tau), Jp [m][2][3] wrt X)"""
    z = p[:, 2]
    a = np.zeros((len(z), 2, 3))
    a[:, 0, 0] = K[:, 0] / z
    a[:, 0, 2] = -(K[:, 0] * (p[:, 0] / z)) / z
    a[:, 1, 1] = K[:, 1] / z
    a[:, 1, 2] = -(K[:, 1] * (p[:, 1] / z)) / z
    Jp = np.einsum("mrk,mkc->mrc", a, R)
    Jw = np.cross(q[:, None, :], a)        # a . (-[q]x) = q x a
    return np.concatenate([Jw, a], axis=2), Jp


class Problem:
    """The observations that take part, after the contract's frame and track rules."""

    def __init__(self, kps, K, Rt, fixed, offsets, nodes, xyz, track_flags=None, max_tracks=None):
        self.K = np.asarray(K, np.float64).reshape(-1, 4)
        self.Rt0 = np.asarray(Rt, np.float64).reshape(-1, 12)
        self.state, self.n_free_all, self.bad_rot = frame_states(self.K, self.Rt0, np.asarray(fixed).reshape(-1))
        self.n_fixed = int((self.state == FIXED).sum())
        self.err = self.n_free_all > MAX_FREE or self.n_fixed == 0
        self.n_free = self.n_free_all
        xy = [np.stack([k["x"], k["y"]], 1).astype(np.float64) if getattr(k, "dtype", None) is not None and k.dtype.names
              else np.asarray(k, np.float64).reshape(-1, 2) for k in kps]
        offsets, nodes = np.asarray(offsets), np.asarray(nodes).reshape(-1, 2)
        xyz = np.asarray(xyz, np.float64).reshape(-1, 3)
        nt = len(offsets) - 1 if max_tracks is None else min(len(offsets) - 1, max_tracks)
        self.nt, self.offsets, self.nodes, self.xyz_in = nt, offsets, nodes, xyz
        self.free_frames = [f for f in range(len(self.K)) if self.state[f] >= 0]
        tracks, ob_t, ob_f, ob_uv, ob_node, dup = [], [], [], [], [], False
        for t in range(nt):
            o = np.arange(offsets[t], offsets[t + 1])
            f = nodes[o, 0]
            if len(set(f.tolist())) != len(f):
                dup = True
                continue
            use = self.state[f] != UNKNOWN
            ok = (track_flags is None or track_flags[t] == 0) and np.isfinite(xyz[t]).all() and use.sum() >= 2 and not self.err
            if not ok:
                continue
            j = len(tracks)
            tracks.append(t)
            for oo in o[use]:
                fr, k = nodes[oo]
                ob_t.append(j)
                ob_f.append(fr)
                ob_uv.append(xy[fr][k])
                ob_node.append(oo)
        self.dup = dup
        self.tracks = np.array(tracks, np.int64)
        self.ob_t, self.ob_f = np.array(ob_t, np.int64), np.array(ob_f, np.int64)
        self.ob_uv, self.ob_node = np.array(ob_uv, np.float64).reshape(-1, 2), np.array(ob_node, np.int64)
        self.ob_cf = self.state[self.ob_f] if len(self.ob_f) else np.zeros(0, np.int64)

    def residuals(self, Rt, X):
        """Rt [F][12], X [n_part][3] -> (r [m][2], z [m], q, p)"""
        R = Rt[self.ob_f, :9].reshape(-1, 3, 3)
        uv, z, q, p = project(R, Rt[self.ob_f, 9:], self.K[self.ob_f], X[self.ob_t])
        return uv - self.ob_uv, z, q, p

    def cost(self, Rt, X, delta):
        r, _, _, _ = self.residuals(Rt, X)
        rho, _ = huber((r * r).sum(1), delta)
        return float(rho.sum())

    def linearise(self, Rt, X, delta):
        r, _, q, p = self.residuals(Rt, X)
        rho, w = huber((r * r).sum(1), delta)
        Jc, Jp = jacobians(Rt[self.ob_f, :9].reshape(-1, 3, 3), self.K[self.ob_f], q, p)
        return dict(r=r, w=w, Jc=Jc, Jp=Jp, C=float(rho.sum()))

    def apply(self, Rt, X, dc, dX):
        Rt2 = Rt.copy()
        for c, f in enumerate(self.free_frames):
            R = Rt[f, :9].reshape(3, 3)
            Rt2[f, :9] = (exp_so3(dc[6 * c:6 * c + 3]) @ R).reshape(9)
            Rt2[f, 9:] = Rt[f, 9:] + dc[6 * c + 3:6 * c + 6]
        return Rt2, X + dX

    def solve_schur(self, lin, lam):
        """(A + lam D) delta = -g by the Schur complement -> (dc [6 n_free], dX [n_part][3]); NotPD if a block or pivot is not
        positive definite"""
        nfr, npt = self.n_free, len(self.tracks)
        w, Jc, Jp, r = lin["w"], lin["Jc"], lin["Jp"], lin["r"]
        V = np.zeros((npt, 3, 3))
        np.add.at(V, self.ob_t, w[:, None, None] * np.einsum("mki,mkj->mij", Jp, Jp))
        gp = np.zeros((npt, 3))
        np.add.at(gp, self.ob_t, w[:, None] * np.einsum("mki,mk->mi", Jp, r))
        Vd = V.copy()
        for i in range(3):
            Vd[:, i, i] += lam * np.clip(V[:, i, i], 1e-6, 1e32)
        if npt:
            if not np.isfinite(Vd).all():       # a NaN block is not positive definite; LAPACK need not say so
                raise NotPD()
            try:
                np.linalg.cholesky(Vd)          # raises if any block is not positive definite
            except np.linalg.LinAlgError:
                raise NotPD()
        Vi = np.linalg.inv(Vd)
        fr = self.ob_cf >= 0
        idx = np.flatnonzero(fr)
        cf = self.ob_cf[idx]
        W = w[idx, None, None] * np.einsum("mki,mkj->mij", Jc[idx], Jp[idx])     # [n][6][3]
        Y = np.einsum("mij,mjk->mik", W, Vi[self.ob_t[idx]])                     # W V*^-1
        U = np.zeros((nfr, 6, 6))
        np.add.at(U, cf, w[idx, None, None] * np.einsum("mki,mkj->mij", Jc[idx], Jc[idx]))
        gc = np.zeros((nfr, 6))
        np.add.at(gc, cf, w[idx, None] * np.einsum("mki,mk->mi", Jc[idx], r[idx]))
        Sf = np.zeros((6 * nfr, 6 * nfr))
        for c in range(nfr):
            Sf[6 * c:6 * c + 6, 6 * c:6 * c + 6] = U[c] + lam * np.diag(np.clip(np.diag(U[c]), 1e-6, 1e32))
        rhs = -gc
        np.add.at(rhs, cf, np.einsum("mij,mj->mi", Y, gp[self.ob_t[idx]]))
        # every pair (a, b) of free observations in one track adds -Y_a W_b^T to block (cam a, cam b).  A track holds at most one
        # observation per frame, so (free camera, track) places each Y_a and W_b once in a [6 n_free][3 n_part] matrix, and the
        # sum over all pairs of all tracks is one product of two of them
        if len(idx):
            tcol = self.ob_t[idx]
            Yb, Wb = np.zeros((nfr, 6, npt, 3)), np.zeros((nfr, 6, npt, 3))
            Yb[cf, :, tcol, :] = Y
            Wb[cf, :, tcol, :] = W
            Sf -= Yb.reshape(6 * nfr, 3 * npt) @ Wb.reshape(6 * nfr, 3 * npt).T
        if nfr:
            if not np.isfinite(Sf).all():
                raise NotPD()
            try:
                L = np.linalg.cholesky(np.tril(Sf) + np.tril(Sf, -1).T)
            except np.linalg.LinAlgError:
                raise NotPD()
            dc = np.linalg.solve(L.T, np.linalg.solve(L, rhs.reshape(-1)))
        else:
            dc = np.zeros(0)
        b = -gp
        if len(idx):
            e = np.einsum("mji,mj->mi", W, dc.reshape(-1, 6)[cf])     # W_a^T dc_a [n][3]
            np.add.at(b, self.ob_t[idx], -e)
        dX = np.einsum("tij,tj->ti", Vi, b)
        return dc, dX

    def x_norm(self, Rt, X):
        ts = Rt[self.free_frames, 9:] if self.free_frames else np.zeros((0, 3))
        return np.sqrt((ts * ts).sum() + (X * X).sum())


def bundle_adjust(kps, K, Rt, fixed, offsets, nodes, xyz, track_flags=None, max_iters=20, huber_px=np.inf, lambda0=1e-3,
                  max_tracks=None, solver=None):
    """The contract's loop.  solver(problem, lin, lam) -> (dc, dX) replaces the Schur solve (tests/test_bundle_ref.py).
    -> dict(Rt, P, xyz [nt][3], node_err [n_nodes], trace [max_iters + 1][2], report [8], decisions (list of 'accept',
    'reject', 'nonpd', 'small'), trial (per attempt: the trial cost C_new of an accept or a reject, NaN for 'nonpd' and
    'small'), small_ratio (of a 'small' stop: ||delta|| / (1e-12 (1 + ||x||)), else None), problem)"""
    pb = Problem(kps, K, Rt, fixed, offsets, nodes, xyz, track_flags, max_tracks)
    solver = solver or (lambda p, lin, lam: p.solve_schur(lin, lam))
    Rt_c = pb.Rt0.copy()
    X = pb.xyz_in[pb.tracks].copy() if len(pb.tracks) else np.zeros((0, 3))
    lam = float(lambda0)
    trace = np.full((max_iters + 1, 2), np.nan)
    lin = pb.linearise(Rt_c, X, huber_px) if len(pb.tracks) else dict(C=0.0)
    C = lin["C"]
    trace[0] = (C, lam)
    it = acc = nonpd = 0
    decisions, trial, small_ratio = [], [], None

    def start_reason():
        if pb.err or len(pb.tracks) == 0:
            return 0
        if C == 0.0:
            return 2
        if lam > 1e16:
            return 4
        if max_iters == 0:
            return 1
        return None
    reason = start_reason()
    while reason is None:
        it += 1
        reason_now, accepted = None, False
        try:
            dc, dX = solver(pb, lin, lam)
            ok = True
        except NotPD:
            ok = False
        if not ok:
            nonpd += 1
            lam *= 10.0
            decisions.append("nonpd")
            trial.append(np.nan)
        elif np.sqrt((dc * dc).sum() + (dX * dX).sum()) <= 1e-12 * (1.0 + pb.x_norm(Rt_c, X)):
            reason_now = 3
            decisions.append("small")
            trial.append(np.nan)
            small_ratio = float(np.sqrt((dc * dc).sum() + (dX * dX).sum()) / (1e-12 * (1.0 + pb.x_norm(Rt_c, X))))
        else:
            Rt_t, X_t = pb.apply(Rt_c, X, dc, dX)
            Cn = pb.cost(Rt_t, X_t, huber_px)
            trial.append(Cn)
            if Cn < C:
                accepted = True
                small = C - Cn <= 1e-12 * C
                C = Cn
                lam = max(lam / 10.0, 1e-12)
                acc += 1
                Rt_c, X = Rt_t, X_t
                lin = pb.linearise(Rt_c, X, huber_px)
                decisions.append("accept")
                if small or C == 0.0:
                    reason_now = 2
            else:
                lam *= 10.0
                decisions.append("reject")
        if reason_now is None:
            if lam > 1e16:
                reason_now = 4
            elif it >= max_iters:
                reason_now = 1
        trace[it] = (C, lam)
        reason = reason_now
        del accepted
    # outputs
    Rt_out = Rt_c
    P = np.full((len(Rt_out), 12), np.nan)
    for f in range(len(Rt_out)):
        if pb.state[f] != UNKNOWN:
            R, t = Rt_out[f, :9].reshape(3, 3), Rt_out[f, 9:]
            M = np.concatenate([R, t[:, None]], 1)
            Kf = pb.K[f]
            P[f, 0:4] = Kf[0] * M[0] + Kf[2] * M[2]
            P[f, 4:8] = Kf[1] * M[1] + Kf[3] * M[2]
            P[f, 8:12] = M[2]
    xyz_out = pb.xyz_in[:pb.nt].copy()
    if len(pb.tracks):
        xyz_out[pb.tracks] = X
    node_err = np.full(len(pb.nodes), np.nan)
    zneg = 0
    if len(pb.tracks):
        r, z, _, _ = pb.residuals(Rt_out, X)
        node_err[pb.ob_node] = np.sqrt((r * r).sum(1))
        zneg = int((~(z > 0)).sum())
    report = np.array([it, acc, reason, pb.n_free_all, len(pb.tracks), len(pb.ob_t), zneg, nonpd], np.int32)
    return dict(Rt=Rt_out, P=P, xyz=xyz_out, node_err=node_err, trace=trace, report=report, decisions=decisions,
                trial=np.array(trial, np.float64), small_ratio=small_ratio, problem=pb)


def camera_centres(Rt):
    Rt = np.asarray(Rt, np.float64).reshape(-1, 12)
    return np.stack([-Rt[f, :9].reshape(3, 3).T @ Rt[f, 9:] for f in range(len(Rt))])
