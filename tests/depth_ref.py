"""The numpy yardstick of the dense stage (include/pgx.h: pgx_depth_maps_dev, pgx_depth_fuse_dev), operation by operation in the
header's order, with the full cost volume in memory; a loop-per-pixel restatement of the depth maps that shares nothing with
the vectorised one but the camera algebra; and the two-plane test scene.  Python floats and numpy float64 scalars do not
contract a b + c, which is what the library's -ffp-contract=off build does.  The yardstick's camera algebra is a transcription
of pgx.h, as the kernel's is: exact_warp and exact_plane_scale restate it in rationals and decimals without those lines, and
scene_rotated shows the two planes to cameras that are turned, rolled, skewed, scaled and mirrored.  A plain helper module."""
import decimal
import itertools
from fractions import Fraction

import numpy as np

NOCAMERA, NOVIEWS, EDGE, HIGHCOST = 1, 2, 4, 8
PEN = 31
_POP8 = np.array([bin(i).count("1") for i in range(256)], dtype=np.int32)


# ---- cameras -----------------------------------------------------------------------------------------------------------

def camera(P):
    """-> (known, adj [3][3], det, sign(det), ||m3||, p4) of one 3 x 4 camera"""
    p = np.asarray(P, dtype=np.float64).reshape(12)
    with np.errstate(all="ignore"):
        m00, m01, m02, m10, m11, m12, m20, m21, m22 = p[0], p[1], p[2], p[4], p[5], p[6], p[8], p[9], p[10]
        adj = np.array([[m11 * m22 - m12 * m21, m02 * m21 - m01 * m22, m01 * m12 - m02 * m11],
                        [m12 * m20 - m10 * m22, m00 * m22 - m02 * m20, m02 * m10 - m00 * m12],
                        [m10 * m21 - m11 * m20, m01 * m20 - m00 * m21, m00 * m11 - m01 * m10]])
        det = (m00 * adj[0, 0] + m01 * adj[1, 0]) + m02 * adj[2, 0]
        n3 = np.sqrt((m20 * m20 + m21 * m21) + m22 * m22)
    known = bool(np.isfinite(p).all() and det != 0.0)
    return known, adj, det, (1.0 if det > 0.0 else -1.0), n3, p[[3, 7, 11]]


def slot_of(frame_ids, F, n_frames, f):
    if f < 0 or f >= n_frames:
        return -1
    if frame_ids is None:
        return int(f) if f < F else -1
    hit = np.flatnonzero(np.asarray(frame_ids) == f)
    return int(hit[0]) if len(hit) else -1


def plan(F, frame_ids, n_frames, P, views, ranges, D):
    """rules 2 and 3 -> (slots [R][1 + S], warp [R][S][12], planes [R][D])"""
    P = np.asarray(P, dtype=np.float64).reshape(-1, 12)
    views = np.asarray(views, dtype=np.int64)
    R, S = views.shape[0], views.shape[1] - 1
    slots = np.full((R, 1 + S), -1, dtype=np.int64)
    warp = np.full((R, S, 12), np.nan)
    planes = np.full((R, D), np.nan)
    for r in range(R):
        fr = views[r, 0]
        sl = slot_of(frame_ids, F, n_frames, fr)
        zn, zf = np.asarray(ranges, dtype=np.float64).reshape(-1, 2)[r]
        ok = sl >= 0
        if ok:
            ok, adj, det, sg, n3, p4r = camera(P[fr])
        ok = bool(ok and zn > 0.0 and zn < zf and np.isfinite(zf))
        if not ok:
            continue
        slots[r, 0] = sl
        izf, izn = 1.0 / zf, 1.0 / zn
        sn = sg * n3
        for k in range(D):
            iz = izf + (float(k) / float(D - 1)) * (izn - izf)
            planes[r, k] = sn * (1.0 / iz)
        for s in range(S):
            fs = views[r, 1 + s]
            ss = slot_of(frame_ids, F, n_frames, fs)
            if ss < 0 or not camera(P[fs])[0]:
                continue
            slots[r, 1 + s] = ss
            Ms, p4s = P[fs].reshape(3, 4)[:, :3], P[fs].reshape(3, 4)[:, 3]
            for i in range(3):
                for j in range(3):
                    warp[r, s, 3 * i + j] = ((Ms[i, 0] * adj[0, j] + Ms[i, 1] * adj[1, j]) + Ms[i, 2] * adj[2, j]) / det
                A = warp[r, s, 3 * i:3 * i + 3]
                warp[r, s, 9 + i] = p4s[i] - ((A[0] * p4r[0] + A[1] * p4r[1]) + A[2] * p4r[2])
    return slots, warp, planes


# ---- rule 1 ------------------------------------------------------------------------------------------------------------

def census(g):
    g = np.asarray(g, dtype=np.float32)
    H, W = g.shape
    out = np.zeros((H, W), dtype=np.uint64)
    ys, xs = np.arange(H)[:, None], np.arange(W)[None, :]
    bit = 0
    with np.errstate(invalid="ignore"):
        for dy in range(-3, 4):
            for dx in range(-4, 5):
                if dx == 0 and dy == 0:
                    continue
                n = g[np.clip(ys + dy, 0, H - 1), np.clip(xs + dx, 0, W - 1)]
                out |= (n < g).astype(np.uint64) << np.uint64(bit)
                bit += 1
    return out


def popcount64(x):
    return _POP8[np.ascontiguousarray(x).view(np.uint8).reshape(x.shape + (8,))].sum(-1).astype(np.int32)


def pixel(q0, q1, q2, W, H):
    """rule 4's validity and nearest pixel (arrays) -> ok, iu, iv"""
    with np.errstate(all="ignore"):
        us, vs = q0 / q2 + 0.5, q1 / q2 + 0.5
        ok = (q2 > 0) & (us >= 0) & (us < W) & (vs >= 0) & (vs < H)
    iu = np.where(ok, np.floor(np.where(ok, us, 0.0)), 0).astype(np.int64)
    iv = np.where(ok, np.floor(np.where(ok, vs, 0.0)), 0).astype(np.int64)
    return ok, iu, iv


def box(raw, a):
    H, W = raw.shape[-2:]
    ys, xs = np.arange(H)[:, None], np.arange(W)[None, :]
    agg = np.zeros_like(raw)
    for dy in range(-a, a + 1):
        for dx in range(-a, a + 1):
            agg += raw[..., np.clip(ys + dy, 0, H - 1), np.clip(xs + dx, 0, W - 1)]
    return agg


def subplane(cm, c0, cp):
    """rule 7's off from agg(k* - 1), agg(k*), agg(k* + 1) (integer arrays or scalars)"""
    cm, c0, cp = (np.asarray(x, dtype=np.int64) for x in (cm, c0, cp))
    n, den = cm - cp, cm - 2 * c0 + cp
    return np.where(den != 0, np.sign(n) * ((np.abs(n) * 128) // np.where(den != 0, den, 1)), 0)


def depth_of(kq8, D, zn, zf):
    izf, izn = 1.0 / zf, 1.0 / zn
    with np.errstate(all="ignore"):
        return 1.0 / (izf + ((np.asarray(kq8, dtype=np.float64) / 256.0) / float(D - 1)) * (izn - izf))


def depth_maps(gray, frame_ids, n_frames, P, views, ranges, D, a, min_views, max_cost, warp=None, planes=None, volumes=False):
    """The depth maps of pgx_depth_maps_dev.  gray [F][H][W] by slot.  warp / planes: evaluate rules 4.. on these tables (the
    device's own) instead of the yardstick's.  cost holds -1 where the device does not write."""
    gray = np.asarray(gray, dtype=np.float32)
    F, H, W = gray.shape
    views = np.asarray(views, dtype=np.int64)
    ranges = np.asarray(ranges, dtype=np.float64).reshape(-1, 2)
    R, S = views.shape[0], views.shape[1] - 1
    slots, wp0, pl0 = plan(F, frame_ids, n_frames, P, views, ranges, D)
    wp = wp0 if warp is None else np.asarray(warp, dtype=np.float64).reshape(R, S, 12)
    pl = pl0 if planes is None else np.asarray(planes, dtype=np.float64).reshape(R, D)
    cen = [census(g) for g in gray]
    v, u = np.mgrid[0:H, 0:W].astype(np.float64)
    kq8 = np.full((R, H, W), -1, dtype=np.int32)
    depth = np.full((R, H, W), np.nan)
    cost = np.full((R, H, W), -1, dtype=np.int32)
    flags = np.zeros((R, H, W), dtype=np.int32)
    vols = []
    for r in range(R):
        if slots[r, 0] < 0:
            flags[r] = NOCAMERA
            vols.append(None)
            continue
        cr = cen[slots[r, 0]]
        raw = np.zeros((D, H, W), dtype=np.int32)
        nval = np.zeros((D, H, W), dtype=np.int32)
        for s in range(S):
            if slots[r, 1 + s] < 0:
                raw += PEN
                continue
            A, b, cs = wp[r, s, :9].reshape(3, 3), wp[r, s, 9:], cen[slots[r, 1 + s]]
            y = [(A[i, 0] * u + A[i, 1] * v) + A[i, 2] for i in range(3)]
            for k in range(D):
                w = pl[r, k]
                ok, iu, iv = pixel(w * y[0] + b[0], w * y[1] + b[1], w * y[2] + b[2], W, H)
                raw[k] += np.where(ok, popcount64(cr ^ cs[iv, iu]), PEN)
                nval[k] += ok
        agg = box(raw, a)
        ks = (agg.astype(np.int64) * 256 + np.arange(D)[:, None, None]).argmin(0)
        take = lambda vol, kk: np.take_along_axis(vol, np.clip(kk, 0, D - 1)[None], 0)[0]  # noqa: E731
        c0 = take(agg, ks)
        fl = np.where(take(nval, ks) < min_views, NOVIEWS, 0) | np.where((ks == 0) | (ks == D - 1), EDGE, 0) | \
            np.where(c0 > max_cost, HIGHCOST, 0)
        kq = 256 * ks + subplane(take(agg, ks - 1), c0, take(agg, ks + 1))
        good = fl == 0
        flags[r], cost[r] = fl, c0
        kq8[r] = np.where(good, kq, -1)
        depth[r] = np.where(good, depth_of(np.where(good, kq, 0), D, ranges[r, 0], ranges[r, 1]), np.nan)
        vols.append((raw, nval, agg))
    nocam = (flags & NOCAMERA) != 0
    summary = np.array([R * H * W, (flags == 0).sum(), nocam.sum(), ((flags & NOVIEWS) != 0).sum(), ((flags & EDGE) != 0).sum(),
                        ((flags & HIGHCOST) != 0).sum(), (slots[:, 0] < 0).sum(), 0], dtype=np.int32)
    out = dict(kq8=kq8, depth=depth, cost=cost, flags=flags, warp=wp0, planes=pl0, summary=summary)
    if volumes:
        out["volumes"] = vols
    return out


def depth_maps_loop(gray, frame_ids, n_frames, P, views, ranges, D, a, min_views, max_cost):
    """The same rule one pixel at a time in Python scalars: census bits from Python comparisons, popcounts from bin(), a cost
    per (pixel, plane, source) on demand.  Small frames only."""
    gray = np.asarray(gray, dtype=np.float32)
    F, H, W = gray.shape
    views = np.asarray(views, dtype=np.int64)
    ranges = np.asarray(ranges, dtype=np.float64).reshape(-1, 2)
    R, S = views.shape[0], views.shape[1] - 1
    slots, wp, pl = plan(F, frame_ids, n_frames, P, views, ranges, D)
    cl = lambda x, hi: min(max(x, 0), hi)  # noqa: E731

    def census_at(sl, x, y):
        c, word, bit = gray[sl, y, x], 0, 0
        for dy in range(-3, 4):
            for dx in range(-4, 5):
                if dx == 0 and dy == 0:
                    continue
                if gray[sl, cl(y + dy, H - 1), cl(x + dx, W - 1)] < c:
                    word |= 1 << bit
                bit += 1
        return word
    cen = [[[census_at(sl, x, y) for x in range(W)] for y in range(H)] for sl in range(F)]
    kq8 = np.full((R, H, W), -1, dtype=np.int32)
    depth = np.full((R, H, W), np.nan)
    cost = np.full((R, H, W), -1, dtype=np.int32)
    flags = np.zeros((R, H, W), dtype=np.int32)
    for r in range(R):
        if slots[r, 0] < 0:
            flags[r] = NOCAMERA
            continue
        memo = {}

        def raw_at(x, y, k):
            if (x, y, k) not in memo:
                tot, nv = 0, 0
                for s in range(S):
                    ss = slots[r, 1 + s]
                    if ss < 0:
                        tot += PEN
                        continue
                    A, w = [float(t) for t in wp[r, s]], float(pl[r, k])
                    q = [w * ((A[3 * i] * x + A[3 * i + 1] * y) + A[3 * i + 2]) + A[9 + i] for i in range(3)]
                    ok = q[2] > 0
                    if ok:
                        us, vs = q[0] / q[2] + 0.5, q[1] / q[2] + 0.5
                        ok = 0 <= us < W and 0 <= vs < H
                    if ok:
                        tot += bin(cen[slots[r, 0]][y][x] ^ cen[ss][int(vs)][int(us)]).count("1")
                        nv += 1
                    else:
                        tot += PEN
                memo[(x, y, k)] = (tot, nv)
            return memo[(x, y, k)]
        for y in range(H):
            for x in range(W):
                agg = [sum(raw_at(cl(x + dx, W - 1), cl(y + dy, H - 1), k)[0] for dy in range(-a, a + 1) for dx in range(-a, a + 1))
                       for k in range(D)]
                ks = min(range(D), key=lambda k: (agg[k], k))
                fl = (NOVIEWS if raw_at(x, y, ks)[1] < min_views else 0) | (EDGE if ks in (0, D - 1) else 0) | \
                    (HIGHCOST if agg[ks] > max_cost else 0)
                flags[r, y, x], cost[r, y, x] = fl, agg[ks]
                if fl == 0:
                    n, den = agg[ks - 1] - agg[ks + 1], agg[ks - 1] - 2 * agg[ks] + agg[ks + 1]
                    off = 0 if den == 0 else (1 if n > 0 else -1) * ((abs(n) * 128) // den)
                    kq8[r, y, x] = 256 * ks + off
                    izf, izn = 1.0 / ranges[r, 1], 1.0 / ranges[r, 0]
                    depth[r, y, x] = 1.0 / (izf + ((float(kq8[r, y, x]) / 256.0) / float(D - 1)) * (izn - izf))
    return dict(kq8=kq8, depth=depth, cost=cost, flags=flags)


# ---- the cross-view filter -----------------------------------------------------------------------------------------------

def fuse(depth, views, n_frames, P, rel_tol, min_agree):
    """pgx_depth_fuse_dev without the capacity: every kept pixel -> dict(xyz [n][3], src [n][2], agree [R][H][W], summary [4])"""
    depth = np.asarray(depth, dtype=np.float64)
    R, H, W = depth.shape
    views = np.asarray(views, dtype=np.int64).reshape(R, -1)
    S = views.shape[1] - 1
    P = np.asarray(P, dtype=np.float64).reshape(-1, 12)
    cams = [camera(P[f]) if 0 <= f < n_frames else (False,) for f in views[:, 0]]
    v, u = np.mgrid[0:H, 0:W].astype(np.float64)
    agree = np.full((R, H, W), -1, dtype=np.int32)
    xyz_all = np.full((R, H, W, 3), np.nan)
    with_depth = with_view = 0
    for r in range(R):
        if not cams[r][0]:
            continue
        _, adj, det, sg, n3, p4 = cams[r]
        z = depth[r]
        has = np.isfinite(z)
        with np.errstate(all="ignore"):
            w = (sg * n3) * z
            t = [w * u - p4[0], w * v - p4[1], w - p4[2]]
            X = [((adj[i, 0] * t[0] + adj[i, 1] * t[1]) + adj[i, 2] * t[2]) / det for i in range(3)]
            ag, anyv = np.zeros((H, W), dtype=np.int32), np.zeros((H, W), dtype=bool)
            for s in range(S):
                f = views[r, 1 + s]
                if f < 0 or f >= n_frames:
                    continue
                rows = np.flatnonzero(views[:, 0] == f)
                if not len(rows) or not cams[rows[0]][0]:
                    continue
                j = rows[0]
                Pj = P[f].reshape(3, 4)
                q = [((Pj[i, 0] * X[0] + Pj[i, 1] * X[1]) + Pj[i, 2] * X[2]) + Pj[i, 3] for i in range(3)]
                ok, iu, iv = pixel(q[0], q[1], q[2], W, H)
                ok &= has
                zj = depth[j][iv, iu]
                d = (cams[j][3] * q[2]) / cams[j][4]
                ag += ok & np.isfinite(zj) & (np.abs(d - zj) <= rel_tol * zj)
                anyv |= ok
        agree[r] = np.where(has, ag, -1)
        xyz_all[r] = np.stack(X, -1)
        with_depth += int(has.sum())
        with_view += int(anyv.sum())
    keep = (agree >= 0) & (agree >= min_agree)
    rr, vv, uu = np.nonzero(keep)
    skipped = sum(1 for c in cams if not c[0])
    return dict(xyz=xyz_all[keep], src=np.stack([rr, vv * W + uu], 1).astype(np.int32), agree=agree, keep=keep,
                summary=np.array([keep.sum(), with_depth, with_view, skipped], dtype=np.int32))


# ---- the test scene: two textured planes, cameras R = I -----------------------------------------------------------------

SCENE_W, SCENE_H, SCENE_F = 96, 64, 120.0
SCENE_D, SCENE_IZ = 32, (1.0 / 6.0, 1.0 / 2.0)       # planes over 1/z in [1/6, 1/2]
SCENE_CENTRES = [(0.0, 0.0, 0.0), (0.6, 0.0, 0.0), (-0.6, 0.0, 0.0), (0.0, 0.6, 0.0), (0.0, -0.6, 0.0)]


def scene_camera(C, W=SCENE_W, H=SCENE_H, f=SCENE_F):
    K = np.array([[f, 0, W / 2], [0, f, H / 2], [0, 0, 1.0]])
    return K @ np.hstack([np.eye(3), -np.asarray(C, dtype=np.float64)[:, None]])


def scene_texture(seed=1):
    """tex(X, Y): the bilinear texture of seeded noise at 12 texels per unit that both scenes paint their planes with"""
    T = np.random.default_rng(seed).random((256, 256)).astype(np.float32)

    def tex(X, Y):
        x, y = (X * 12.0) % 255, (Y * 12.0) % 255
        x0, y0 = np.clip(np.floor(x).astype(int), 0, 254), np.clip(np.floor(y).astype(int), 0, 254)
        fx, fy = x - x0, y - y0
        return T[y0, x0] * (1 - fx) * (1 - fy) + T[y0, x0 + 1] * fx * (1 - fy) + T[y0 + 1, x0] * (1 - fx) * fy + T[y0 + 1, x0 + 1] * fx * fy
    return tex


def scene_render(C, slant=0.0, seed=1, W=SCENE_W, H=SCENE_H, f=SCENE_F):
    """A back plane z = 4 + slant x and a front rectangle z = 3 (|x| < 0.5, |y| < 0.35), each with a bilinear texture of seeded
    noise at 12 texels per unit, seen from centre C -> (grey [H][W] float32, true depth [H][W])"""
    tex = scene_texture(seed)
    C = np.asarray(C, dtype=np.float64)
    v, u = np.mgrid[0:H, 0:W].astype(np.float64)
    dx, dy = (u - W / 2) / f, (v - H / 2) / f
    tb = (4 + slant * C[0] - C[2]) / (1 - slant * dx)
    tf = (3 - C[2]) * np.ones_like(tb)
    hit = (np.abs(C[0] + tf * dx) < 0.5) & (np.abs(C[1] + tf * dy) < 0.35)
    t = np.where(hit, tf, tb)
    X, Y = C[0] + t * dx, C[1] + t * dy
    return np.where(hit, tex(X + 7.3, Y + 1.1), tex(X, Y)).astype(np.float32), t


def scene(slant=0.0, seed=1):
    """The five frames -> dict(gray [5][H][W], ztrue [5][H][W], P [5][12], ktrue [5][H][W] in planes, range (z_near, z_far))"""
    imgs = [scene_render(C, slant, seed) for C in SCENE_CENTRES]
    izf, izn = SCENE_IZ
    z = np.stack([t for _, t in imgs])               # R = I: the ray parameter is the depth in the camera's frame
    return dict(gray=np.stack([g for g, _ in imgs]), ztrue=z, P=np.stack([scene_camera(C).reshape(12) for C in SCENE_CENTRES]),
                ktrue=(1.0 / z - izf) / (izn - izf) * (SCENE_D - 1), range=(2.0, 6.0))


def all_views(n=5):
    """every frame as the reference, the others as its sources"""
    return np.array([[r] + [j for j in range(n) if j != r] for r in range(n)], dtype=np.int32)


# ---- an independent camera reference: exact rationals and decimals, no cofactor line of pgx.h written out ------------------

U53 = Fraction(1, 2**53)


def _exact_camera(P):
    p = [[Fraction(float(x)) for x in row] for row in np.asarray(P, dtype=np.float64).reshape(3, 4)]
    return [row[:3] for row in p], [row[3] for row in p]


def _perm_terms(M):
    """the six signed terms of the Leibniz determinant"""
    out = []
    for perm in itertools.permutations(range(3)):
        inv = sum(1 for i in range(3) for j in range(i + 1, 3) if perm[i] > perm[j])
        out.append((-1) ** inv * M[0][perm[0]] * M[1][perm[1]] * M[2][perm[2]])
    return out


def _gauss_jordan_inverse(M):
    n = 3
    a = [list(M[i]) + [Fraction(int(i == j)) for j in range(n)] for i in range(n)]
    for c in range(n):
        piv = max(range(c, n), key=lambda i: abs(a[i][c]))
        if a[piv][c] == 0:
            raise ZeroDivisionError("singular camera")
        a[c], a[piv] = a[piv], a[c]
        a[c] = [x / a[c][c] for x in a[c]]
        for i in range(n):
            if i != c and a[i][c] != 0:
                a[i] = [x - a[i][c] * y for x, y in zip(a[i], a[c])]
    return [row[n:] for row in a]


def exact_warp(P_r, P_s):
    """The plane-induced warp of rule 3 in exact rationals of the float64 inputs: A = M_s M_r^-1 by Gauss-Jordan, b = p4_s - A p4_r,
    and a forward-error bound per entry for rule 3 evaluated in float64 (u = 2^-53):
      bound(A_ij) = 16 u N_ij / |det| (1 + D_abs / |det|), N_ij = sum_k |M_s[i][k]| (|a b| + |c d|) over the two products of the
      cofactor that is entry (k, j) of the adjugate, D_abs = the determinant's six terms taken absolute (at most 8 roundings on
      the numerator, at most 7 on det);
      bound(b_i) = 4 u (|p4_s[i]| + sum_k |A_ik| |p4_r[k]|) + sum_k bound(A_ik) |p4_r[k]|.
    -> (A [3][3], b [3], bound_A [3][3], bound_b [3]), all Fractions"""
    Mr, p4r = _exact_camera(P_r)
    Ms, p4s = _exact_camera(P_s)
    inv = _gauss_jordan_inverse(Mr)
    terms = _perm_terms(Mr)
    det, d_abs = abs(sum(terms)), sum(abs(t) for t in terms)
    A = [[sum(Ms[i][k] * inv[k][j] for k in range(3)) for j in range(3)] for i in range(3)]
    b = [p4s[i] - sum(A[i][k] * p4r[k] for k in range(3)) for i in range(3)]
    # entry (k, j) of the adjugate is the minor of M_r without row j and column k: its two products, in absolute value
    mag = [[abs(Mr[(j + 1) % 3][(k + 1) % 3] * Mr[(j + 2) % 3][(k + 2) % 3]) + abs(Mr[(j + 1) % 3][(k + 2) % 3] * Mr[(j + 2) % 3][(k + 1) % 3])
            for j in range(3)] for k in range(3)]
    bA = [[16 * U53 * sum(abs(Ms[i][k]) * mag[k][j] for k in range(3)) / det * (1 + d_abs / det) for j in range(3)] for i in range(3)]
    bb = [4 * U53 * (abs(p4s[i]) + sum(abs(A[i][k]) * abs(p4r[k]) for k in range(3))) + sum(bA[i][k] * abs(p4r[k]) for k in range(3))
          for i in range(3)]
    return A, b, bA, bb


def exact_plane_scale(P_r):
    """sign(det M_r) ||m3_r|| of rule 2 as a Decimal at 200 digits"""
    with decimal.localcontext() as ctx:
        ctx.prec = 200
        M = [[decimal.Decimal(float(x)) for x in row[:3]] for row in np.asarray(P_r, dtype=np.float64).reshape(3, 4)]
        det = sum(_perm_terms(M))
        n3 = (M[2][0] * M[2][0] + M[2][1] * M[2][1] + M[2][2] * M[2][2]).sqrt()
        return n3.copy_sign(det)


def plan_against_exact(P, views, ranges, D, warp, planes):
    """A plan's tables (the yardstick's or the device's; every frame its own slot) against the exact reference, per (r, s) block:
    -> (the worst |warp entry - exact| / its bound, the worst relative error of a w_k against exact_plane_scale (1 / iz_k) in
    units of u = 2^-53, with 1 / iz_k the float64 of rule 2).  Blocks of -1 sources must be NaN, every other one finite."""
    P = np.asarray(P, dtype=np.float64).reshape(-1, 12)
    views = np.asarray(views, dtype=np.int64)
    R, S = views.shape[0], views.shape[1] - 1
    warp, planes = np.asarray(warp, dtype=np.float64).reshape(R, S, 12), np.asarray(planes, dtype=np.float64).reshape(R, D)
    ranges = np.asarray(ranges, dtype=np.float64).reshape(-1, 2)
    worst_w, worst_p = Fraction(0), Fraction(0)
    for r in range(R):
        sn = exact_plane_scale(P[views[r, 0]])
        izf, izn = 1.0 / ranges[r, 1], 1.0 / ranges[r, 0]
        with decimal.localcontext() as ctx:
            ctx.prec = 200
            for k in range(D):
                want = sn * decimal.Decimal(1.0 / (izf + (float(k) / float(D - 1)) * (izn - izf)))
                assert np.isfinite(planes[r, k]), (r, k)
                rel = abs((decimal.Decimal(float(planes[r, k])) - want) / want)
                worst_p = max(worst_p, Fraction(rel) / U53)
        for s in range(S):
            if views[r, 1 + s] < 0:
                assert np.isnan(warp[r, s]).all(), (r, s)
                continue
            assert np.isfinite(warp[r, s]).all(), (r, s)
            A, b, bA, bb = exact_warp(P[views[r, 0]], P[views[r, 1 + s]])
            want = [A[i][j] for i in range(3) for j in range(3)] + b
            bound = [bA[i][j] for i in range(3) for j in range(3)] + bb
            for e in range(12):
                err = abs(Fraction(float(warp[r, s, e])) - want[e])
                if err > 0:
                    worst_w = max(worst_w, err / bound[e] if bound[e] > 0 else Fraction(10**9))
    return float(worst_w), float(worst_p)


# ---- the same two planes seen by general cameras: rotated, rolled, skewed, scaled, mirrored ----------------------------------

ROT_K = np.array([[120.0, 1.5, 51.0], [0.0, 132.0, 30.0], [0.0, 0.0, 1.0]])
ROT_ROLLS = (7.0, -5.0, 11.0, -9.0, 4.0)
ROT_TARGET = (0.0, 0.0, 4.0)
ROT_SCALES = (-2.5, 1.0, 1e-3, 40.0, 0.3)              # any scale, one of them negative
ROT_SCALES_POW2 = (-4.0, 1.0, 2.0**-10, 32.0, 0.25)    # scales that every float64 operation of the rule commutes with
# frame 0 as the reference of row 0 only: with a negative scale it is no valid source (rule 4's q_2 > 0)
ROT_VIEWS = np.array([[0, 1, 2, 3, 4], [1, 2, 3, 4, -1], [2, 1, 3, 4, -1], [3, 1, 2, 4, -1], [4, 1, 2, 3, -1]], dtype=np.int32)


def posed_camera(K, R, C, lam=1.0):
    """lam K [R | -R C] as [3][4]; lam multiplies the finished float64 matrix, so a power of two scales it exactly"""
    R = np.asarray(R, dtype=np.float64)
    return lam * (np.asarray(K, dtype=np.float64) @ np.hstack([R, -(R @ np.asarray(C, dtype=np.float64))[:, None]]))


def look_at(C, target, roll_deg):
    """The rotation (world -> camera) whose optical axis points from C at target, x to the right of world y, then rolled about
    the optical axis by roll_deg"""
    z = np.asarray(target, dtype=np.float64) - np.asarray(C, dtype=np.float64)
    z /= np.linalg.norm(z)
    x = np.cross([0.0, 1.0, 0.0], z)
    x /= np.linalg.norm(x)
    c, s = np.cos(np.radians(roll_deg)), np.sin(np.radians(roll_deg))
    return np.array([[c, -s, 0.0], [s, c, 0.0], [0.0, 0.0, 1.0]]) @ np.stack([x, np.cross(z, x), z])


def scaled_cameras(P, scales):
    return np.asarray(P, dtype=np.float64).reshape(-1, 12) * np.asarray(scales, dtype=np.float64)[:, None]


def scene_rotated(seed=1, W=SCENE_W, H=SCENE_H):
    """scene()'s world (back plane z = 4, front rectangle z = 3, scene_render's textures) from SCENE_CENTRES, every optical axis
    at ROT_TARGET and rolled by ROT_ROLLS, through ROT_K (skew, two focal lengths, an off-centre principal point).  Pixel (u, v)
    sees along C + t R^T K^-1 (u, v, 1).  -> dict(gray [5][H][W], ztrue [5][H][W] = R[2] . (X - C), X [5][H][W][3], P [5][12]
    at scale 1, R, C, ktrue in planes, range)"""
    tex = scene_texture(seed)
    v, u = np.mgrid[0:H, 0:W].astype(np.float64)
    pix = np.stack([u, v, np.ones_like(u)], -1)
    Kinv = np.linalg.inv(ROT_K)
    gray, ztrue, Xs, Ps, Rs = [], [], [], [], []
    for C, roll in zip(SCENE_CENTRES, ROT_ROLLS):
        C = np.asarray(C, dtype=np.float64)
        Rm = look_at(C, ROT_TARGET, roll)
        d = pix @ (Rm.T @ Kinv).T                     # the ray directions in the world
        tb, tf = (4.0 - C[2]) / d[..., 2], (3.0 - C[2]) / d[..., 2]
        Xf = C + tf[..., None] * d
        hit = (np.abs(Xf[..., 0]) < 0.5) & (np.abs(Xf[..., 1]) < 0.35)
        X = np.where(hit[..., None], Xf, C + tb[..., None] * d)
        gray.append(np.where(hit, tex(X[..., 0] + 7.3, X[..., 1] + 1.1), tex(X[..., 0], X[..., 1])).astype(np.float32))
        ztrue.append((X - C) @ Rm[2])
        Xs.append(X)
        Ps.append(posed_camera(ROT_K, Rm, C).reshape(12))
        Rs.append(Rm)
    z = np.stack(ztrue)
    izf, izn = SCENE_IZ
    return dict(gray=np.stack(gray), ztrue=z, X=np.stack(Xs), P=np.stack(Ps), R=np.stack(Rs), C=np.array(SCENE_CENTRES),
                ktrue=(1.0 / z - izf) / (izn - izf) * (SCENE_D - 1), range=(2.0, 6.0))


def assert_scaled_tables(plain, scaled, views, lam):
    """Cameras scaled by powers of two lam[f] scale the tables exactly: w_k by lam_r, A by lam_s / lam_r, b by lam_s"""
    views, lam = np.asarray(views), np.asarray(lam, dtype=np.float64)
    for r in range(len(views)):
        lr = lam[views[r, 0]]
        assert (scaled["planes"][r] == lr * plain["planes"][r]).all(), r
        for s, f in enumerate(views[r, 1:]):
            if f < 0:
                assert np.isnan(scaled["warp"][r, s]).all() and np.isnan(plain["warp"][r, s]).all()
                continue
            assert np.isfinite(scaled["warp"][r, s]).all(), (r, s)
            assert (scaled["warp"][r, s, :9] == (lam[f] / lr) * plain["warp"][r, s, :9]).all(), (r, s)
            assert (scaled["warp"][r, s, 9:] == lam[f] * plain["warp"][r, s, 9:]).all(), (r, s)


def saturated_case(W=35, H=34, S=8, D=9):
    """The largest raw cost the rule can give: the reference image x + W y, S sources that are its negative (every census bit
    the other way), 1 + S identical cameras (the warp is the identity at every plane) -> gray, P, views, ranges, parameters"""
    v, u = np.mgrid[0:H, 0:W]
    g = (u + W * v).astype(np.float32)
    gray = np.stack([g] + [-g] * S)
    P = np.stack([scene_camera((0.0, 0.0, 0.0), W, H, 40.0).reshape(12)] * (1 + S))
    return gray, P, np.arange(1 + S, dtype=np.int32)[None], [(2.0, 6.0)], dict(D=D, a=3, min_views=S)


def within_one_plane(kq8, flags, ktrue):
    """per map the fraction of its pixels that carry no flag and lie within one plane of the truth"""
    good = (np.asarray(flags) == 0) & (np.abs(np.asarray(kq8) / 256.0 - ktrue) <= 1.0)
    return good.reshape(len(good), -1).mean(1)
