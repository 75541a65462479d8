"""The yardstick of the cloud merge (include/pgx.h: pgx_cloud_merge_dev, pgx_rgba8_batch_dev), operation by operation in the
header's order, in two forms that share no line of the rule: `merge`, vectorised numpy (np.unique on the keys, np.add.at on int64,
np.minimum.at), and `merge_loop`, one loop per point in Python ints, floats and a dict, with its own back-projection.  Python
floats and numpy float64 do not contract a b + c, which is what the library's -ffp-contract=off build does.  The constants of
k_cloud.hip that the GPU tests size their cases by are read from the source (kernel_constants), and its hash is restated
(table_hash).  A plain helper module."""
import math
import os
import re

import numpy as np

import depth_ref

GB = 1 << 20           # the bias of a cell coordinate in the key
INT_KEYS = ("keys", "cnt", "sp", "nn", "sn", "nc", "sc", "first", "info", "rgba8", "pt_normal", "has_normal", "cell_of", "report")
FLOAT_KEYS = ("xyz", "normal")


def bits(a):
    return np.ascontiguousarray(a).view(np.uint8).tobytes()


# ---- pgx_rgba8_batch_dev --------------------------------------------------------------------------------------------------

def pack_rgba8(dewarped):
    """pgx_dewarp's output [..][4] (uint16: the high byte of each channel; uint8: the bytes) -> uint32, channel c in bits 8 c.."""
    d = np.asarray(dewarped)
    b = (d >> 8).astype(np.uint32) if d.dtype == np.uint16 else d.astype(np.uint32)
    return b[..., 0] | b[..., 1] << np.uint32(8) | b[..., 2] << np.uint32(16) | b[..., 3] << np.uint32(24)


# ---- the vectorised form ----------------------------------------------------------------------------------------------------

def _backproject(cam, u, v, z):
    """the filter's back-projection (depth_ref.fuse's lines) of pixels (u, v) at depths z, arrays -> [3] arrays"""
    _, adj, det, sg, n3, p4 = cam
    with np.errstate(all="ignore"):
        w = (sg * n3) * z
        t = [w * u - p4[0], w * v - p4[1], w - p4[2]]
        return [((adj[i, 0] * t[0] + adj[i, 1] * t[1]) + adj[i, 2] * t[2]) / det for i in range(3)]


def _diff(cam, dmap, u, v, du, dv, z, Xc, disc_tol):
    H, W = dmap.shape
    out = []
    for sgn in (1, -1):
        uu, vv = u + sgn * du, v + sgn * dv
        inside = (uu >= 0) & (uu < W) & (vv >= 0) & (vv < H)
        zz = dmap[np.where(inside, vv, 0), np.where(inside, uu, 0)]
        with np.errstate(all="ignore"):
            counts = inside & np.isfinite(zz) & (np.abs(zz - z) <= disc_tol * z)
        out.append((counts, _backproject(cam, uu.astype(np.float64), vv.astype(np.float64), zz)))
    (f, Xf), (b, Xb) = out
    with np.errstate(all="ignore"):
        d = [np.where(f & b, Xf[i] - Xb[i], np.where(f, Xf[i] - Xc[i], Xc[i] - Xb[i])) for i in range(3)]
    return f | b, d


def point_normals(src_r, pix, used, depth, views, n_frames, P, k, disc_tol):
    """rule 2 for the used points -> (has [n] bool, q [n][3] int32)"""
    R, H, W = depth.shape
    n = len(pix)
    has, q = np.zeros(n, dtype=bool), np.zeros((n, 3), dtype=np.int32)
    for r in range(R):
        f = int(views[r, 0])
        if not 0 <= f < n_frames:
            continue
        cam = depth_ref.camera(P[f])
        if not cam[0]:
            continue
        idx = np.flatnonzero(used & (src_r == r))
        if not len(idx):
            continue
        v, u = pix[idx] // W, pix[idx] % W
        z = depth[r][v, u]
        fu, fv = u.astype(np.float64), v.astype(np.float64)
        Xc = _backproject(cam, fu, fv, z)
        hu, du = _diff(cam, depth[r], u, v, k, 0, z, Xc, disc_tol)
        hv, dv = _diff(cam, depth[r], u, v, 0, k, z, Xc, disc_tol)
        adj = cam[1]
        with np.errstate(all="ignore"):
            nv = [du[1] * dv[2] - du[2] * dv[1], du[2] * dv[0] - du[0] * dv[2], du[0] * dv[1] - du[1] * dv[0]]
            e = [(adj[i, 0] * fu + adj[i, 1] * fv) + adj[i, 2] for i in range(3)]
            s = (nv[0] * e[0] + nv[1] * e[1]) + nv[2] * e[2]
            L = np.sqrt((nv[0] * nv[0] + nv[1] * nv[1]) + nv[2] * nv[2])
            ok = np.isfinite(z) & hu & hv & np.isfinite(L) & (L != 0) & np.isfinite(s) & (s != 0)
            for a in range(3):
                m = np.where(s > 0, -nv[a], nv[a]) / L
                q[idx, a] = np.where(ok, np.floor(np.where(ok, m, 0.0) * 32767.0 + 0.5), 0).astype(np.int32)
        has[idx] = ok
    return has, q


def merge(xyz, src, depth, views, n_frames, P, cell, origin, k=1, disc_tol=0.02, min_support=1, rgba8=None, frame_ids=None,
          count=None):
    """pgx_cloud_merge_dev without the capacity.  xyz [max_in][3], src [max_in][2]; count = d_count[0] or None.
    -> dict: per cell in ascending first keys, cnt, sp [c][3], nn, sn [c][3], nc, sc [c][3], first (every cell), kept [c] bool;
    per kept cell xyz, normal, rgba8, info; per point pt_normal, has_normal, cell_of; report [8]"""
    xyz = np.asarray(xyz, dtype=np.float64).reshape(-1, 3)
    src = np.asarray(src, dtype=np.int64).reshape(-1, 2)
    depth = np.asarray(depth, dtype=np.float64)
    R, H, W = depth.shape
    views = np.asarray(views, dtype=np.int64).reshape(R, -1)
    P = np.asarray(P, dtype=np.float64).reshape(-1, 12)
    max_in = len(xyz)
    n = max_in if count is None else min(max(int(count), 0), max_in)
    X, r, pix = xyz[:n], src[:n, 0], src[:n, 1]
    o = np.asarray(origin, dtype=np.float64)
    with np.errstate(all="ignore"):
        t = (X - o) / cell
        g = np.floor(t)
        used = np.isfinite(X).all(1) & (r >= 0) & (r < R) & (pix >= 0) & (pix < W * H) & ((g >= -GB) & (g < GB)).all(1)
        gi = np.where(used[:, None], g, 0).astype(np.int64)
        p = np.where(used[:, None], np.floor((t - g) * 65536.0), 0).astype(np.int64)
    key = (gi[:, 0] + GB) << 42 | (gi[:, 1] + GB) << 21 | (gi[:, 2] + GB)
    rs, ps = np.where(used, r, 0), np.where(used, pix, 0)
    has, q = point_normals(rs, ps, used, depth, views, n_frames, P, k, disc_tol)
    hasc, col = np.zeros(n, dtype=bool), np.zeros(n, dtype=np.int64)
    if rgba8 is not None:
        rgba8 = np.asarray(rgba8, dtype=np.uint32)
        F = len(rgba8)
        slot = np.array([depth_ref.slot_of(frame_ids, F, n_frames, int(f)) for f in views[:, 0]], dtype=np.int64)
        hasc = used & (slot[rs] >= 0)
        col = np.where(hasc, rgba8.reshape(F, -1)[np.where(hasc, slot[rs], 0), ps] & np.uint32(0xFFFFFF), 0).astype(np.int64)
    ui = np.flatnonzero(used)
    ukeys, inv = np.unique(key[ui], return_inverse=True)
    C = len(ukeys)
    first = np.full(C, np.iinfo(np.int64).max, dtype=np.int64)
    np.minimum.at(first, inv, ui)
    order = np.argsort(first)
    rank = np.empty(C, dtype=np.int64)
    rank[order] = np.arange(C)
    cidx = rank[inv]                          # the cell of each used point, cells numbered in ascending first
    cnt, nn, nc = (np.zeros(C, dtype=np.int64) for _ in range(3))
    sp, sn, sc = (np.zeros((C, 3), dtype=np.int64) for _ in range(3))
    np.add.at(cnt, cidx, 1)
    np.add.at(sp, cidx, p[ui])
    hn, hc = has[ui], hasc[ui]
    np.add.at(nn, cidx[hn], 1)
    np.add.at(sn, cidx[hn], q[ui][hn].astype(np.int64))
    np.add.at(nc, cidx[hc], 1)
    np.add.at(sc, cidx[hc], np.stack([(col[ui][hc] >> (8 * c)) & 255 for c in range(3)], 1))
    keys, first = ukeys[order], first[order]
    kept = cnt >= min_support
    out_of = np.where(kept, np.cumsum(kept) - 1, -2)
    cell_of = np.full(n, -1, dtype=np.int32)
    cell_of[ui] = out_of[cidx]
    kk = np.flatnonzero(kept)
    gk = np.stack([(keys[kk] >> 42) & 0x1FFFFF, (keys[kk] >> 21) & 0x1FFFFF, keys[kk] & 0x1FFFFF], 1) - GB
    c2 = cnt[kk][:, None]
    out_xyz = o + (gk.astype(np.float64) + ((2 * sp[kk] + c2).astype(np.float64) / (2 * c2).astype(np.float64)) / 65536.0) * cell
    s = sn[kk].astype(np.float64)
    L = np.sqrt((s[:, 0] * s[:, 0] + s[:, 1] * s[:, 1]) + s[:, 2] * s[:, 2])
    hnrm = (nn[kk] != 0) & (L != 0)
    with np.errstate(all="ignore"):
        normal = np.where(hnrm[:, None], s / np.where(hnrm, L, 1.0)[:, None], 0.0).astype(np.float32)
    n2 = np.maximum(nc[kk], 1)[:, None]
    ch = (2 * sc[kk] + n2) // (2 * n2)
    rgb = np.where(nc[kk] != 0, ch[:, 0] | ch[:, 1] << 8 | ch[:, 2] << 16 | 255 << 24, 0).astype(np.uint32)
    info = np.stack([cnt[kk], nn[kk], nc[kk], first[kk]], 1).astype(np.int32)
    report = np.array([n, used.sum(), n - used.sum(), has.sum(), hasc.sum(), C, kept.sum(), 0], dtype=np.int32)
    return dict(keys=keys, cnt=cnt, sp=sp, nn=nn, sn=sn, nc=nc, sc=sc, first=first, kept=kept, xyz=out_xyz, normal=normal, rgba8=rgb,
                info=info, pt_normal=np.where(has[:, None], q, 0).astype(np.int32), has_normal=has, cell_of=cell_of, report=report,
                used=used, p=p, g=gi)


# ---- the restatement: one loop per point, Python ints and floats, a dict ---------------------------------------------------------

def _camera_loop(P12):
    """-> None for an unknown camera, else (adj rows, det, sign * ||m3||, p4) in Python floats, cofactors written out per entry"""
    p = [float(x) for x in P12]
    if not all(math.isfinite(x) for x in p):
        return None
    M = [p[0:3], p[4:7], p[8:11]]

    def cof(i, j):   # entry (i, j) of the adjugate: the minor of M without row j and column i, a b - c d
        r0, r1 = [x for x in range(3) if x != j]
        c0, c1 = [x for x in range(3) if x != i]
        a, b, c, d = M[r0][c0], M[r1][c1], M[r0][c1], M[r1][c0]
        return (a * b - c * d) if (i + j) % 2 == 0 else (c * d - a * b)
    adj = [[cof(i, j) for j in range(3)] for i in range(3)]
    det = (M[0][0] * adj[0][0] + M[0][1] * adj[1][0]) + M[0][2] * adj[2][0]
    if det == 0.0:
        return None
    n3 = math.sqrt((M[2][0] * M[2][0] + M[2][1] * M[2][1]) + M[2][2] * M[2][2])
    return adj, det, (1.0 if det > 0.0 else -1.0) * n3, (p[3], p[7], p[11])


def _point_loop(cam, u, v, z):
    adj, det, sn, p4 = cam
    w = sn * z
    t = (w * float(u) - p4[0], w * float(v) - p4[1], w - p4[2])
    return [((adj[i][0] * t[0] + adj[i][1] * t[1]) + adj[i][2] * t[2]) / det for i in range(3)]


def _fdiv(a, b):
    """IEEE a / b for Python floats (b == 0 included)"""
    return float(np.float64(a) / np.float64(b))


def merge_loop(xyz, src, depth, views, n_frames, P, cell, origin, k=1, disc_tol=0.02, min_support=1, rgba8=None, frame_ids=None,
               count=None):
    """The same rule one point at a time.  -> the same dict as merge (without used, p, g)"""
    xyz = np.asarray(xyz, dtype=np.float64).reshape(-1, 3)
    src = np.asarray(src).reshape(-1, 2)
    depth = np.asarray(depth, dtype=np.float64)
    R, H, W = depth.shape
    views = np.asarray(views).reshape(R, -1)
    P = np.asarray(P, dtype=np.float64).reshape(-1, 12)
    n = len(xyz) if count is None else min(max(int(count), 0), len(xyz))
    cams = [(_camera_loop(P[int(f)]) if 0 <= int(f) < n_frames else None) for f in views[:, 0]]
    F = 0 if rgba8 is None else len(rgba8)
    cells, order = {}, []
    ptn, hasn_all, cell_key = np.zeros((n, 3), dtype=np.int32), np.zeros(n, dtype=bool), [None] * n
    n_used = n_norm = n_col = 0
    with np.errstate(all="ignore"):
        for i in range(n):
            X = [float(x) for x in xyz[i]]
            r, pix = int(src[i, 0]), int(src[i, 1])
            if not all(math.isfinite(x) for x in X) or not 0 <= r < R or not 0 <= pix < W * H:
                continue
            t = [_fdiv(X[a] - float(origin[a]), float(cell)) for a in range(3)]
            if not all(math.isfinite(x) for x in t):
                continue
            g = [math.floor(x) for x in t]
            if not all(-GB <= x < GB for x in g):
                continue
            n_used += 1
            key = (g[0] + GB) << 42 | (g[1] + GB) << 21 | (g[2] + GB)
            p = [math.floor((t[a] - float(g[a])) * 65536.0) for a in range(3)]
            v, u = divmod(pix, W)
            q, cam, z = None, cams[r], float(depth[r, v, u])
            if cam is not None and math.isfinite(z):
                Xc = _point_loop(cam, u, v, z)

                def diff(du, dv):
                    pts = []
                    for sgn in (1, -1):
                        uu, vv = u + sgn * du, v + sgn * dv
                        zz = float(depth[r, vv, uu]) if 0 <= uu < W and 0 <= vv < H else math.nan
                        pts.append(_point_loop(cam, uu, vv, zz) if math.isfinite(zz) and abs(zz - z) <= disc_tol * z else None)
                    f, b = pts
                    if f and b:
                        return [f[a] - b[a] for a in range(3)]
                    if f:
                        return [f[a] - Xc[a] for a in range(3)]
                    if b:
                        return [Xc[a] - b[a] for a in range(3)]
                    return None
                du, dv = diff(k, 0), diff(0, k)
                if du and dv:
                    nv = [du[1] * dv[2] - du[2] * dv[1], du[2] * dv[0] - du[0] * dv[2], du[0] * dv[1] - du[1] * dv[0]]
                    e = [(cam[0][a][0] * float(u) + cam[0][a][1] * float(v)) + cam[0][a][2] for a in range(3)]
                    s = (nv[0] * e[0] + nv[1] * e[1]) + nv[2] * e[2]
                    L2 = (nv[0] * nv[0] + nv[1] * nv[1]) + nv[2] * nv[2]
                    L = math.sqrt(L2) if L2 >= 0 and math.isfinite(L2) else math.nan if L2 != L2 else math.inf
                    if math.isfinite(L) and L != 0.0 and math.isfinite(s) and s != 0.0:
                        q = [math.floor(((-x if s > 0 else x) / L) * 32767.0 + 0.5) for x in nv]
            colour = None
            if rgba8 is not None:
                sl = depth_ref.slot_of(frame_ids, F, n_frames, int(views[r, 0]))
                if sl >= 0:
                    colour = int(np.asarray(rgba8).reshape(F, -1)[sl, pix]) & 0xFFFFFF
            if key not in cells:
                cells[key] = dict(cnt=0, sp=[0, 0, 0], nn=0, sn=[0, 0, 0], nc=0, sc=[0, 0, 0], first=i)
                order.append(key)
            c = cells[key]
            cell_key[i] = key
            c["cnt"] += 1
            for a in range(3):
                c["sp"][a] += p[a]
            if q is not None:
                n_norm += 1
                c["nn"] += 1
                ptn[i], hasn_all[i] = q, True
                for a in range(3):
                    c["sn"][a] += q[a]
            if colour is not None:
                n_col += 1
                c["nc"] += 1
                for a in range(3):
                    c["sc"][a] += (colour >> (8 * a)) & 255
    C = len(order)
    get = lambda name: np.array([cells[kx][name] for kx in order], dtype=np.int64).reshape((C, 3) if name[0] == "s" else (C,))  # noqa: E731
    out_index, xyz_o, nrm_o, rgb_o, info_o = {}, [], [], [], []
    for kx in order:
        c = cells[kx]
        if c["cnt"] < min_support:
            out_index[kx] = -2
            continue
        out_index[kx] = len(xyz_o)
        g = [((kx >> sh) & 0x1FFFFF) - GB for sh in (42, 21, 0)]
        xyz_o.append([float(origin[a]) + (float(g[a]) + (float(2 * c["sp"][a] + c["cnt"]) / float(2 * c["cnt"])) / 65536.0) * float(cell)
                      for a in range(3)])
        s = [float(x) for x in c["sn"]]
        L = math.sqrt((s[0] * s[0] + s[1] * s[1]) + s[2] * s[2])
        nrm_o.append([np.float32(x / L) for x in s] if c["nn"] and L != 0.0 else [np.float32(0)] * 3)
        ch = [(2 * x + c["nc"]) // (2 * c["nc"]) for x in c["sc"]] if c["nc"] else None
        rgb_o.append((ch[0] | ch[1] << 8 | ch[2] << 16 | 255 << 24) if ch else 0)
        info_o.append([c["cnt"], c["nn"], c["nc"], c["first"]])
    cell_of = np.array([-1 if kx is None else out_index[kx] for kx in cell_key], dtype=np.int32).reshape(n)
    cnt = get("cnt")
    return dict(keys=np.array(order, dtype=np.int64).reshape(C), cnt=cnt, sp=get("sp"), nn=get("nn"), sn=get("sn"), nc=get("nc"),
                sc=get("sc"), first=get("first"), kept=cnt >= min_support, xyz=np.array(xyz_o, dtype=np.float64).reshape(-1, 3),
                normal=np.array(nrm_o, dtype=np.float32).reshape(-1, 3), rgba8=np.array(rgb_o, dtype=np.uint32).reshape(-1),
                info=np.array(info_o, dtype=np.int32).reshape(-1, 4), pt_normal=ptn, has_normal=hasn_all, cell_of=cell_of,
                report=np.array([n, n_used, n - n_used, n_norm, n_col, C, len(xyz_o), 0], dtype=np.int32))


def assert_same(a, b, keys=INT_KEYS + FLOAT_KEYS):
    for k in keys:
        x, y = np.asarray(a[k]), np.asarray(b[k])
        assert x.shape == y.shape, (k, x.shape, y.shape)
        if k in FLOAT_KEYS:
            assert bits(x.astype(y.dtype)) == bits(y), (k, np.argwhere(x != y)[:5])
        else:
            assert (x.astype(np.int64) == y.astype(np.int64)).all(), (k, np.argwhere(x != y)[:5])


def by_key(m):
    """a merge's cells sorted by key: what a permuted list must leave unchanged"""
    o = np.argsort(m["keys"])
    return {k: np.asarray(m[k])[o] for k in ("keys", "cnt", "sp", "nn", "sn", "nc", "sc")}


# ---- k_cloud.hip's constants and hash ------------------------------------------------------------------------------------------

def kernel_constants(csrc):
    text = open(os.path.join(csrc, "k_cloud.hip")).read()
    c = {k: int(v) for k, v in re.findall(r"\b(CLD_NT|CLD_GRID_MAX|CLD_LG_TMIN|CLD_ACC) = (\d+)", text)}
    c["CLD_HASH_MUL"] = int(re.search(r"CLD_HASH_MUL = (0x[0-9A-Fa-f]+)ull", text).group(1), 16)
    assert "(key * CLD_HASH_MUL) >> (64 - lg)" in text and "h = (h + 1) & mask" in text   # the hash and the probe restated below
    assert "< 2 * (size_t)a.max_in" in text                                              # ... and the table's size
    return c


def table_lg(max_in, c):
    lg = c["CLD_LG_TMIN"]
    while (1 << lg) < 2 * max_in:
        lg += 1
    return lg


def table_hash(key, lg, c):
    return ((int(key) * c["CLD_HASH_MUL"]) & (2**64 - 1)) >> (64 - lg)


def key_of(g):
    return (int(g[0]) + GB) << 42 | (int(g[1]) + GB) << 21 | (int(g[2]) + GB)


# ---- cases and scenes ----------------------------------------------------------------------------------------------------------------------

CELL, ORIGIN = 1.0 / 32.0, (-8.0, -8.0, -8.0)     # the grid of the scene tests

# the fraction of normals within 20 degrees of the truth that the yardstick measures on the sweep's depths (32 coarse planes: the
# sweep's noise, not the rule's), less 0.01 and rounded down to two digits (DESIGN.md section 28 has the measured figures):
# (case, k) -> (points with a normal, cells with support >= 3)
# measured: plain 0.9541 / 0.9959 (k = 1), 0.9828 / 0.9988 (k = 3); rotated 0.6608 / 0.8901 (k = 1), 0.8523 / 0.9727 (k = 3)
FLOORS = {("plain", 1): (0.94, 0.98), ("plain", 3): (0.97, 0.98), ("rotated", 1): (0.65, 0.88), ("rotated", 3): (0.84, 0.96)}


def boundary_case(seed=2):
    """a 12 x 9 rig of three maps (one of them skipped: an unknown camera) with smooth depths, and a list that holds every pixel
    twice, non-finite coordinates, bad src, and a point in every boundary cell"""
    rng = np.random.default_rng(seed)
    W, H = 12, 9
    C = [(0.0, 0.0, 0.0), (0.3, 0.0, 0.0), (0.0, 0.25, 0.0)]
    P = np.stack([depth_ref.scene_camera(c, W, H, 14.0).reshape(12) for c in C] + [np.full(12, np.nan)])
    views = np.array([[0, 1, 2], [1, 0, 2], [3, 0, 1]], dtype=np.int32)       # map 2: frame 3 has no camera
    v, u = np.mgrid[0:H, 0:W]
    depth = np.stack([3.0 + 0.02 * u + 0.01 * v, 3.5 - 0.015 * u + 0.0 * v, 4.0 + 0.0 * u + 0.0 * v]).astype(np.float64)
    depth[0, 4, 5] = np.nan
    depth[1, 2, 3] = 9.0                                                      # a discontinuity
    f = depth_ref.fuse(np.where(np.isfinite(depth), depth, 3.0), views, 4, P, 0.5, 0)
    xyz, src = f["xyz"], f["src"]
    xyz = np.concatenate([xyz, xyz[::3] + 1e-3, rng.uniform(-1, 1, (40, 3))])
    src = np.concatenate([src, src[::3], np.stack([rng.integers(0, 3, 40), rng.integers(0, W * H, 40)], 1)]).astype(np.int32)
    # map 2's pixels: the filter skips the map, the merge still bins points that name it
    xyz = np.concatenate([xyz, rng.uniform(-1, 1, (10, 3))])
    src = np.concatenate([src, np.stack([np.full(10, 2), rng.integers(0, W * H, 10)], 1)]).astype(np.int32)
    bad = np.array([[np.nan, 0, 0], [0, np.inf, 0], [0, 0, -np.inf], [0.5, 0.5, 0.5], [0.5, 0.5, 0.5], [0.5, 0.5, 0.5], [0.5, 0.5, 0.5]])
    bad_src = np.array([[0, 1], [0, 2], [1, 3], [-1, 0], [3, 0], [0, -1], [0, W * H]], dtype=np.int32)
    lo, hi = ORIGIN[0] - GB * CELL, ORIGIN[0] + GB * CELL            # the grid's faces
    edge = []
    for a in range(3):
        for x in (lo, hi - CELL, lo - CELL, hi, np.nextafter(hi, 0.0), np.nextafter(lo, -np.inf)):
            e = [0.25, 0.25, 0.25]
            e[a] = x
            edge.append(e)
    edge = np.array(edge)
    xyz = np.concatenate([xyz, bad, edge])
    src = np.concatenate([src, bad_src, np.tile([[0, 7]], (len(edge), 1))]).astype(np.int32)
    perm = rng.permutation(len(xyz))
    rgba8 = rng.integers(0, 2**32, (3, H, W), dtype=np.uint32)              # slots: frames 1, 0, 2; frame 3 has none
    return dict(xyz=xyz[perm], src=src[perm], depth=depth, views=views, P=P, rgba8=rgba8, frame_ids=np.array([1, 0, 2], np.int32), W=W, H=H)


def angle_to(normals, target):
    """the angle in radians between each row and the unit vector target (rows of zeros give pi)"""
    nv = np.asarray(normals, dtype=np.float64)
    ln = np.linalg.norm(nv, axis=1)
    c = np.where(ln > 0, (nv @ np.asarray(target, dtype=np.float64)) / np.where(ln > 0, ln, 1.0), -1.0)
    return np.arccos(np.clip(c, -1.0, 1.0))


def grey_to_rgba16(gray):
    """frames of grey in [0, 1] -> [F][H][W][4] uint16 with channels g, g / 2, g / 4 and full alpha: three different bytes"""
    g = np.round(np.asarray(gray, dtype=np.float64) * 65535.0).astype(np.uint16)
    return np.stack([g, g // 2, g // 4, np.full_like(g, 65535)], -1)
