"""The yardstick of the mesh's decimation (include/pgx.h: pgx_mesh_decimate_dev), operation by operation in the header's order, in
two forms that share no code beyond the input layout (mesh_clean_ref._prep): `decimate`, vectorised numpy (np.unique over block
rows, np.add.at on int64 for every sum), and `decimate_loop`, one loop per triangle and vertex in Python ints (wrapped to int64 by
hand) and floats with dicts for the tables.  The constants of k_meshdecimate.hip that the GPU tests size their cases by are read
from the source (kernel_constants), and its keys and hashes are restated (block_key, table_hash, triple_hash), held to the kernel's
text.  The shapes and scenes are mesh_clean_ref's, by import.  A plain helper module."""
import functools
import math
import os
import re

import numpy as np

import mesh_clean_ref as C
import mesh_ref

bits = C.bits
OUT_KEYS = ("xyz", "normal", "rgba8", "info", "tri")
INT_KEYS = ("rgba8", "info", "tri", "vertex_map", "level", "report")
FLOAT_KEYS = ("xyz", "normal")
LIM = C.LIM
Q_MAX = 2**36 - 1
CELL, ORIGIN = C.CELL, C.ORIGIN


# ---- the vectorised form ----------------------------------------------------------------------------------------------------

def _tri_m(qa, qb, qc, scale):
    """floor((n / L) * scale + 0.5) of the triangles' normals on int64 positions [k][3], zeros where L is 0 or not finite"""
    with np.errstate(all="ignore"):
        e1, e2 = (qb - qa).astype(np.float64), (qc - qa).astype(np.float64)
        n = np.stack([e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1], e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2],
                      e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]], 1)
        L = np.sqrt((n[:, 0] * n[:, 0] + n[:, 1] * n[:, 1]) + n[:, 2] * n[:, 2])
        ok = (L != 0) & np.isfinite(L)
        return np.where(ok[:, None], np.floor((np.where(ok[:, None], n, 0.0) / np.where(ok, L, 1.0)[:, None]) * scale + 0.5), 0.0).astype(np.int64)


def decimate(xyz, normal, rgba8, info, tri, cell, origin, lmin=0, lmax=3, flat_q=1015, counts=None):
    """pgx_mesh_decimate_dev without the capacities -> dict: the outputs xyz, normal, rgba8, info, tri; vertex_map [nv], level
    [nv], report [8]; and for the tests q [nv][3] int64, Q [vertices out][3] int64, kept_tri [nt] bool, src_tri (the old index of
    every output triangle)"""
    xyz, normal, rgba8, info, tri, nv, nt = C._prep(xyz, normal, rgba8, info, tri, counts)
    o = np.asarray(origin, dtype=np.float64)
    cell, lmin, lmax, flat_q = float(cell), int(lmin), int(lmax), int(flat_q)
    X, T = xyz[:nv], tri[:nt].astype(np.int64)
    # 1 valid / used / q
    with np.errstate(all="ignore"):
        t = (X - o) / cell
        valid = np.isfinite(X).all(1) & ((t >= -LIM) & (t < LIM)).all(1)
        q = np.where(valid[:, None], np.floor(np.where(valid[:, None], t, 0.0) * 65536.0 + 0.5), 0.0).astype(np.int64)
    q = np.minimum(q, Q_MAX)
    inr = ((T >= 0) & (T < nv)).all(1)
    Tc = np.where(inr[:, None], T, 0)
    used = inr & (Tc[:, 0] != Tc[:, 1]) & (Tc[:, 0] != Tc[:, 2]) & (Tc[:, 1] != Tc[:, 2])
    if nv:
        used &= valid[Tc].all(1)
    U = T[used]
    uidx = np.flatnonzero(used)
    member = np.bincount(U.reshape(-1), minlength=nv) > 0
    # 2 triangle normals
    m = _tri_m(q[U[:, 0]], q[U[:, 1]], q[U[:, 2]], 1024.0) if len(U) else np.zeros((0, 3), dtype=np.int64)
    # 3, 4 blocks, the flat test, the level
    lev = np.full(nv, lmin, dtype=np.int64)
    sofar = member.copy()
    corners, mm = U.reshape(-1), np.repeat(m, 3, axis=0)
    for l in range(lmin + 1, lmax + 1):
        if not len(U):
            break
        B = q >> (16 + l)
        _, inv = np.unique(B[corners], axis=0, return_inverse=True)
        inv = inv.reshape(-1)
        N = np.bincount(inv).astype(np.int64)
        S = np.zeros((len(N), 3), dtype=np.int64)
        np.add.at(S, inv, mm)
        with np.errstate(all="ignore"):
            S2 = (S[:, 0] * S[:, 0] + S[:, 1] * S[:, 1]) + S[:, 2] * S[:, 2]
            flat = S2.astype(np.float64) >= float(flat_q * flat_q) * (N.astype(np.float64) * N.astype(np.float64))
        vflat = np.zeros(nv, dtype=bool)
        vflat[corners] = flat[inv]
        sofar &= vflat
        lev[sofar] = l
    # 5 clusters
    mem = np.flatnonzero(member)
    Lm = lev[mem]
    Bm = q[mem] >> (16 + Lm)[:, None]
    _, cid = np.unique(np.concatenate([Lm[:, None], Bm], 1), axis=0, return_inverse=True)
    cid = cid.reshape(-1)
    nc = int(cid.max()) + 1 if len(mem) else 0
    name = np.full(nc, nv, dtype=np.int64)
    np.minimum.at(name, cid, mem)
    cn = np.bincount(cid, minlength=nc).astype(np.int64)
    org = Bm << (16 + Lm)[:, None]
    s = np.zeros((nc, 3), dtype=np.int64)
    np.add.at(s, cid, q[mem] - org)
    sc = np.zeros((nc, 4), dtype=np.int64)
    by = ((rgba8[:nv][mem].astype(np.int64)[:, None] >> (8 * np.arange(4))) & 0xFF)
    np.add.at(sc, cid, by)
    corg = np.zeros((nc, 3), dtype=np.int64)
    corg[cid] = org
    clev = np.zeros(nc, dtype=np.int64)
    clev[cid] = Lm
    den = np.maximum(2 * cn, 1)
    Q = corg + (2 * s + cn[:, None]) // den[:, None]
    col = (2 * sc + cn[:, None]) // den[:, None]
    vc = np.full(nv, -1, dtype=np.int64)
    vc[mem] = cid
    # 6 triangles
    c3 = vc[U] if len(U) else np.zeros((0, 3), dtype=np.int64)
    nondeg = (c3[:, 0] != c3[:, 1]) & (c3[:, 0] != c3[:, 2]) & (c3[:, 1] != c3[:, 2])
    c3n, idxn = c3[nondeg], uidx[nondeg]
    r = np.argmin(name[c3n], 1) if len(c3n) else np.zeros(0, dtype=np.int64)
    rot = np.stack([np.take_along_axis(c3n, ((r + j) % 3)[:, None], 1)[:, 0] for j in range(3)], 1) if len(c3n) else c3n
    _, first = np.unique(name[rot], axis=0, return_index=True) if len(rot) else (None, np.zeros(0, dtype=np.int64))
    first = np.sort(first)                                      # np.unique returns the first occurrence: the smallest old index
    K, src = rot[first], idxn[first]
    # 7 output
    cused = np.zeros(nc, dtype=bool)
    cused[K.reshape(-1)] = True
    outc = np.flatnonzero(cused)
    outc = outc[np.argsort(name[outc])]
    cnew = np.full(nc, -1, dtype=np.int64)
    cnew[outc] = np.arange(len(outc))
    out_tri = cnew[K].astype(np.int32).reshape(-1, 3)
    out_xyz = o + (Q[outc].astype(np.float64) / 65536.0) * cell
    out_rgba = (col[outc] << (8 * np.arange(4))).sum(1).astype(np.uint32)
    out_info = np.stack([name[outc], clev[outc], cn[outc], np.zeros(len(outc), dtype=np.int64)], 1).astype(np.int32)
    mo = _tri_m(Q[K[:, 0]], Q[K[:, 1]], Q[K[:, 2]], 32767.0) if len(K) else np.zeros((0, 3), dtype=np.int64)
    sn = np.zeros((nc, 3), dtype=np.int64)
    for j in range(3):
        np.add.at(sn, K[:, j], mo)
    x = sn[outc].astype(np.float64)
    L2 = np.sqrt((x[:, 0] * x[:, 0] + x[:, 1] * x[:, 1]) + x[:, 2] * x[:, 2])
    out_normal = np.where((L2 != 0)[:, None], x / np.where(L2 != 0, L2, 1.0)[:, None], 0.0).astype(np.float32)
    msrc = np.zeros((nt, 3), dtype=np.int64)
    msrc[uidx] = m
    flipped = int(((mo * msrc[src]).sum(1) < 0).sum())
    vmap = np.full(nv, -1, dtype=np.int64)
    vmap[mem] = np.where(cused[cid], cnew[cid], -2)
    level = np.where(member, lev, -1)
    kept_tri = np.zeros(nt, dtype=bool)
    kept_tri[src] = True
    report = np.array([nv, nt, used.sum(), nc, len(c3n) - len(K), len(outc), len(K), flipped], dtype=np.int32)
    return dict(xyz=out_xyz.reshape(-1, 3), normal=out_normal.reshape(-1, 3), rgba8=out_rgba.reshape(-1), info=out_info.reshape(-1, 4),
                tri=out_tri, vertex_map=vmap.astype(np.int32), level=level.astype(np.int32), report=report, q=q, Q=Q[outc], kept_tri=kept_tri,
                src_tri=src)


# ---- the restatement: one loop per triangle and vertex, Python ints and floats, dicts for the tables ----------------------------

_wrap = C._wrap


def _m_loop(qa, qb, qc, scale):
    e1 = [float(_wrap(qb[i] - qa[i])) for i in range(3)]
    e2 = [float(_wrap(qc[i] - qa[i])) for i in range(3)]
    n = [e1[1] * e2[2] - e1[2] * e2[1], e1[2] * e2[0] - e1[0] * e2[2], e1[0] * e2[1] - e1[1] * e2[0]]
    try:
        L = math.sqrt((n[0] * n[0] + n[1] * n[1]) + n[2] * n[2])
    except (OverflowError, ValueError):
        return [0, 0, 0]
    if L == 0.0 or not math.isfinite(L):
        return [0, 0, 0]
    return [math.floor((x / L) * scale + 0.5) for x in n]


def decimate_loop(xyz, normal, rgba8, info, tri, cell, origin, lmin=0, lmax=3, flat_q=1015, counts=None):
    """The same rule one vertex and one triangle at a time -> the same dict as decimate (without q, Q, kept_tri, src_tri)"""
    xyz, normal, rgba8, info, tri, nv, nt = C._prep(xyz, normal, rgba8, info, tri, counts)
    org0 = [float(x) for x in origin]
    cell, lmin, lmax, flat_q = float(cell), int(lmin), int(lmax), int(flat_q)
    q, valid = [], []
    for v in range(nv):
        ok, qv = True, [0, 0, 0]
        for a in range(3):
            X = float(xyz[v, a])
            t = (X - org0[a]) / cell if math.isfinite(X) else math.nan
            if not (-LIM <= t < LIM):
                ok = False
                continue
            qv[a] = min(math.floor(t * 65536.0 + 0.5), Q_MAX)
        valid.append(ok)
        q.append(qv if ok else [0, 0, 0])
    used, tm, member = [], {}, set()
    for k in range(nt):
        a, b, c = (int(x) for x in tri[k])
        if not (all(0 <= x < nv for x in (a, b, c)) and a != b and a != c and b != c and valid[a] and valid[b] and valid[c]):
            continue
        used.append(k)
        tm[k] = _m_loop(q[a], q[b], q[c], 1024.0)
        member.update((a, b, c))

    def block(v, l):
        return tuple(x >> (16 + l) for x in q[v])
    flat = {}
    for l in range(lmin + 1, lmax + 1):
        tab = {}
        for k in used:
            for v in tri[k]:
                e = tab.setdefault(block(int(v), l), [0, 0, 0, 0])
                for i in range(3):
                    e[i] = _wrap(e[i] + tm[k][i])
                e[3] += 1
        for key, e in tab.items():
            S2 = _wrap(_wrap(_wrap(e[0] * e[0]) + _wrap(e[1] * e[1])) + _wrap(e[2] * e[2]))
            flat[(l,) + key] = float(S2) >= float(flat_q * flat_q) * (float(e[3]) * float(e[3]))
    level, clusters = {}, {}
    for v in sorted(member):
        L = lmin
        while L < lmax and flat[(L + 1,) + block(v, L + 1)]:
            L += 1
        level[v] = L
        clusters.setdefault((L,) + block(v, L), []).append(v)
    cname = {key: mem[0] for key, mem in clusters.items()}      # members in ascending order: the first is the smallest
    vkey = {v: key for key, mem in clusters.items() for v in mem}
    cQ, ccol = {}, {}
    for key, mem in clusters.items():
        L, n = key[0], len(mem)
        Q = []
        for a in range(3):
            o_a = key[1 + a] << (16 + L)
            s = sum(q[v][a] - o_a for v in mem)
            Q.append(o_a + (2 * s + n) // (2 * n))
        cQ[key] = Q
        ccol[key] = sum((((2 * sum((int(rgba8[v]) >> (8 * j)) & 0xFF for v in mem) + n) // (2 * n)) << (8 * j)) for j in range(4))
    seen, kept, nondeg = set(), [], 0
    for k in used:
        keys = [vkey[int(v)] for v in tri[k]]
        if len(set(keys)) < 3:
            continue
        nondeg += 1
        names = [cname[x] for x in keys]
        r = names.index(min(names))
        rot = tuple(keys[(r + j) % 3] for j in range(3))
        if rot in seen:
            continue
        seen.add(rot)
        kept.append((k, rot))
    outk = sorted({key for _, rot in kept for key in rot}, key=lambda key: cname[key])
    cnew = {key: i for i, key in enumerate(outk)}
    sums = {key: [0, 0, 0] for key in outk}
    flipped = 0
    for k, rot in kept:
        mo = _m_loop(cQ[rot[0]], cQ[rot[1]], cQ[rot[2]], 32767.0)
        if sum(mo[i] * tm[k][i] for i in range(3)) < 0:
            flipped += 1
        for key in rot:
            sums[key] = [sums[key][i] + mo[i] for i in range(3)]
    oxyz, onrm, orgb, oinf = [], [], [], []
    for key in outk:
        oxyz.append([org0[a] + (float(cQ[key][a]) / 65536.0) * cell for a in range(3)])
        x = [float(y) for y in sums[key]]
        L = math.sqrt((x[0] * x[0] + x[1] * x[1]) + x[2] * x[2])
        onrm.append([np.float32(y / L) for y in x] if L != 0.0 else [np.float32(0)] * 3)
        orgb.append(ccol[key])
        oinf.append([cname[key], key[0], len(clusters[key]), 0])
    A = len(outk)
    vmap = [(cnew.get(vkey[v], -2) if v in member else -1) for v in range(nv)]
    lv = [level.get(v, -1) for v in range(nv)]
    report = np.array([nv, nt, len(used), len(clusters), nondeg - len(kept), A, len(kept), flipped], dtype=np.int32)
    return dict(xyz=np.array(oxyz, dtype=np.float64).reshape(A, 3), normal=np.array(onrm, dtype=np.float32).reshape(A, 3),
                rgba8=np.array(orgb, dtype=np.uint32).reshape(A), info=np.array(oinf, dtype=np.int32).reshape(A, 4),
                tri=np.array([[cnew[key] for key in rot] for _, rot in kept], dtype=np.int32).reshape(-1, 3),
                vertex_map=np.array(vmap, dtype=np.int32).reshape(nv), level=np.array(lv, dtype=np.int32).reshape(nv), report=report)


def assert_same(a, b, keys=INT_KEYS + FLOAT_KEYS):
    for k in keys:
        x, y = np.asarray(a[k]), np.asarray(b[k])
        assert x.shape == y.shape, (k, x.shape, y.shape)
        if k in FLOAT_KEYS:
            assert bits(x.astype(y.dtype)) == bits(y), (k, np.argwhere(x != y)[:5])
        else:
            assert (x.astype(np.int64) == y.astype(np.int64)).all(), (k, np.argwhere(x != y)[:5])


# ---- k_meshdecimate.hip's constants, keys and hashes ------------------------------------------------------------------------------

def kernel_constants(csrc):
    text = open(os.path.join(csrc, "k_meshdecimate.hip")).read()
    c = {k: int(v) for k, v in re.findall(r"constexpr int (MDC_NT|MDC_GRID_MAX|MDC_LG_SLOTS|MDC_SLOTS|MDC_FLUSH_AT|MDC_LG_TMIN) = (\d+)", text)}
    c.update({k: int(v, 16) for k, v in re.findall(r"constexpr unsigned long long (MDC_HASH_MUL|MDC_TRI_MUL1|MDC_TRI_MUL2) = 0x([0-9A-Fa-f]+)ull", text)})
    # the keys, the hashes and the probe restated below
    for needle in ("(key * MDC_HASH_MUL) >> (64 - lg)", "h = (h + 1) & mask", "(unsigned)c0 * MDC_HASH_MUL + (unsigned long long)(unsigned)c1 * MDC_TRI_MUL1",
                   "(unsigned long long)(unsigned)c2 * MDC_TRI_MUL2", "1ull << 63 | (unsigned long long)l << 60 | (unsigned long long)(b0 + 524288) << 40",
                   "if (l == 0) return cld_key_of((int)b0, (int)b1, (int)b2);", "(1ll << lg) < 2ll * (long long)n"):
        assert needle in text, needle
    return c


def table_lg(n, c):
    """lg of the table the device uses for n vertices or triangles"""
    lg = c["MDC_LG_TMIN"]
    while lg < 30 and (1 << lg) < 2 * n:
        lg += 1
    return lg


def block_key(l, b):
    """mdc_key: level 0 is the cloud's key of the cell; above, 20 bits a coordinate, the level in bits 60 .. 62, bit 63 set"""
    if l == 0:
        return (b[0] + 2**20) << 42 | (b[1] + 2**20) << 21 | (b[2] + 2**20)
    return 1 << 63 | l << 60 | (b[0] + 2**19) << 40 | (b[1] + 2**19) << 20 | (b[2] + 2**19)


def table_hash(key, lg, c):
    return ((key * c["MDC_HASH_MUL"]) % 2**64) >> (64 - lg)


def triple_hash(c0, c1, c2, lg, c):
    return ((c0 * c["MDC_HASH_MUL"] + c1 * c["MDC_TRI_MUL1"] + c2 * c["MDC_TRI_MUL2"]) % 2**64) >> (64 - lg)


def cells_hashing_to(l, lg, slots, count, c, span=400):
    """`count` blocks (b0, b1, 0) of level l with 0 <= b0, b1 < span whose keys hash into `slots` of a table of 1 << lg entries"""
    out = []
    for b0 in range(span):
        for b1 in range(span):
            if table_hash(block_key(l, (b0, b1, 0)), lg, c) in slots:
                out.append((b0, b1, 0))
                if len(out) == count:
                    return out
    raise AssertionError("not enough blocks")


# ---- figures ----------------------------------------------------------------------------------------------------------------------

def plane_distance(m):
    """the area-weighted mean distance of the two-plane scenes' surface to the nearer plane (z = 3, z = 4), each triangle sampled
    at its vertices, edge midpoints and centroid; and the triangle count"""
    X, T = m["xyz"], m["tri"]
    if not len(T):
        return 0.0
    a, b, c = X[T[:, 0]], X[T[:, 1]], X[T[:, 2]]
    area = 0.5 * np.linalg.norm(np.cross(b - a, c - a), axis=1)
    pts = np.stack([a, b, c, (a + b) / 2, (b + c) / 2, (c + a) / 2, (a + b + c) / 3], 1)
    d = np.minimum(np.abs(pts[..., 2] - 3.0), np.abs(pts[..., 2] - 4.0)).mean(1)
    return float((d * area).sum() / area.sum())


@functools.lru_cache(maxsize=None)
def cleaned_truth(case):
    """the truth mesh of mesh_clean_ref after the clean stage (min_tris 100, 5 iterations) -> mesh dict"""
    t, m = C.truth_mesh(case)
    return C.clean(*(m[k] for k in OUT_KEYS), mesh_ref.CELL, mesh_ref.TRUTH_ORIGIN, min_tris=100, iters=5, lam=C.LAM, mu=C.MU)


def extent(m):
    return (m["xyz"].max(0) - m["xyz"].min(0)) if len(m["xyz"]) else np.zeros(3)
