"""The yardstick of the mesh's clean stage (include/pgx.h: pgx_mesh_clean_dev), operation by operation in the header's order, in
two forms that share no code beyond the input layout (_prep): `clean`, vectorised numpy (components by np.minimum.at with pointer
jumping to a fixpoint, np.add.at on int64 for every sum), and `clean_loop`, one loop per triangle and vertex in Python ints (wrapped
to int64 by hand) and floats with a dict union-find.  Python floats and numpy float64 do not contract a b + c, which is what the
library's -ffp-contract=off build does.  The constants of k_meshclean.hip that the GPU tests size their cases by are read from the
source (kernel_constants).  The shapes and scenes that the CPU and the GPU tests share stand at the end.  A plain helper module."""
import functools
import math
import os
import re

import numpy as np

import cloud_ref
import mesh_ref

bits = cloud_ref.bits
OUT_KEYS = ("xyz", "normal", "rgba8", "info", "tri")
INT_KEYS = ("rgba8", "info", "tri", "vertex_map", "comp", "report")
FLOAT_KEYS = ("xyz", "normal")
LIM = float(2**20)
STEP_MAX = float(2**62)


def _prep(xyz, normal, rgba8, info, tri, counts):
    """the input layout: arrays of the ABI's types, and nv, nt by the header's clamp of counts = (vertices, triangles) or None"""
    xyz = np.asarray(xyz, dtype=np.float64).reshape(-1, 3)
    normal = np.asarray(normal, dtype=np.float32).reshape(-1, 3)
    rgba8 = np.asarray(rgba8).astype(np.uint32).reshape(-1)
    info = np.asarray(info, dtype=np.int32).reshape(-1, 4)
    tri = np.asarray(tri, dtype=np.int32).reshape(-1, 3)
    nv, nt = len(xyz), len(tri)
    if counts is not None:
        nv, nt = min(max(int(counts[0]), 0), nv), min(max(int(counts[1]), 0), nt)
    return xyz, normal, rgba8, info, tri, nv, nt


# ---- the vectorised form ----------------------------------------------------------------------------------------------------

def clean(xyz, normal, rgba8, info, tri, cell, origin, min_tris=1, min_frac_pm=0, iters=0, lam=0.5, mu=-0.53, counts=None):
    """pgx_mesh_clean_dev without the capacities -> dict: the outputs xyz, normal, rgba8, info, tri; vertex_map [nv], comp [nv],
    report [8]; q [nv][3] int64, the final fixed-point positions (of the kept vertices), and kept_tri [nt] bool"""
    xyz, normal, rgba8, info, tri, nv, nt = _prep(xyz, normal, rgba8, info, tri, counts)
    o = np.asarray(origin, dtype=np.float64)
    cell = float(cell)
    X, T = xyz[:nv], tri[:nt].astype(np.int64)
    # 1 valid / used
    with np.errstate(all="ignore"):
        t = (X - o) / cell
        valid = np.isfinite(X).all(1) & ((t >= -LIM) & (t < LIM)).all(1)
        q = np.where(valid[:, None], np.floor(np.where(valid[:, None], t, 0.0) * 65536.0 + 0.5), 0.0).astype(np.int64)
    inr = ((T >= 0) & (T < nv)).all(1)
    Tc = np.where(inr[:, None], T, 0)
    used = inr & (Tc[:, 0] != Tc[:, 1]) & (Tc[:, 0] != Tc[:, 2]) & (Tc[:, 1] != Tc[:, 2])
    if nv:
        used &= valid[Tc].all(1)
    U = T[used]
    # 2 components: every vertex takes the smallest label among the vertices and labels of its triangles, then jumps
    lab = np.arange(nv, dtype=np.int64)
    while len(U):
        m = np.repeat(lab[U].min(1), 3)
        new = lab.copy()
        np.minimum.at(new, U.reshape(-1), m)
        np.minimum.at(new, lab[U].reshape(-1), m)
        new = new[new]
        if (new == lab).all():
            break
        lab = new
    deg = np.bincount(U.reshape(-1), minlength=nv).astype(np.int64)
    inused = deg > 0
    cnt = np.bincount(lab[U[:, 0]], minlength=nv).astype(np.int64)
    big = int(cnt.max()) if nv else 0
    names = np.flatnonzero(inused & (lab == np.arange(nv)))
    keptc = (cnt >= int(min_tris)) & (1000 * cnt >= int(min_frac_pm) * big)
    vkept = inused & keptc[lab]
    tkept = used.copy()
    tkept[used] = keptc[lab[U[:, 0]]]
    vmap = np.where(vkept, np.cumsum(vkept) - 1, np.where(inused, -2, -1)).astype(np.int32)
    comp = np.where(inused, lab, -1).astype(np.int32)
    K = T[tkept]
    kv = np.flatnonzero(vkept)
    # 3 smoothing
    out_xyz, out_normal = X[kv].copy(), normal[:nv][kv].copy()
    if iters > 0:
        d = np.bincount(K.reshape(-1), minlength=nv).astype(np.int64)
        den = (2 * d).astype(np.float64)
        for _ in range(int(iters)):
            for f in ((float(lam),) if float(mu) == 0.0 else (float(lam), float(mu))):
                D = np.zeros((nv, 3), dtype=np.int64)
                for j in range(3):
                    v, o1, o2 = K[:, j], K[:, (j + 1) % 3], K[:, (j + 2) % 3]
                    np.add.at(D, v, (q[o1] - q[v]) + (q[o2] - q[v]))
                with np.errstate(all="ignore"):
                    r = np.floor((f * D.astype(np.float64)) / den[:, None] + 0.5)
                r = np.clip(np.where(vkept[:, None], r, 0.0), -STEP_MAX, STEP_MAX)
                q = q + r.astype(np.int64)
        # 4 normals
        with np.errstate(all="ignore"):
            e1 = (q[K[:, 1]] - q[K[:, 0]]).astype(np.float64)
            e2 = (q[K[:, 2]] - q[K[:, 0]]).astype(np.float64)
            n = np.stack([e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1], e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2],
                          e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]], 1)
            L = np.sqrt((n[:, 0] * n[:, 0] + n[:, 1] * n[:, 1]) + n[:, 2] * n[:, 2])
            ok = (L != 0) & np.isfinite(L)
            m = np.where(ok[:, None], np.floor((np.where(ok[:, None], n, 0.0) / np.where(ok, L, 1.0)[:, None]) * 32767.0 + 0.5), 0.0).astype(np.int64)
        s = np.zeros((nv, 3), dtype=np.int64)
        for j in range(3):
            np.add.at(s, K[:, j], m)
        x = s[kv].astype(np.float64)
        L2 = np.sqrt((x[:, 0] * x[:, 0] + x[:, 1] * x[:, 1]) + x[:, 2] * x[:, 2])
        out_normal = np.where((L2 != 0)[:, None], x / np.where(L2 != 0, L2, 1.0)[:, None], 0.0).astype(np.float32)
        out_xyz = o + (q[kv].astype(np.float64) / 65536.0) * cell
    out_tri = vmap[K].astype(np.int32).reshape(-1, 3)
    report = np.array([nv, nt, used.sum(), len(names), keptc[names].sum(), len(kv), len(K), big], dtype=np.int32)
    return dict(xyz=out_xyz.reshape(-1, 3), normal=out_normal.reshape(-1, 3), rgba8=rgba8[:nv][kv], info=info[:nv][kv].reshape(-1, 4),
                tri=out_tri, vertex_map=vmap, comp=comp, report=report, q=q, kept_tri=tkept)


# ---- the restatement: one loop per triangle and vertex, Python ints and floats, a dict union-find ---------------------------------

def _wrap(x):
    """a Python int as the int64 it is in two's complement"""
    return ((x + 2**63) % 2**64) - 2**63


def clean_loop(xyz, normal, rgba8, info, tri, cell, origin, min_tris=1, min_frac_pm=0, iters=0, lam=0.5, mu=-0.53, counts=None):
    """The same rule one vertex and one triangle at a time -> the same dict as clean (without q, kept_tri)"""
    xyz, normal, rgba8, info, tri, nv, nt = _prep(xyz, normal, rgba8, info, tri, counts)
    org = [float(x) for x in origin]
    cell = float(cell)
    q, valid = [], []
    for v in range(nv):
        ok, qv = True, [0, 0, 0]
        for a in range(3):
            X = float(xyz[v, a])
            if not math.isfinite(X):
                ok = False
                continue
            t = (X - org[a]) / cell
            if not (-LIM <= t < LIM):
                ok = False
                continue
            qv[a] = math.floor(t * 65536.0 + 0.5)
        valid.append(ok)
        q.append(qv if ok else [0, 0, 0])
    parent = {}

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x
    used = []
    for k in range(nt):
        a, b, c = (int(x) for x in tri[k])
        u = all(0 <= x < nv for x in (a, b, c)) and a != b and a != c and b != c and valid[a] and valid[b] and valid[c]
        used.append(u)
        if not u:
            continue
        for x in (a, b, c):
            parent.setdefault(x, x)
        for x in (b, c):
            ra, rx = find(a), find(x)
            if ra != rx:
                parent[max(ra, rx)] = min(ra, rx)           # the smaller index on top: the root is the component's name
    cnt = {}
    for k in range(nt):
        if used[k]:
            r = find(int(tri[k, 0]))
            cnt[r] = cnt.get(r, 0) + 1
    big = max(cnt.values()) if cnt else 0
    keptc = {r: c >= int(min_tris) and 1000 * c >= int(min_frac_pm) * big for r, c in cnt.items()}
    vmap, comp, kv = [], [], []
    for v in range(nv):
        if v not in parent:
            vmap.append(-1)
            comp.append(-1)
            continue
        r = find(v)
        comp.append(r)
        if keptc[r]:
            vmap.append(len(kv))
            kv.append(v)
        else:
            vmap.append(-2)
    K = [k for k in range(nt) if used[k] and keptc[find(int(tri[k, 0]))]]
    oxyz = [[float(x) for x in xyz[v]] for v in kv]
    onrm = [[np.float32(x) for x in normal[v]] for v in kv]
    if iters > 0:
        inc = {v: [] for v in kv}
        for k in K:
            for x in tri[k]:
                inc[int(x)].append(k)
        for _ in range(int(iters)):
            for f in ((float(lam),) if float(mu) == 0.0 else (float(lam), float(mu))):
                nq = [row[:] for row in q]
                for v in kv:
                    d = len(inc[v])
                    for a in range(3):
                        D = 0
                        for k in inc[v]:
                            o1, o2 = [int(x) for x in tri[k] if int(x) != v]
                            D = _wrap(D + _wrap(_wrap(q[o1][a] - q[v][a]) + _wrap(q[o2][a] - q[v][a])))
                        r = math.floor((f * float(D)) / float(2 * d) + 0.5)
                        r = max(-2**62, min(2**62, r))
                        nq[v][a] = _wrap(q[v][a] + r)
                q = nq
        m = {}
        for k in K:
            a, b, c = (int(x) for x in tri[k])
            e1 = [float(_wrap(q[b][i] - q[a][i])) for i in range(3)]
            e2 = [float(_wrap(q[c][i] - q[a][i])) for i in range(3)]
            n = [e1[1] * e2[2] - e1[2] * e2[1], e1[2] * e2[0] - e1[0] * e2[2], e1[0] * e2[1] - e1[1] * e2[0]]
            L = math.sqrt((n[0] * n[0] + n[1] * n[1]) + n[2] * n[2])
            m[k] = None if L == 0.0 or not math.isfinite(L) else [math.floor((x / L) * 32767.0 + 0.5) for x in n]
        oxyz, onrm = [], []
        for v in kv:
            s = [0, 0, 0]
            for k in inc[v]:
                if m[k] is not None:
                    s = [s[i] + m[k][i] for i in range(3)]
            x = [float(y) for y in s]
            L = math.sqrt((x[0] * x[0] + x[1] * x[1]) + x[2] * x[2])
            onrm.append([np.float32(y / L) for y in x] if L != 0.0 else [np.float32(0)] * 3)
            oxyz.append([org[a] + (float(q[v][a]) / 65536.0) * cell for a in range(3)])
    otri = [[vmap[int(x)] for x in tri[k]] for k in K]
    A = len(kv)
    report = np.array([nv, nt, sum(used), len(cnt), sum(keptc.values()), A, len(K), big], dtype=np.int32)
    return dict(xyz=np.array(oxyz, dtype=np.float64).reshape(A, 3), normal=np.array(onrm, dtype=np.float32).reshape(A, 3),
                rgba8=rgba8[kv].reshape(A), info=info[kv].reshape(A, 4), tri=np.array(otri, dtype=np.int32).reshape(-1, 3),
                vertex_map=np.array(vmap, dtype=np.int32).reshape(nv), comp=np.array(comp, dtype=np.int32).reshape(nv), report=report)


def assert_same(a, b, keys=INT_KEYS + FLOAT_KEYS):
    for k in keys:
        x, y = np.asarray(a[k]), np.asarray(b[k])
        assert x.shape == y.shape, (k, x.shape, y.shape)
        if k in FLOAT_KEYS:
            assert bits(x.astype(y.dtype)) == bits(y), (k, np.argwhere(x != y)[:5])
        else:
            assert (x.astype(np.int64) == y.astype(np.int64)).all(), (k, np.argwhere(x != y)[:5])


# ---- k_meshclean.hip's constants --------------------------------------------------------------------------------------------------

def kernel_constants(csrc):
    text = open(os.path.join(csrc, "k_meshclean.hip")).read()
    return {k: int(v) for k, v in re.findall(r"constexpr int (MCL_NT|MCL_GRID_MAX|MCL_UNION_GRID|MCL_SLOTS|MCL_LONG_ROW) = (\d+)", text)}


# ---- shapes ---------------------------------------------------------------------------------------------------------------------

CELL, ORIGIN = 0.25, (-8.0, -8.0, -8.0)


def attrs(xyz, tri, seed=0):
    """a mesh dict of the ABI's arrays round positions and triangles: random normals, colours and info"""
    rng = np.random.default_rng(seed)
    xyz = np.asarray(xyz, dtype=np.float64).reshape(-1, 3)
    n = len(xyz)
    return dict(xyz=xyz, normal=rng.standard_normal((n, 3)).astype(np.float32), rgba8=rng.integers(0, 2**32, n, dtype=np.uint32),
                info=rng.integers(-2**31, 2**31, (n, 4)).astype(np.int32), tri=np.asarray(tri, dtype=np.int32).reshape(-1, 3))


def grid_plane(nx, ny, cell=CELL, origin=ORIGIN, z=3.0, jitter=0.0, seed=0):
    """an nx x ny lattice of vertices on multiples of `cell` at height z, every quad split along the same diagonal, wound to face
    -z; with jitter every coordinate moves by up to jitter * cell"""
    j, i = np.mgrid[0:ny, 0:nx]
    xyz = np.stack([origin[0] + (i + 8.0) * cell, origin[1] + (j + 8.0) * cell, np.full(i.shape, float(z))], -1).reshape(-1, 3)
    if jitter:
        xyz = xyz + np.random.default_rng(seed).uniform(-jitter * cell, jitter * cell, xyz.shape)
    v = (j * nx + i)[:-1, :-1].reshape(-1)
    tri = np.stack([np.stack([v, v + nx, v + nx + 1], 1), np.stack([v, v + nx + 1, v + 1], 1)], 1).reshape(-1, 3)
    return xyz, tri


def strip(n_tris, reverse=False, cell=CELL, origin=ORIGIN, seed=0):
    """a triangle strip of n_tris triangles over n_tris + 2 jittered vertices: one long chain; reverse numbers the vertices from
    the far end, so the component's name is the vertex the strip reaches last"""
    n = n_tris + 2
    k = np.arange(n)
    xyz = np.stack([origin[0] + (k // 2 + 4.0) * cell, origin[1] + (k % 2 + 4.0) * cell, np.full(n, 3.0)], -1)
    xyz = xyz + np.random.default_rng(seed).uniform(-0.2 * cell, 0.2 * cell, xyz.shape)
    t = np.arange(n_tris)
    tri = np.stack([t, np.where(t % 2 == 0, t + 1, t + 2), np.where(t % 2 == 0, t + 2, t + 1)], 1)
    if reverse:
        tri = (n - 1) - tri
    return xyz, tri


def fan(n_tris, cell=CELL, origin=ORIGIN):
    """vertex 0 in n_tris triangles round it (a cone: the hub stands off the rim's plane), and a last triangle that hangs on
    vertex 1: its two other vertices, the last two, have degree 1"""
    ang = 2.0 * np.pi * np.arange(n_tris) / n_tris
    rim = np.stack([origin[0] + 40.0 * cell + 8.0 * cell * np.cos(ang), origin[1] + 40.0 * cell + 8.0 * cell * np.sin(ang), np.full(n_tris, 3.0)], -1)
    hub = np.array([[origin[0] + 40.0 * cell, origin[1] + 40.0 * cell, 3.0 - 2.0 * cell]])
    tail = np.array([[origin[0] + 52.0 * cell, origin[1] + 40.0 * cell, 3.0], [origin[0] + 52.0 * cell, origin[1] + 42.0 * cell, 3.1]])
    k = np.arange(n_tris)
    tri = np.concatenate([np.stack([np.zeros(n_tris, dtype=np.int64), 1 + k, 1 + (k + 1) % n_tris], 1), [[1, n_tris + 1, n_tris + 2]]])
    return np.concatenate([hub, rim, tail]), tri


def twin_fans(n_a, n_b, cell=CELL, origin=ORIGIN):
    """two cones whose hubs are vertices 0 and 1, neighbours in one wave, with n_a and n_b triangles; their rims touch in no
    vertex: two components"""
    def rim(n, cx):
        ang = 2.0 * np.pi * np.arange(n) / n
        return np.stack([origin[0] + cx * cell + 8.0 * cell * np.cos(ang), origin[1] + 40.0 * cell + 8.0 * cell * np.sin(ang), np.full(n, 3.0)], -1)
    hubs = np.array([[origin[0] + 40.0 * cell, origin[1] + 40.0 * cell, 3.0 - 2.0 * cell], [origin[0] + 70.0 * cell, origin[1] + 40.0 * cell, 3.0 + 3.0 * cell]])
    ka, kb = np.arange(n_a), np.arange(n_b)
    tri = np.concatenate([np.stack([np.zeros(n_a, dtype=np.int64), 2 + ka, 2 + (ka + 1) % n_a], 1),
                          np.stack([np.ones(n_b, dtype=np.int64), 2 + n_a + kb, 2 + n_a + (kb + 1) % n_b], 1)])
    return np.concatenate([hubs, rim(n_a, 40.0), rim(n_b, 70.0)]), tri


def islands(sizes, cell=CELL, origin=ORIGIN, seed=0):
    """one small strip of sizes[i] triangles per entry, side by side: len(sizes) components"""
    xs, ts, at = [], [], 0
    for i, s in enumerate(sizes):
        x, t = strip(int(s), seed=seed + i)
        xs.append(x + np.array([0.0, (3.0 * (i % 1000)) * cell, (i // 1000) * cell]))
        ts.append(t + at)
        at += len(x)
    return np.concatenate(xs), np.concatenate(ts)


def singles(n, cell=CELL, origin=ORIGIN, seed=0):
    """n triangles of three vertices of their own: n components of one triangle"""
    k = np.arange(3 * n)
    xyz = np.stack([origin[0] + (k % 3000 + 4.0) * cell, origin[1] + (k // 3000 + 4.0) * cell, np.full(3 * n, 3.0)], -1)
    xyz = xyz + np.random.default_rng(seed).uniform(-0.3 * cell, 0.3 * cell, xyz.shape)
    return xyz, k.reshape(n, 3)


def messy(seed=3):
    """every kind of vertex and triangle the rule tells apart: NaN, infinite and out-of-range vertices (t at -2^20, just below
    2^20 and at 2^20), triangles with a repeated, a negative and a too-large index and with an invalid vertex, bare vertices, and
    components of 1, 2, 3, 5, 8 and 40 triangles"""
    xyz, tri = islands([1, 2, 3, 5, 8, 40, 3, 1], seed=seed)
    n = len(xyz)
    lo, hi = ORIGIN[0] - LIM * CELL, ORIGIN[0] + LIM * CELL
    extra = np.array([[np.nan, 0, 0], [0, np.inf, 0], [0, 0, -np.inf], [lo, 0, 0], [np.nextafter(hi, -np.inf), 0, 0], [hi, 0, 0],
                      [0, np.nextafter(lo, -np.inf), 0], [0, 0, hi], [1.0, 1.0, 1.0], [1.5, 1.0, 1.0], [1.0, 1.5, 1.0],
                      [2.0, 2.0, 2.0], [2.5, 2.0, 2.0]])       # the last two are bare: valid and in no triangle
    e = n + np.arange(len(extra))
    bad = [[0, 0, 1], [1, 2, 1], [3, 4, 4], [-1, 0, 1], [0, 1, n + len(extra)], [0, 1, 2**31 - 1], [0, 1, e[0]], [e[1], 1, 2], [2, e[2], 3],
           [0, 1, e[5]], [0, e[6], 1], [e[7], 0, 1],
           [e[3], e[4], e[8]], [e[8], e[9], e[10]]]                # the last two are used: lo and just below hi are valid
    return np.concatenate([xyz, extra]), np.concatenate([tri, np.array(bad, dtype=np.int64)])


# ---- scenes ---------------------------------------------------------------------------------------------------------------------

LAM, MU = 0.5, -0.53


@functools.lru_cache(maxsize=None)
def truth_mesh(case):
    """mesh_ref's mesh of a truth case on the truth grid -> (inputs, mesh)"""
    t = mesh_ref.truth_inputs(case)
    m = mesh_ref.mesh(t["xyz"], t["src"], t["depth"], t["views"], 5, t["P"], mesh_ref.CELL, mesh_ref.TRUTH_ORIGIN, band=mesh_ref.TRUTH_BAND,
                      trunc_cells=mesh_ref.TRUTH_TRUNC, agree=t["agree"], min_agree=t["min_agree"])
    return t, m


FLOATER_AT = ((-0.8, 0.6, 2.2), (0.9, -0.7, 2.5), (0.2, 0.9, 5.2))


@functools.lru_cache(maxsize=None)
def planted_case():
    """scene_rotated() at its true depths with extra points in the list, off the planes: each seeds voxels of its own.  Where the
    maps see free space the TSDF of those voxels is positive and has no surface; a blob appears where maps are wrong, as the
    floaters of a real run do: every map that sees a planted point gets 3 x 3 pixels of the point's depth at its projection.  Two
    of the three points grow a closed blob of a few triangles -> (inputs, mesh)"""
    t = dict(mesh_ref.truth_inputs("rotated-true"))
    depth = t["depth"].copy()
    P = np.reshape(t["P"], (-1, 3, 4))
    H, W = depth.shape[1:]
    pts = []
    for X in FLOATER_AT:
        for r in range(depth.shape[0]):
            f = int(t["views"][r][0])
            qh = P[f] @ np.array([X[0], X[1], X[2], 1.0])
            u, v = int(qh[0] / qh[2] + 0.5), int(qh[1] / qh[2] + 0.5)
            if qh[2] > 0 and 1 <= u < W - 1 and 1 <= v < H - 1:
                depth[r, v - 1:v + 2, u - 1:u + 2] = qh[2] / np.linalg.norm(P[f][2, :3])
        pts.append(X)
    t["depth"] = depth
    t["xyz"] = np.concatenate([t["xyz"], np.array(pts)])
    t["src"] = np.concatenate([t["src"], np.tile([[0, 0]], (len(pts), 1))]).astype(np.int32)
    m = mesh_ref.mesh(t["xyz"], t["src"], t["depth"], t["views"], 5, t["P"], mesh_ref.CELL, mesh_ref.TRUTH_ORIGIN, band=mesh_ref.TRUTH_BAND,
                      trunc_cells=mesh_ref.TRUTH_TRUNC)
    return t, m


def figures(m, cell):
    """the truth figures of a (cleaned) mesh of the two-plane scenes: mesh_ref.truth_figures and the bounding box's extent"""
    f = mesh_ref.truth_figures(m, cell, mesh_ref.TRUTH_TRUNC * cell)
    f["extent"] = (m["xyz"].max(0) - m["xyz"].min(0)) if len(m["xyz"]) else np.zeros(3)
    return f
