"""The yardstick of the mesh (include/pgx.h: pgx_mesh_dev), operation by operation in the header's order, in two forms that share
no line of rules 2 to 5: `mesh`, vectorised numpy (np.unique on the keys, np.add.at on int64, sorted-key lookups), and `mesh_loop`,
one loop per voxel, cube and edge in Python ints, floats and a dict, with its own projection.  Rule 1, the used test and the cell
of a point, is cloud_ref's in both (the library shares it the same way: pgx_cloudkey.h).  Python floats and numpy float64 do not
contract a b + c, which is what the library's -ffp-contract=off build does.  The constants of k_mesh.hip that the GPU tests size
their cases by are read from the source (kernel_constants), and its hash is restated (table_hash).  A plain helper module."""
import math
import os
import re

import numpy as np

import cloud_ref
import depth_ref

GB = cloud_ref.GB
MARGIN = 4
OUT_KEYS = ("xyz", "normal", "rgba8", "info", "tri")
INT_KEYS = ("vox", "ord", "w", "st", "nc", "sc", "rgba8", "info", "tri", "report")
FLOAT_KEYS = ("xyz", "normal")
bits = cloud_ref.bits


def used_cells(xyz, src, depth, views, n_frames, P, cell, origin, count):
    """rule 1: cloud_ref's used test and g, and the margin of MARGIN cells -> n, used [n] bool, g [n][3] int64"""
    m = cloud_ref.merge(xyz, src, depth, views, n_frames, P, cell, origin, count=count)
    g = m["g"]
    used = m["used"] & ((g >= -GB + MARGIN) & (g < GB - MARGIN)).all(1)
    return int(m["report"][0]), used, g


def pack(c):
    c = np.asarray(c, dtype=np.int64)
    return (c[..., 0] + GB) << 42 | (c[..., 1] + GB) << 21 | (c[..., 2] + GB)


def unpack(keys):
    keys = np.asarray(keys, dtype=np.int64)
    return np.stack([(keys >> 42) & 0x1FFFFF, (keys >> 21) & 0x1FFFFF, keys & 0x1FFFFF], -1) - GB


def _prep(xyz, src, depth, views, P, agree, rgba8):
    xyz = np.asarray(xyz, dtype=np.float64).reshape(-1, 3)
    src = np.asarray(src, dtype=np.int64).reshape(-1, 2)
    depth = np.asarray(depth, dtype=np.float64)
    R = depth.shape[0]
    views = np.asarray(views, dtype=np.int64).reshape(R, -1)
    P = np.asarray(P, dtype=np.float64).reshape(-1, 12)
    agree = None if agree is None else np.asarray(agree, dtype=np.int64).reshape(depth.shape)
    rgba8 = None if rgba8 is None else np.asarray(rgba8).astype(np.uint32).reshape((-1,) + depth.shape[1:])
    return xyz, src, depth, views, P, agree, rgba8


# ---- the vectorised form ----------------------------------------------------------------------------------------------------

def mesh(xyz, src, depth, views, n_frames, P, cell, origin, band=1, trunc_cells=3, min_weight=1, agree=None, min_agree=0, rgba8=None,
         frame_ids=None, count=None):
    """pgx_mesh_dev without the capacities -> dict: per voxel in ascending ord vox [V] (keys), ord, w, st, nc, sc [V][3]; the
    outputs xyz, normal, rgba8, info, tri; report [8]"""
    xyz, src, depth, views, P, agree, rgba8 = _prep(xyz, src, depth, views, P, agree, rgba8)
    R, H, W = depth.shape
    B = int(band)
    n, used, g = used_cells(xyz, src, depth, views, n_frames, P, cell, origin, count)
    o = np.asarray(origin, dtype=np.float64)
    trunc = float(trunc_cells) * float(cell)
    # 2 voxels: the first point of each occupied cell dilates
    ui = np.flatnonzero(used)
    ckeys, cfirst = np.unique(pack(g[ui]), return_index=True)
    cfirst = ui[cfirst]                                        # ui ascends: the first occurrence is the smallest i
    nb = np.arange((2 * B) ** 3, dtype=np.int64)
    d = np.stack([nb % (2 * B), nb // (2 * B) % (2 * B), nb // (4 * B * B)], -1)
    nodes = (unpack(ckeys)[:, None, :] - (B - 1) + d[None, :, :]).reshape(-1, 3)
    nord = (256 * cfirst[:, None] + nb[None, :]).reshape(-1)
    nkeys = pack(nodes)
    vkeys, inv = np.unique(nkeys, return_inverse=True)
    vord = np.full(len(vkeys), np.iinfo(np.int64).max, dtype=np.int64)
    np.minimum.at(vord, inv.reshape(-1), nord)
    by_ord = np.argsort(vord)
    vkeys, vord = vkeys[by_ord], vord[by_ord]                  # voxels in ascending ord
    V = len(vkeys)
    c = unpack(vkeys).reshape(V, 3)
    # 3 TSDF
    X = [o[a] + c[:, a].astype(np.float64) * cell for a in range(3)]
    w, st, nc = (np.zeros(V, dtype=np.int64) for _ in range(3))
    sc = np.zeros((V, 3), dtype=np.int64)
    F = 0 if rgba8 is None else len(rgba8)
    for r in range(R):
        f = int(views[r, 0])
        if not 0 <= f < n_frames:
            continue
        cam = depth_ref.camera(P[f])
        if not cam[0]:
            continue
        Pr = P[f].reshape(3, 4)
        with np.errstate(all="ignore"):
            q = [((Pr[i, 0] * X[0] + Pr[i, 1] * X[1]) + Pr[i, 2] * X[2]) + Pr[i, 3] for i in range(3)]
            ok, iu, iv = depth_ref.pixel(q[0], q[1], q[2], W, H)
            z = depth[r][iv, iu]
            ok = ok & np.isfinite(z)
            if agree is not None:
                ok = ok & (agree[r][iv, iu] >= min_agree)
            dd = (cam[3] * q[2]) / cam[4]
            s = z - dd
            cnt = ok & (s >= -trunc)
            t = np.where(s > trunc, trunc, s)
            tq = np.floor((np.where(cnt, t, 0.0) / trunc) * 32767.0 + 0.5).astype(np.int64)
        w += cnt
        st += np.where(cnt, tq, 0)
        sl = depth_ref.slot_of(frame_ids, F, n_frames, f) if rgba8 is not None else -1
        if sl >= 0:
            cc = cnt & (s <= trunc)
            col = rgba8[sl][iv, iu].astype(np.int64)
            nc += cc
            for k in range(3):
                sc[:, k] += np.where(cc, (col >> (8 * k)) & 255, 0)
    valid = w >= min_weight
    inside = valid & (st < 0)
    with np.errstate(all="ignore"):
        phi = st.astype(np.float64) / w.astype(np.float64)
    # lookups by sorted key
    by_key = np.argsort(vkeys)
    skeys = vkeys[by_key]

    def find(keys):
        if V == 0:
            return np.full(np.shape(keys), -1, dtype=np.int64)
        p = np.clip(np.searchsorted(skeys, keys), 0, V - 1)
        return np.where(skeys[p] == keys, by_key[p], -1)
    # 4 vertices
    corner = np.array([[j & 1, j >> 1 & 1, j >> 2 & 1] for j in range(8)], dtype=np.int64)
    idx8 = find(pack(c[:, None, :] + corner[None, :, :]))      # [V][8]
    v8 = (idx8 >= 0) & valid[np.maximum(idx8, 0)]
    complete = v8.all(1)
    in8 = inside[np.maximum(idx8, 0)] & complete[:, None]
    mask = (in8.astype(np.int64) << np.arange(8)).sum(1)
    active = complete & (mask != 0) & (mask != 255)
    act = np.flatnonzero(active)
    A = len(act)
    vidx = np.full(V, -1, dtype=np.int64)
    vidx[act] = np.arange(A)
    p8, i8 = phi[idx8[act]].reshape(A, 8), in8[act].reshape(A, 8)
    m, G, k = np.zeros((A, 3)), np.zeros((A, 3)), np.zeros(A, dtype=np.int64)
    with np.errstate(all="ignore"):
        for ax in range(3):
            lb, hb = [x for x in range(3) if x != ax]
            for t4 in range(4):
                lo = (t4 & 1) << lb | (t4 >> 1) << hb
                hi = lo | 1 << ax
                G[:, ax] = G[:, ax] + (p8[:, hi] - p8[:, lo])
                cross = i8[:, lo] != i8[:, hi]
                tau = p8[:, lo] / (p8[:, lo] - p8[:, hi])
                for x in range(3):
                    m[:, x] = np.where(cross, m[:, x] + (tau if x == ax else float(lo >> x & 1)), m[:, x])
                k += cross
        ca = c[act].reshape(A, 3)
        out_xyz = o + (ca.astype(np.float64) + m / k.astype(np.float64)[:, None]) * cell
        L = np.sqrt((G[:, 0] * G[:, 0] + G[:, 1] * G[:, 1]) + G[:, 2] * G[:, 2])
        hn = (L != 0) & np.isfinite(L)
        normal = np.where(hn[:, None], G / np.where(hn, L, 1.0)[:, None], 0.0).astype(np.float32)
    nc8 = np.zeros(A, dtype=np.int64)
    sc8 = np.zeros((A, 3), dtype=np.int64)
    np.add.at(nc8, np.repeat(np.arange(A), 8), nc[idx8[act]].reshape(-1))
    np.add.at(sc8, np.repeat(np.arange(A), 8), sc[idx8[act]].reshape(-1, 3))
    n2 = np.maximum(nc8, 1)[:, None]
    ch = (2 * sc8 + n2) // (2 * n2)
    rgb = np.where(nc8 != 0, ch[:, 0] | ch[:, 1] << 8 | ch[:, 2] << 16 | 255 << 24, 0).astype(np.uint32)
    info = np.concatenate([ca, (mask[act] | k << 8)[:, None]], 1).astype(np.int32).reshape(A, 4)
    # 5 triangles
    quads = np.zeros((V, 3), dtype=bool)
    qv = np.zeros((V, 3, 4), dtype=np.int64)
    e = np.eye(3, dtype=np.int64)
    for ax in range(3):
        b, c2 = (ax + 1) % 3, (ax + 2) % 3
        nxt = idx8[:, 1 << ax]
        differ = valid & (nxt >= 0) & valid[np.maximum(nxt, 0)] & (inside != inside[np.maximum(nxt, 0)])
        Q = [find(pack(c - e[b] - e[c2])), find(pack(c - e[c2])), np.arange(V), find(pack(c - e[b]))]
        allc = differ.copy()
        for j in range(4):
            allc &= (Q[j] >= 0) & complete[np.maximum(Q[j], 0)]
            qv[:, ax, j] = vidx[np.maximum(Q[j], 0)]
        quads[:, ax] = allc
    vv, aa = np.nonzero(quads)                                 # row-major: ascending (ord, axis)
    q4 = qv[vv, aa]
    ins = inside[vv]
    t1 = np.where(ins[:, None], q4[:, [0, 1, 2]], q4[:, [0, 2, 1]])
    t2 = np.where(ins[:, None], q4[:, [0, 2, 3]], q4[:, [0, 3, 2]])
    tri = np.stack([t1, t2], 1).reshape(-1, 3).astype(np.int32)
    report = np.array([n, used.sum(), len(ckeys), V, valid.sum(), A, len(tri), 0], dtype=np.int32)
    return dict(vox=vkeys, ord=vord, w=w, st=st, nc=nc, sc=sc, xyz=out_xyz.reshape(A, 3), normal=normal.reshape(A, 3), rgba8=rgb, info=info,
                tri=tri, report=report, valid=valid, inside=inside)


# ---- the restatement: one loop per voxel, cube and edge, Python ints and floats, a dict -------------------------------------------

def mesh_loop(xyz, src, depth, views, n_frames, P, cell, origin, band=1, trunc_cells=3, min_weight=1, agree=None, min_agree=0,
              rgba8=None, frame_ids=None, count=None):
    """The same rule one voxel, one cube and one edge at a time -> the same dict as mesh (without valid, inside)"""
    xyz, src, depth, views, P, agree, rgba8 = _prep(xyz, src, depth, views, P, agree, rgba8)
    R, H, W = depth.shape
    B, cell = int(band), float(cell)
    n, used, g = used_cells(xyz, src, depth, views, n_frames, P, cell, origin, count)
    org = [float(x) for x in origin]
    trunc = float(trunc_cells) * cell
    vox, seen = {}, set()                                     # node -> ord
    for i in range(n):
        if not used[i]:
            continue
        gi = tuple(int(x) for x in g[i])
        if gi in seen:
            continue
        seen.add(gi)
        for d2 in range(2 * B):
            for d1 in range(2 * B):
                for d0 in range(2 * B):
                    node = (gi[0] - B + 1 + d0, gi[1] - B + 1 + d1, gi[2] - B + 1 + d2)
                    o = 256 * i + (d2 * 2 * B + d1) * 2 * B + d0
                    if node not in vox or o < vox[node]:
                        vox[node] = o
    order = sorted(vox, key=vox.get)
    cams = []
    for r in range(R):
        f = int(views[r, 0])
        cm = cloud_ref._camera_loop(P[f]) if 0 <= f < n_frames else None
        sl = depth_ref.slot_of(frame_ids, len(rgba8), n_frames, f) if rgba8 is not None else -1
        cams.append(None if cm is None else ([float(x) for x in P[f]], cm[2], sl))
    state = {}
    for node in order:
        X = [org[a] + float(node[a]) * cell for a in range(3)]
        w = st = nc = 0
        sc = [0, 0, 0]
        for r in range(R):
            if cams[r] is None:
                continue
            p, sn, sl = cams[r]                               # sn = sign(det) ||m3||: d = q_2 / (||m3|| / sign) needs them apart
            q = [((p[4 * i] * X[0] + p[4 * i + 1] * X[1]) + p[4 * i + 2] * X[2]) + p[4 * i + 3] for i in range(3)]
            if not q[2] > 0.0:
                continue
            us, vs = cloud_ref._fdiv(q[0], q[2]) + 0.5, cloud_ref._fdiv(q[1], q[2]) + 0.5
            if not (0.0 <= us < W and 0.0 <= vs < H):
                continue
            u, v = int(us), int(vs)
            z = float(depth[r, v, u])
            if not math.isfinite(z) or (agree is not None and int(agree[r, v, u]) < min_agree):
                continue
            sg = 1.0 if sn > 0.0 else -1.0
            dist = cloud_ref._fdiv(sg * q[2], abs(sn))
            s = z - dist
            if not s >= -trunc:
                continue
            t = trunc if s > trunc else s
            w += 1
            st += math.floor((t / trunc) * 32767.0 + 0.5)
            if s <= trunc and sl >= 0:
                colour = int(rgba8[sl, v, u])
                nc += 1
                for a in range(3):
                    sc[a] += (colour >> (8 * a)) & 255
        state[node] = (w, st, nc, sc)
    valid = {node: state[node][0] >= min_weight for node in order}
    inside = {node: valid[node] and state[node][1] < 0 for node in order}

    def corners(cu):
        return [(cu[0] + (j & 1), cu[1] + (j >> 1 & 1), cu[2] + (j >> 2 & 1)) for j in range(8)]

    def is_complete(cu):
        return all(valid.get(x, False) for x in corners(cu))
    EDGES = [(ax, (t & 1) << [x for x in range(3) if x != ax][0] | (t >> 1) << [x for x in range(3) if x != ax][1])
             for ax in range(3) for t in range(4)]
    vindex, oxyz, onrm, orgb, oinf = {}, [], [], [], []
    for cu in order:
        if not is_complete(cu):
            continue
        cs = corners(cu)
        ins = [inside[x] for x in cs]
        if all(ins) or not any(ins):
            continue
        phi = [float(state[x][1]) / float(state[x][0]) for x in cs]
        m, G, k = [0.0, 0.0, 0.0], [0.0, 0.0, 0.0], 0
        for ax, lo in EDGES:
            hi = lo | 1 << ax
            G[ax] = G[ax] + (phi[hi] - phi[lo])
            if ins[lo] != ins[hi]:
                tau = phi[lo] / (phi[lo] - phi[hi])
                for a in range(3):
                    m[a] = m[a] + (tau if a == ax else float(lo >> a & 1))
                k += 1
        vindex[cu] = len(oxyz)
        oxyz.append([org[a] + (float(cu[a]) + m[a] / float(k)) * cell for a in range(3)])
        L2 = (G[0] * G[0] + G[1] * G[1]) + G[2] * G[2]
        L = math.sqrt(L2) if math.isfinite(L2) else math.inf
        onrm.append([np.float32(x / L) for x in G] if L != 0.0 and math.isfinite(L) else [np.float32(0)] * 3)
        tnc = sum(state[x][2] for x in cs)
        tsc = [sum(state[x][3][a] for x in cs) for a in range(3)]
        ch = [(2 * x + tnc) // (2 * tnc) for x in tsc] if tnc else None
        orgb.append((ch[0] | ch[1] << 8 | ch[2] << 16 | 255 << 24) if ch else 0)
        oinf.append([cu[0], cu[1], cu[2], sum(1 << j for j in range(8) if ins[j]) | k << 8])
    tri = []
    for cu in order:
        for ax in range(3):
            nx = tuple(cu[a] + (1 if a == ax else 0) for a in range(3))
            if not (valid[cu] and valid.get(nx, False) and inside[cu] != inside[nx]):
                continue
            b, c2 = (ax + 1) % 3, (ax + 2) % 3

            def back(node, *axes):
                return tuple(node[a] - (1 if a in axes else 0) for a in range(3))
            Q = [back(cu, b, c2), back(cu, c2), cu, back(cu, b)]
            if not all(x in valid and is_complete(x) for x in Q):
                continue
            v = [vindex[x] for x in Q]
            tri += [[v[0], v[1], v[2]], [v[0], v[2], v[3]]] if inside[cu] else [[v[0], v[2], v[1]], [v[0], v[3], v[2]]]
    V, A = len(order), len(oxyz)
    get = lambda j: np.array([state[x][j] for x in order], dtype=np.int64).reshape((V, 3) if j == 3 else (V,))  # noqa: E731
    report = np.array([n, int(used.sum()), len(seen), V, sum(valid.values()), A, len(tri), 0], dtype=np.int32)
    return dict(vox=pack(np.array(order, dtype=np.int64).reshape(V, 3)), ord=np.array([vox[x] for x in order], dtype=np.int64).reshape(V),
                w=get(0), st=get(1), nc=get(2), sc=get(3), xyz=np.array(oxyz, dtype=np.float64).reshape(A, 3),
                normal=np.array(onrm, dtype=np.float32).reshape(A, 3), rgba8=np.array(orgb, dtype=np.uint32).reshape(A),
                info=np.array(oinf, dtype=np.int32).reshape(A, 4), tri=np.array(tri, dtype=np.int32).reshape(-1, 3), report=report)


def assert_same(a, b, keys=INT_KEYS + FLOAT_KEYS):
    for k in keys:
        x, y = np.asarray(a[k]), np.asarray(b[k])
        assert x.shape == y.shape, (k, x.shape, y.shape)
        if k in FLOAT_KEYS:
            assert bits(x.astype(y.dtype)) == bits(y), (k, np.argwhere(x != y)[:5])
        else:
            assert (x.astype(np.int64) == y.astype(np.int64)).all(), (k, np.argwhere(x != y)[:5])


def by_cube(m):
    """a mesh up to renumbering: the vertices sorted by their cube, the triangles as sorted rows of cube triples (each rotated to
    start at its smallest cube: the orientation stays)"""
    info = np.asarray(m["info"])
    o = np.lexsort(info[:, :3].T[::-1]) if len(info) else np.zeros(0, dtype=np.int64)
    rank = np.empty(len(o), dtype=np.int64)
    rank[o] = np.arange(len(o))
    t = rank[np.asarray(m["tri"], dtype=np.int64)] if len(m["tri"]) else np.zeros((0, 3), dtype=np.int64)
    first = t.argmin(1) if len(t) else np.zeros(0, dtype=np.int64)
    t = np.stack([t[np.arange(len(t)), (first + j) % 3] for j in range(3)], 1) if len(t) else t
    t = t[np.lexsort(t.T[::-1])] if len(t) else t
    return dict(xyz=np.asarray(m["xyz"])[o], normal=np.asarray(m["normal"])[o], rgba8=np.asarray(m["rgba8"])[o], info=info[o], tri=t)


# ---- the exact invariants of any mesh of the rule ------------------------------------------------------------------------------

def check_invariants(m, cell, origin):
    xyz, info, tri = m["xyz"], m["info"].astype(np.int64), m["tri"].astype(np.int64)
    A = len(xyz)
    o = np.asarray(origin, dtype=np.float64)
    lo, hi = o + info[:, :3].astype(np.float64) * cell, o + (info[:, :3] + 1).astype(np.float64) * cell
    assert ((xyz >= lo) & (xyz <= hi)).all()                  # the closed box of the cube
    assert len(tri) % 2 == 0 and (len(tri) == 0 or (tri.min() >= 0 and tri.max() < A))
    q = tri.reshape(-1, 6)
    assert all(len(set(row)) == 4 for row in q.tolist())       # a quad's four vertices are distinct
    assert (q[:, 0] == q[:, 3]).all()
    # every diagonal v0 - v2 is in exactly two triangles
    und = {}
    for t in tri:
        for a, b in ((0, 1), (1, 2), (2, 0)):
            kx = (min(t[a], t[b]), max(t[a], t[b]))
            und[kx] = und.get(kx, 0) + 1
    for row in q:
        d2 = row[2] if row[2] == row[4] else row[1]          # the vertex both triangles share besides v0
        assert und[(min(row[0], d2), max(row[0], d2))] == 2


def orientation_exceptions(m):
    """the triangles whose cross product has no positive dot product with the normal of one of its vertices"""
    xyz, nrm, tri = m["xyz"], m["normal"].astype(np.float64), m["tri"].astype(np.int64)
    if not len(tri):
        return 0
    cr = np.cross(xyz[tri[:, 1]] - xyz[tri[:, 0]], xyz[tri[:, 2]] - xyz[tri[:, 0]])
    good = np.ones(len(tri), dtype=bool)
    for j in range(3):
        good &= (cr * nrm[tri[:, j]]).sum(1) > 0
    return int((~good).sum())


def directed_edges(tri):
    d = {}
    for t in np.asarray(tri, dtype=np.int64):
        for a, b in ((0, 1), (1, 2), (2, 0)):
            d[(int(t[a]), int(t[b]))] = d.get((int(t[a]), int(t[b])), 0) + 1
    return d


# ---- k_mesh.hip's constants and hash --------------------------------------------------------------------------------------------

def kernel_constants(csrc):
    text = open(os.path.join(csrc, "k_mesh.hip")).read()
    c = {k: int(v) for k, v in re.findall(r"\b(MSH_NT|MSH_GRID_MAX|MSH_LG_TMIN|MSH_MARGIN) = (\d+)", text)}
    c["MSH_HASH_MUL"] = int(re.search(r"MSH_HASH_MUL = (0x[0-9A-Fa-f]+)ull", text).group(1), 16)
    assert "(key * MSH_HASH_MUL) >> (64 - lg)" in text and "h = (h + 1) & mask" in text   # the hash and the probe restated below
    assert "< 2 * (size_t)a.max_voxels" in text                                           # ... and the table's size
    return c


def table_lg(max_voxels, c):
    lg = c["MSH_LG_TMIN"]
    while (1 << lg) < 2 * max_voxels:
        lg += 1
    return lg


def table_hash(key, lg, c):
    return ((int(key) * c["MSH_HASH_MUL"]) & (2**64 - 1)) >> (64 - lg)


# ---- cases ---------------------------------------------------------------------------------------------------------------------------

CELL, ORIGIN = cloud_ref.CELL, cloud_ref.ORIGIN


def boundary_case():
    """cloud_ref.boundary_case (NaN and infinite points, bad src, a skipped map, every boundary cell and one outside) with the
    points that this rule's margin turns away and keeps: g at -2^20 + 4 and 2^20 - 5 (used) and one cell further out (not), a -P
    camera, and agreement counts"""
    c = cloud_ref.boundary_case()
    lo, hi = ORIGIN[0] - GB * CELL, ORIGIN[0] + GB * CELL
    edge = []
    for a in range(3):
        for x in (lo + 4 * CELL, lo + 3 * CELL, hi - 5 * CELL, hi - 4 * CELL):
            e = [0.25, 0.25, 0.25]
            e[a] = x + CELL / 4
            edge.append(e)
    P = c["P"].copy()
    P[1] = -P[1]
    f = depth_ref.fuse(np.where(np.isfinite(c["depth"]), c["depth"], 3.0), c["views"], 4, P, 0.05, 0)
    return dict(c, xyz=np.concatenate([c["xyz"], np.array(edge)]), src=np.concatenate([c["src"], np.tile([[0, 7]], (len(edge), 1))]).astype(np.int32),
                P=P, agree=f["agree"])


def plane_case(zconst, band=1, trunc_cells=3):
    """scene()'s five R = I cameras with depth maps that are the constant zconst, the list the filter makes of them"""
    sc = depth_ref.scene(0.0)
    depth = np.full((5, depth_ref.SCENE_H, depth_ref.SCENE_W), float(zconst))
    f = depth_ref.fuse(depth, depth_ref.all_views(), 5, sc["P"], 0.05, 1)
    return dict(xyz=f["xyz"], src=f["src"], depth=depth, views=depth_ref.all_views(), P=sc["P"], agree=f["agree"])


def truth_figures(m, cell, trunc):
    """the Truth figures of a mesh of the two-plane scenes (back plane z = 4, front rectangle z = 3, |x| < 0.5, |y| < 0.35)"""
    xyz, nrm = m["xyz"], m["normal"]
    dist = np.minimum(np.abs(xyz[:, 2] - 4.0), np.abs(xyz[:, 2] - 3.0))
    near = dist <= cell / 4
    # the distance in (x, y) to the rectangle's silhouette: its outline
    dx, dy = np.abs(xyz[:, 0]) - 0.5, np.abs(xyz[:, 1]) - 0.35
    outside = np.hypot(np.maximum(dx, 0), np.maximum(dy, 0))
    sil = np.where((dx <= 0) & (dy <= 0), np.minimum(-dx, -dy), outside)
    sel = near & (sil > trunc)
    ang = cloud_ref.angle_to(nrm[sel], (0, 0, -1)) if sel.any() else np.zeros(0)
    return dict(vertices=len(xyz), triangles=len(m["tri"]), near=float(near.mean()) if len(xyz) else 0.0,
                worst=float(dist.max()) if len(xyz) else 0.0, normals=float((ang <= np.radians(20.0)).mean()) if len(ang) else 0.0,
                mean=float(dist.mean()) if len(xyz) else 0.0)


# The grid of the truth cases.  The scenes' planes z = 3 and z = 4 are lattice layers of ORIGIN's grid; the sign of phi at a node
# that lies on the surface is the sign of d's rounding error (with R = I, d is exact: the exact special case of
# tests/test_mesh_ref.py), which is the degenerate case of every iso-surface rule.  The truth cases put the layers 0.4 cell off.
TRUTH_ORIGIN = (-8.0, -8.0, -8.0 + 0.4 / 32.0)
TRUTH_BAND, TRUTH_TRUNC = 2, 3

# case -> (vertices, triangles, floor of the fraction of vertices within cell / 4 of a plane, floor of the fraction of normals
# within 20 degrees of (0, 0, -1) among those more than trunc from the silhouette, ceiling of the largest distance to the nearer
# plane, triangles whose orientation disagrees with a vertex normal).  The floors are the measured fractions less 0.01, rounded
# down to two digits; the ceiling the measured distance plus 0.01, rounded up (DESIGN.md section 29 has the measured figures):
# rotated-true 0.96427 / 1.0 / 0.04179; plain 0.09621 / 0.99760 / 0.18438; rotated 0.36916 / 0.86844 / 0.18438.
FLOORS = {"rotated-true": (6689, 12692, 0.95, 0.99, 0.06, 0), "plain": (6652, 12598, 0.08, 0.98, 0.20, 0),
          "rotated": (7807, 14388, 0.35, 0.85, 0.20, 82)}


def truth_inputs(case):
    """-> dict(depth, P, min_agree, xyz, src, agree): rotated-true: scene_rotated() at its true depths through the filter at
    0.05 / 1; plain and rotated: the sweep's maps of scene(0.0) and scene_rotated() through the filter at 0.05 / 2"""
    V = depth_ref.all_views()
    sc = depth_ref.scene(0.0) if case == "plain" else depth_ref.scene_rotated()
    if case == "rotated-true":
        depth, k = sc["ztrue"], 1
    else:
        depth, k = depth_ref.depth_maps(sc["gray"], None, 5, sc["P"], V, [sc["range"]] * 5, depth_ref.SCENE_D, 2, 2, 2**30)["depth"], 2
    f = depth_ref.fuse(depth, V, 5, sc["P"], 0.05, k)
    return dict(depth=depth, P=sc["P"], min_agree=k, xyz=f["xyz"], src=f["src"], agree=f["agree"], views=V)


def floor2(x):
    """a measured fraction less 0.01, rounded down to two digits"""
    return math.floor((x - 0.01) * 100.0) / 100.0
