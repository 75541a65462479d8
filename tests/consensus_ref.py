"""numpy float64 restatement of track consensus (include/pgx.h, "track consensus"): the yardstick of
tests/test_gpu_consensus.py.  Every value is a float64 and every operation one IEEE operation in the order the header
writes it (sums of three as ((a + b) + c), no dot products from a library), vectorised over the hypotheses and the
observations of one track only -- so the integer outputs can be held to this file exactly.  Besides the outputs it
reports, per track, whether any decision of any hypothesis lies within `rel` of its threshold (`near`)."""
import math

import numpy as np

FEWVIEWS, LOWPARALLAX, NOCONSENSUS, SHORT = 1, 2, 4, 8
TRI_FEWVIEWS = 1
M64 = (1 << 64) - 1


def splitmix64(s):
    """-> (new state, value)"""
    s = (s + 0x9E3779B97F4A7C15) & M64
    z = s
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return s, z ^ (z >> 31)


def sampled_pair(seed, t, h, n):
    """ransac_stream(seed, t, h) and ransac_draw(st, n, 2): two distinct positions, the smaller first"""
    st = (seed ^ ((t & 0xFFFFFFFF) << 32) ^ (((h & 0xFFFFFFFF) * 0xD1B54A32D192ED03) & M64)) & M64
    ids = []
    while len(ids) < 2:
        st, z = splitmix64(st)
        c = z % n
        if c not in ids:
            ids.append(int(c))
    return min(ids), max(ids)


def pairs_of(n_k, max_hyp, seed, t):
    """the hypotheses' pairs (i [nh], j [nh]) and whether they are the exhaustive list"""
    n_p = n_k * (n_k - 1) // 2
    if n_p <= max_hyp:
        i, j = np.triu_indices(n_k, 1)      # lexicographic
        return i, j, True
    ij = [sampled_pair(seed, t, h, n_k) for h in range(max_hyp)]
    return np.array([p[0] for p in ij]), np.array([p[1] for p in ij]), False


def frames(P):
    """P [F][12] -> (known [F], M [F][3][3], Minv [F][3][3], C [F][3], sgn [F]) by the header's rule"""
    P = np.asarray(P, dtype=np.float64).reshape(-1, 3, 4)
    M, p4 = P[:, :, :3].copy(), P[:, :, 3]
    fin = np.isfinite(P).all(axis=(1, 2))
    m = lambda r, c: M[:, r, c]
    with np.errstate(all="ignore"):
        k = np.empty_like(M)                # cofactors
        k[:, 0, 0] = m(1, 1) * m(2, 2) - m(1, 2) * m(2, 1)
        k[:, 0, 1] = m(1, 2) * m(2, 0) - m(1, 0) * m(2, 2)
        k[:, 0, 2] = m(1, 0) * m(2, 1) - m(1, 1) * m(2, 0)
        k[:, 1, 0] = m(0, 2) * m(2, 1) - m(0, 1) * m(2, 2)
        k[:, 1, 1] = m(0, 0) * m(2, 2) - m(0, 2) * m(2, 0)
        k[:, 1, 2] = m(0, 1) * m(2, 0) - m(0, 0) * m(2, 1)
        k[:, 2, 0] = m(0, 1) * m(1, 2) - m(0, 2) * m(1, 1)
        k[:, 2, 1] = m(0, 2) * m(1, 0) - m(0, 0) * m(1, 2)
        k[:, 2, 2] = m(0, 0) * m(1, 1) - m(0, 1) * m(1, 0)
        det = (m(0, 0) * k[:, 0, 0] + m(0, 1) * k[:, 0, 1]) + m(0, 2) * k[:, 0, 2]
        known = fin & (det != 0)
        Minv = np.transpose(k, (0, 2, 1)) / det[:, None, None]
        C = -((Minv[:, :, 0] * p4[:, 0:1] + Minv[:, :, 1] * p4[:, 1:2]) + Minv[:, :, 2] * p4[:, 2:3])
    return known, M, Minv, C, np.where(det > 0, 1.0, -1.0)


def dot3(x, y):
    return (x[..., 0] * y[..., 0] + x[..., 1] * y[..., 1]) + x[..., 2] * y[..., 2]


def _close(p, q, rel):
    return np.abs(p - q) <= rel * np.maximum(np.abs(p), np.abs(q))


def hypotheses(d, C, i, j, cos2, rel):
    """d, C [n_k][3] of the known observations; pairs (i, j) -> (valid [nh], X' [nh][3] relative to C_i, near [nh])"""
    di, dj = d[i], d[j]
    w0 = C[i] - C[j]
    a, b, c, dd, e = dot3(di, di), dot3(di, dj), dot3(dj, dj), dot3(di, w0), dot3(dj, w0)
    with np.errstate(all="ignore"):
        den = a * c - b * b
        gate = (b > 0) & (b * b >= cos2 * (a * c))
        s = (b * e - c * dd) / den
        tt = (a * e - b * dd) / den
        valid = ~gate & (den > 0) & (s > 0) & (tt > 0)
        X = 0.5 * (s[:, None] * di + (tt[:, None] * dj - w0))
        near = ((b > 0) & _close(b * b, cos2 * (a * c), rel)) | _close(a * c, b * b, rel)
        live = ~gate & (den > 0)
        near |= live & (_close(b * e, c * dd, rel) | _close(a * e, b * dd, rel))
    return valid, X, near


def inliers(X, Ci, M, C, uv, sgn, px, rel):
    """X, Ci [nh][3]; M [n_k][3][3], C [n_k][3], uv [n_k][2], sgn [n_k] -> (inlier [nh][n_k], near [nh])"""
    with np.errstate(all="ignore"):
        y = X[:, None, :] + (Ci[:, None, :] - C[None, :, :])                      # [nh][n_k][3]
        t = M[None, :, :, :] * y[:, :, None, :]                                   # [nh][n_k][3 rows][3]
        h = (t[..., 0] + t[..., 1]) + t[..., 2]
        w = h[..., 2]
        ap, bp, ep = h[..., 0] - uv[None, :, 0] * w, h[..., 1] - uv[None, :, 1] * w, px * w
        lhs, rhs = ap * ap + bp * bp, ep * ep
        inl = (sgn[None, :] * w > 0) & (lhs <= rhs)
        near = _close(lhs, rhs, rel) | (np.abs(w) <= rel * np.abs(t[..., 2, :]).sum(-1))
    return inl, near.any(axis=1)


def consensus(kps, P, offsets, nodes, inlier_px=4.0, min_parallax_deg=1.0, min_inliers=2, min_len=2, max_hyp=256, seed=0,
              in_summary=None, track_of=None, stride=None, rel=1e-9):
    """kps[frame] = [n][2] (x, y) or KEYPOINT_DTYPE; P [n_frames][12]; offsets [n_tracks + 1]; nodes [n_nodes][2];
    in_summary [8] (slots 2, 3, 4, 6 are copied); track_of [n_frames][stride] or None (a rewritten copy is returned).
    -> dict(offsets, nodes, summary [8], map [n], xyz [n_out][3], flags [n_out], stats [n][4], report [8], track_of,
            near [n] bool, keep [n_nodes] bool)"""
    known, M, Minv, C, sgn = frames(P)
    nf = len(known)
    xy = [np.stack([k["x"], k["y"]], 1).astype(np.float64) if k.dtype.names else np.asarray(k, dtype=np.float64).reshape(-1, 2)
          for k in kps]
    if stride is None:
        stride = max(1, max(len(k) for k in xy))
    offsets, nodes = np.asarray(offsets), np.asarray(nodes).reshape(-1, 2)
    nt = len(offsets) - 1
    min_len = max(1, int(min_len))
    c1 = math.cos(min_parallax_deg * math.pi / 180.0)
    cos2 = c1 * c1
    stats = np.zeros((nt, 4), np.int32)
    near = np.zeros(nt, bool)
    keep = np.zeros(len(nodes), bool)
    point = np.full((nt, 3), np.nan)
    kept = np.zeros(nt, np.int64)
    rep = np.zeros(8, np.int64)
    memo = {}
    for t in range(nt):
        o = np.arange(offsets[t], offsets[t + 1])
        f, k = nodes[o, 0], nodes[o, 1]
        valid = (f >= 0) & (f < nf) & (k >= 0) & (k < stride)
        kn = valid.copy()
        kn[valid] = known[f[valid]]
        n_k = int(kn.sum())
        key = (tuple(f), tuple(k))
        sampled = n_k * (n_k - 1) // 2 > max_hyp
        if not sampled and key in memo:
            bits, inl_n, hwin, X, kp_t, nr = memo[key]
        else:
            bits, inl_n, hwin, X, nr = 0, 0, -1, np.full(3, np.nan), False
            kp_t = valid.copy()
            if n_k < 2:
                bits = FEWVIEWS
            else:
                fk, kk = f[kn], k[kn]
                uv = np.array([xy[a][b] if b < len(xy[a]) else (0.0, 0.0) for a, b in zip(fk, kk)], dtype=np.float64).reshape(-1, 2)
                Mi = Minv[fk]
                d = sgn[fk][:, None] * ((Mi[:, :, 0] * uv[:, 0:1] + Mi[:, :, 1] * uv[:, 1:2]) + Mi[:, :, 2])
                i, j, _ = pairs_of(n_k, max_hyp, seed, t)
                ok, Xh, nr_h = hypotheses(d, C[fk], i, j, cos2, rel)
                nr = bool(nr_h.any())
                if not ok.any():
                    bits = LOWPARALLAX
                else:
                    hs = np.flatnonzero(ok)
                    inl, nr_p = inliers(Xh[hs], C[fk][i[hs]], M[fk], C[fk], uv, sgn[fk], inlier_px, rel)
                    nr = nr or bool(nr_p.any())
                    cnt = inl.sum(1)
                    w = int(np.argmax(cnt))            # the first of the largest: ties to the smallest h
                    hwin, inl_n = int(hs[w]), int(cnt[w])
                    X = Xh[hwin] + C[fk][i[hwin]]
                    if inl_n < min_inliers:
                        bits = NOCONSENSUS
                    kp_t[np.flatnonzero(kn)] = inl[w]
            if not sampled:
                memo[key] = (bits, inl_n, hwin, X, kp_t, nr)
        n_keep = int(kp_t.sum())
        rep[2] += len(o)
        if not bits & (FEWVIEWS | LOWPARALLAX | NOCONSENSUS):
            rep[4] += n_k - inl_n
        if bits & NOCONSENSUS:
            n_keep = 0
        elif n_keep < min_len:
            bits |= SHORT
            n_keep = 0
        rep[5] += bool(bits & NOCONSENSUS)
        rep[6] += bool(bits & SHORT)
        rep[7] += bool(bits & (FEWVIEWS | LOWPARALLAX))
        stats[t] = (n_k, inl_n, hwin, bits)
        near[t], keep[o], point[t], kept[t] = nr, kp_t, X, n_keep
    surv = kept > 0
    tmap = np.where(surv, np.cumsum(surv) - 1, -1).astype(np.int32)
    out_off = np.concatenate([[0], np.cumsum(kept[surv])]).astype(np.int32)
    node_track = np.repeat(np.arange(nt), np.diff(offsets))
    sel = keep & surv[node_track]
    summary = np.zeros(8, np.int32)
    if in_summary is not None:
        summary[[2, 3, 4, 6]] = np.asarray(in_summary)[[2, 3, 4, 6]]
    summary[0], summary[1], summary[5] = surv.sum(), sel.sum(), kept.max(initial=0)
    rep[0], rep[1], rep[3] = nt, surv.sum(), sel.sum()
    und = (stats[surv, 3] & (FEWVIEWS | LOWPARALLAX)) != 0
    out = dict(offsets=out_off, nodes=nodes[sel].astype(np.int32), summary=summary, map=tmap,
               xyz=np.where(und[:, None], np.nan, point[surv]), flags=np.where(und, TRI_FEWVIEWS, 0).astype(np.int32), stats=stats,
               report=rep.astype(np.int32), near=near, keep=keep, track_of=None)
    if track_of is not None:
        to = np.array(track_of, dtype=np.int32).reshape(nf, -1)
        f, k = nodes[:, 0], nodes[:, 1]
        ok = (f >= 0) & (f < nf) & (k >= 0) & (k < stride)
        val = np.where(surv[node_track], np.where(keep, tmap[node_track], -3), -1)
        to[f[ok], k[ok]] = val[ok]
        out["track_of"] = to
    return out


def plant_swaps(scene, offsets, nodes, frac, seed):
    """Wrong observations by swapping the keypoints of two tracks in a frame they share: rng = default_rng(seed); cand =
    rng.permutation(nt)[: int(frac * nt) // 2 * 2] taken as pairs (a, b); a pair is skipped unless both tracks have >= 3
    nodes and share a frame; f = rng.choice(common); the two keypoint indices in frame f are swapped.
    -> (nodes with the swaps, planted [n_nodes] bool)"""
    rng = np.random.default_rng(seed)
    offsets, nodes = np.asarray(offsets), np.array(nodes).reshape(-1, 2)
    nt = len(offsets) - 1
    planted = np.zeros(len(nodes), bool)
    cand = rng.permutation(nt)[: int(frac * nt) // 2 * 2]
    for a, b in cand.reshape(-1, 2):
        ra, rb = np.arange(offsets[a], offsets[a + 1]), np.arange(offsets[b], offsets[b + 1])
        if len(ra) < 3 or len(rb) < 3:
            continue
        common = np.intersect1d(nodes[ra, 0], nodes[rb, 0])
        if not len(common):
            continue
        f = rng.choice(common)
        ia, ib = ra[nodes[ra, 0] == f][0], rb[nodes[rb, 0] == f][0]
        nodes[ia, 1], nodes[ib, 1] = nodes[ib, 1], nodes[ia, 1]
        planted[ia] = planted[ib] = True
    return nodes, planted


def brute_force(kps, P, offsets, nodes, inlier_px, min_parallax_deg):
    """Another formulation of the exhaustive form, for scenes near the origin: every pair's midpoint in world coordinates by
    np.linalg.lstsq-free closed form with library dot products, scored with P directly (h = P (X, 1), a division-free
    pixel test).  -> per track (n_k, inliers of the winner, winning h or -1, keep mask of the track's nodes) or None where
    undecided"""
    P3 = np.asarray(P, dtype=np.float64).reshape(-1, 3, 4)
    fin = np.isfinite(P3).all(axis=(1, 2))
    xy = [np.stack([k["x"], k["y"]], 1).astype(np.float64) if k.dtype.names else np.asarray(k, dtype=np.float64).reshape(-1, 2)
          for k in kps]
    cosm = math.cos(math.radians(min_parallax_deg))
    offsets, nodes = np.asarray(offsets), np.asarray(nodes).reshape(-1, 2)
    out = []
    for t in range(len(offsets) - 1):
        nd = nodes[offsets[t]:offsets[t + 1]]
        kn = np.array([fin[f] and np.linalg.det(P3[f][:, :3]) != 0 for f, _ in nd], dtype=bool)
        obs = nd[kn]
        if len(obs) < 2:
            out.append(None)
            continue
        cams = []
        for f, k in obs:
            Mm, p4 = P3[f][:, :3], P3[f][:, 3]
            Mi = np.linalg.inv(Mm)
            d = np.sign(np.linalg.det(Mm)) * (Mi @ np.array([xy[f][k][0], xy[f][k][1], 1.0]))
            cams.append((-Mi @ p4, d, P3[f], xy[f][k], np.sign(np.linalg.det(Mm))))
        best, h = (-1, -1, None), -1
        for i in range(len(obs)):
            for j in range(i + 1, len(obs)):
                h += 1
                (Ci, di, _, _, _), (Cj, dj, _, _, _) = cams[i], cams[j]
                cosang = di @ dj / np.sqrt((di @ di) * (dj @ dj))
                if cosang >= cosm:
                    continue
                A = np.stack([di, -dj], 1)
                st, *_ = np.linalg.lstsq(A, Cj - Ci, rcond=None)
                if not (st[0] > 0 and st[1] > 0):
                    continue
                X = 0.5 * ((Ci + st[0] * di) + (Cj + st[1] * dj))
                inl = []
                for (_, _, Pm, uv, sg) in cams:
                    hh = Pm[:, :3] @ X + Pm[:, 3]
                    inl.append(sg * hh[2] > 0 and (hh[0] - uv[0] * hh[2]) ** 2 + (hh[1] - uv[1] * hh[2]) ** 2 <= (inlier_px * hh[2]) ** 2)
                if sum(inl) > best[0]:
                    best = (sum(inl), h, np.array(inl))
        if best[1] < 0:
            out.append(None)
            continue
        keep = np.ones(len(nd), bool)
        keep[np.flatnonzero(kn)] = best[2]
        out.append((len(obs), best[0], best[1], keep))
    return out
