"""numpy float64 restatement of multi-view track triangulation (include/pgx.h, "multi-view triangulation of tracks"): the
yardstick of tests/test_gpu_triangulate.py.  The null vector comes from np.linalg.svd of the 2n x 4 system (the kernel takes
the Gram matrix's smallest eigenvector by Jacobi), the Gauss-Newton steps from np.linalg.solve; tests/test_triangulate_ref.py
ties this file to a literal Python loop.  Besides the outputs it returns the quantity behind every flag decision, so that a
test can leave out tracks that lie within rounding of a threshold."""
import numpy as np

FEWVIEWS, DEGENERATE, BEHIND, PARALLAX, REPROJ = 1, 2, 4, 8, 16
W_MIN = 1e-12     # |v[3]| <= W_MIN: the null vector is at infinity


def cameras(P):
    """P [F][12] -> (known [F] bool, C [F][3], sign det M [F], ||m3|| [F])"""
    P = np.asarray(P, dtype=np.float64).reshape(-1, 3, 4)
    M, p4 = P[:, :, :3], P[:, :, 3]
    finite = np.isfinite(P).all(axis=(1, 2))
    with np.errstate(all="ignore"):
        det = np.linalg.det(np.where(finite[:, None, None], M, 0.0))
        known = finite & (det != 0)
        C = np.full((len(P), 3), np.nan)
        if known.any():
            C[known] = -np.linalg.solve(M[known], p4[known][:, :, None])[:, :, 0]
    return known, C, np.where(det > 0, 1.0, -1.0), np.linalg.norm(P[:, 2, :3], axis=1)


def _project(Q, X):
    h = Q[:, :, :3] @ X + Q[:, :, 3]
    return h[:, :2] / h[:, 2:3], h[:, 2]


def triangulate(kps, P, offsets, nodes, min_parallax_deg, max_reproj_px, refine_iters):
    """kps[frame] = [n][2] (x, y) or KEYPOINT_DTYPE; P [n_frames][12]; offsets [n_tracks + 1]; nodes [n_nodes][2].
    -> dict(xyz, quality, flags, node_err, summary [8], and per track: w = |v[3]|, maxe, parallax, min_depth)"""
    P = np.asarray(P, dtype=np.float64).reshape(-1, 3, 4)
    known, C, sgn, n3 = cameras(P)
    xy = [np.stack([k["x"], k["y"]], 1).astype(np.float64) if k.dtype.names else np.asarray(k, dtype=np.float64) for k in kps]
    offsets, nodes = np.asarray(offsets), np.asarray(nodes).reshape(-1, 2)
    nt = len(offsets) - 1
    out = dict(xyz=np.full((nt, 3), np.nan), quality=np.full((nt, 3), np.nan), flags=np.zeros(nt, np.int32),
               node_err=np.full(len(nodes), np.nan), w=np.full(nt, np.nan), maxe=np.full(nt, np.nan),
               parallax=np.full(nt, np.nan), min_depth=np.full(nt, np.nan))
    used_total = 0
    for t in range(nt):
        o = np.arange(offsets[t], offsets[t + 1])
        f = nodes[o, 0]
        use = known[f]
        o, f = o[use], f[use]
        used_total += len(o)
        if len(o) < 2:
            out["flags"][t] = FEWVIEWS
            continue
        uv = np.array([xy[fr][k] for fr, k in nodes[o]])
        S = C[f].mean(axis=0)
        Q = P[f].copy()
        Q[:, :, 3] += Q[:, :, :3] @ S
        rows = np.concatenate([uv[:, 0:1] * Q[:, 2] - Q[:, 0], uv[:, 1:2] * Q[:, 2] - Q[:, 1]])
        rows /= np.linalg.norm(rows, axis=1, keepdims=True)
        v = np.linalg.svd(rows)[2][-1]
        out["w"][t] = abs(v[3])
        if not np.isfinite(v).all() or abs(v[3]) <= W_MIN:
            out["flags"][t] = DEGENERATE
            continue
        X = v[:3] / v[3]
        if refine_iters > 0:
            cost_prev, Xp = 0.0, X
            for it in range(refine_iters + 1):
                p, z = _project(Q, X)
                r = p - uv
                c = float((r ** 2).sum())
                if it > 0 and not c < cost_prev:
                    X = Xp
                    break
                if it == refine_iters:
                    break
                J = (Q[:, :2, :3] - p[:, :, None] * Q[:, 2:3, :3]) / z[:, None, None]    # [n][2][3]
                J, r = J.reshape(-1, 3), r.reshape(-1)
                with np.errstate(all="ignore"):
                    try:
                        d = -np.linalg.solve(J.T @ J, J.T @ r)
                    except np.linalg.LinAlgError:
                        d = np.full(3, np.nan)
                if np.linalg.norm(d) <= 1e-12 * (1 + np.linalg.norm(S + X)):
                    break
                Xp, cost_prev, X = X, c, X + d
        p, z = _project(Q, X)
        e = np.linalg.norm(p - uv, axis=1)
        out["node_err"][o] = e
        depth = sgn[f] * z / n3[f]
        dirs = C[f] - (S + X)
        dirs /= np.linalg.norm(dirs, axis=1, keepdims=True)
        i, j = np.triu_indices(len(o), 1)
        ang = np.degrees(np.arctan2(np.linalg.norm(np.cross(dirs[i], dirs[j]), axis=1), (dirs[i] * dirs[j]).sum(1)))
        par = float(np.nanmax(ang)) if len(ang) and not np.isnan(ang).all() else 0.0
        fl = (BEHIND if (depth <= 0).any() else 0) | (PARALLAX if par < min_parallax_deg else 0) | \
             (REPROJ if not e.max() <= max_reproj_px else 0)
        out["xyz"][t] = S + X
        out["quality"][t] = (np.sqrt((e ** 2).sum() / len(o)), e.max(), par)
        out["flags"][t] = fl
        out["maxe"][t], out["parallax"][t], out["min_depth"][t] = e.max(), par, depth.min()
    fl = out["flags"]
    out["summary"] = np.array([nt, (fl == 0).sum()] + [((fl >> b) & 1).sum() for b in range(5)] + [used_total], dtype=np.int32)
    return out


def stop_band(kps, P, offsets, nodes, ref):
    """Per track, how far from the yardstick's refined point another correct implementation may stop: the radius within which
    the cost cannot tell two points apart in float64.  Each residual is a difference of two values of ~1e3 px, so the cost
    carries a rounding error of about dC = 2 eps sum |r_i| |uv_i|; a step d changes the cost by about d^T J^T J d, so two points
    within sqrt(dC / lambda_min(J^T J)) of each other compare in either order, and the refinement's stop test ("the cost did not
    decrease") may end anywhere in that ball.  On narrow baselines (short tracks of scenes with 64 or 130 frames on a 60..120
    degree arc) this radius exceeds 1e-9 of the camera distance: two formulations of this yardstick (SVD or Gram matrix start)
    differ by up to 4e-9 there, and more refinement steps do not reduce it; the kernel stays within 0.7 of the radius.  On
    33..64-node tracks over 130 frames on a 60-degree arc the two starts still differ by up to 1.1e-9, so tracks of that
    length can pass 1e-9 only with this band.  Tests
    whose scenes have such tracks hold the refined points to max(1e-9 dist, this radius) (tests/test_gpu_geometry_limits.py).
    -> [n_tracks] (NaN where the yardstick has no point)"""
    P3 = np.asarray(P, dtype=np.float64).reshape(-1, 3, 4)
    known, C, _, _ = cameras(P)
    xy = [np.stack([k["x"], k["y"]], 1).astype(np.float64) if k.dtype.names else np.asarray(k, dtype=np.float64) for k in kps]
    offsets, nodes = np.asarray(offsets), np.asarray(nodes).reshape(-1, 2)
    eps = np.finfo(np.float64).eps
    out = np.full(len(offsets) - 1, np.nan)
    for t in np.flatnonzero(np.isfinite(ref["xyz"]).all(1)):
        nd = nodes[offsets[t]:offsets[t + 1]]
        nd = nd[known[nd[:, 0]]]
        f = nd[:, 0]
        S = C[f].mean(axis=0)
        Q = P3[f].copy()
        Q[:, :, 3] += Q[:, :, :3] @ S
        uv = np.array([xy[fr][k] for fr, k in nd])
        p, z = _project(Q, ref["xyz"][t] - S)
        J = ((Q[:, :2, :3] - p[:, :, None] * Q[:, 2:3, :3]) / z[:, None, None]).reshape(-1, 3)
        dC = 2.0 * eps * (np.abs(p - uv) * np.abs(uv)).sum()
        out[t] = np.sqrt(dC / np.linalg.eigvalsh(J.T @ J)[0])
    return out


def near_threshold(ref, min_parallax_deg, max_reproj_px, rel=1e-6):
    """Tracks whose flag decision lies within `rel` of its threshold (the tests exclude them from flag equality)."""
    def close(x, thr):
        return np.isfinite(x) & (np.abs(x - thr) <= rel * np.maximum(np.abs(thr), 1e-300))
    near = close(ref["w"], W_MIN) | close(ref["parallax"], min_parallax_deg) | (np.abs(ref["min_depth"]) <= rel)
    if np.isfinite(max_reproj_px):
        near |= close(ref["maxe"], max_reproj_px)
    return near


def truth_tracks(scene, min_len=2):
    """The true tracks of a synth.make_scene scene (every point seen in >= min_len frames), in the track graph's order:
    -> (offsets, nodes, point of each track)"""
    seen = {}
    for f, pid in enumerate(scene["point_id"]):
        for k, p in enumerate(pid):
            seen.setdefault(int(p), []).append((f, k))
    tr = sorted((sorted(v), p) for p, v in seen.items() if len(v) >= min_len)
    offsets = np.cumsum([0] + [len(t) for t, _ in tr]).astype(np.int32)
    nodes = np.array([n for t, _ in tr for n in t], dtype=np.int32).reshape(-1, 2)
    return offsets, nodes, np.array([p for _, p in tr], dtype=np.int64)


def flag_cases():
    """Purpose-built tracks, one per flag bit: -> (kps per frame [F] of [n][2] ints, P [F][12], tracks [(bit, [(frame, kp)])]).
    Every frame holds the keypoints of the cases that use it; cameras K = (1200, 960, 540)."""
    import photogrammetry_amd.synth as synth
    cams, kps, tracks = [], [], []

    def frame(P, uv):
        cams.append(np.asarray(P, dtype=np.float64).reshape(12))
        kps.append(np.asarray(uv, dtype=np.int64).reshape(-1, 2))
        return len(cams) - 1

    def proj(P, X):
        h = P[:, :3] @ X + P[:, 3]
        return np.round(h[:2] / h[2])
    X = np.array([0.1, 0.2, 0.0])
    # FEWVIEWS: a 2-view track whose second camera is NaN
    A = synth.look_at_camera([0, 0, -5], [0, 0, 0])
    tracks.append((FEWVIEWS, [(frame(A, [proj(A, X)]), 0), (frame(np.full((3, 4), np.nan), [[700, 300]]), 0)]))
    # BEHIND: the second camera looks away from the point, which projects through its back
    B = synth.look_at_camera([0.5, 0, -10], [0.5, 0, -20])
    tracks.append((BEHIND, [(frame(A, [proj(A, X)]), 0), (frame(B, [proj(B, X)]), 0)]))
    # PARALLAX: two cameras 5/1200 apart, side by side, see (1/6, 1/4, 0) at exact pixels 1 px apart: 0.048 degrees.  (Two
    # cameras with one centre give no point at all: their rays meet at the centre, or everywhere on one line.)
    P1, P2 = synth.look_at_camera([0, 0, -5], [0, 0, 0]), synth.look_at_camera([5 / 1200, 0, -5], [5 / 1200, 0, 0])
    tracks.append((PARALLAX, [(frame(P1, [[1000, 600]]), 0), (frame(P2, [[999, 600]]), 0)]))
    # REPROJ: four views of X, one of them linked to the keypoint of another point (a consistent but wrong track)
    Y = np.array([-0.6, 0.4, 0.5])
    Cs = [synth.look_at_camera([5 * np.sin(a), 0, -5 * np.cos(a)], [0, 0, 0]) for a in np.radians([-30, -10, 10, 30])]
    tracks.append((REPROJ, [(frame(Cs[0], [proj(Cs[0], X)]), 0), (frame(Cs[1], [proj(Cs[1], X)]), 0),
                            (frame(Cs[2], [proj(Cs[2], Y)]), 0), (frame(Cs[3], [proj(Cs[3], X)]), 0)]))
    # DEGENERATE: parallel rays from distinct centres (both through the principal point): the point is at infinity
    D1, D2 = synth.look_at_camera([0, 0, -5], [0, 0, 0]), synth.look_at_camera([1, 0, -5], [1, 0, 0])
    tracks.append((DEGENERATE, [(frame(D1, [[960, 540]]), 0), (frame(D2, [[960, 540]]), 0)]))
    return kps, np.array(cams), tracks
