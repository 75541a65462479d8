"""CPU test (no GPU): the triangulation yardstick of tests/triangulate_ref.py (used by tests/test_gpu_triangulate.py).
  * it equals a literal Python loop over the observations -- scalar floats, the Gram matrix's smallest eigenvector by cyclic
    Jacobi and the 3x3 normal equations by the adjugate, as the kernel does it -- on rounded keypoints, NaN cameras, a scene
    far from the origin and the purpose-built flag cases;
  * on unrounded projections it recovers the true points to 1e-9 relative.
"""
import math

import numpy as np
import pytest

import triangulate_ref as ref
from photogrammetry_amd import synth


def _cam(p):
    m = [[p[4 * r + c] for c in range(4)] for r in range(3)]
    if not all(math.isfinite(x) for x in p):
        return None
    (a, b, c), (d, e, f), (g, h, i) = (row[:3] for row in m)
    k = [[e * i - f * h, f * g - d * i, d * h - e * g], [c * h - b * i, a * i - c * g, b * g - a * h], [b * f - c * e, c * d - a * f, a * e - b * d]]
    det = a * k[0][0] + b * k[0][1] + c * k[0][2]
    if det == 0:
        return None
    C = [-(k[0][j] * m[0][3] + k[1][j] * m[1][3] + k[2][j] * m[2][3]) / det for j in range(3)]
    return m, C, (1.0 if det > 0 else -1.0), math.sqrt(g * g + h * h + i * i)


def _null_vector(G):
    A = [row[:] for row in G]
    V = [[1.0 if i == j else 0.0 for j in range(4)] for i in range(4)]
    for _ in range(8):
        for p, q in ((0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3)):
            if A[p][q] == 0:
                continue
            th = (A[q][q] - A[p][p]) / (2 * A[p][q])
            t = (1.0 if th >= 0 else -1.0) / (abs(th) + math.sqrt(th * th + 1))
            c = 1 / math.sqrt(t * t + 1)
            s = t * c
            for k in range(4):
                A[k][p], A[k][q] = c * A[k][p] - s * A[k][q], s * A[k][p] + c * A[k][q]
            for k in range(4):
                A[p][k], A[q][k] = c * A[p][k] - s * A[q][k], s * A[p][k] + c * A[q][k]
            for k in range(4):
                V[k][p], V[k][q] = c * V[k][p] - s * V[k][q], s * V[k][p] + c * V[k][q]
    col = min(range(4), key=lambda j: A[j][j])
    return [V[k][col] for k in range(4)]


def loop_triangulate(kps, P, offsets, nodes, min_par, max_e, iters):
    """-> list of (xyz, (rms, max, parallax), flags) and node errors, one scalar at a time"""
    cams = [_cam(list(map(float, p))) for p in np.asarray(P).reshape(-1, 12)]
    res, nerr = [], [float("nan")] * len(nodes)
    for t in range(len(offsets) - 1):
        obs = []
        for o in range(offsets[t], offsets[t + 1]):
            f, k = int(nodes[o][0]), int(nodes[o][1])
            if cams[f] is not None:
                obs.append((o, float(kps[f][k][0]), float(kps[f][k][1]), cams[f]))
        if len(obs) < 2:
            res.append((None, None, ref.FEWVIEWS))
            continue
        S = [sum(c[1][j] for _, _, _, c in obs) / len(obs) for j in range(3)]
        Qs = [[row[:3] + [row[3] + sum(row[j] * S[j] for j in range(3))] for row in c[0]] for _, _, _, c in obs]
        G = [[0.0] * 4 for _ in range(4)]
        for (o, u, v, c), Q in zip(obs, Qs):
            for r in ([u * Q[2][j] - Q[0][j] for j in range(4)], [v * Q[2][j] - Q[1][j] for j in range(4)]):
                n = math.sqrt(sum(x * x for x in r))
                r = [x / n for x in r]
                for i in range(4):
                    for j in range(4):
                        G[i][j] += r[i] * r[j]
        w = _null_vector(G)
        if not all(math.isfinite(x) for x in w) or abs(w[3]) <= 1e-12:
            res.append((None, None, ref.DEGENERATE))
            continue
        X = [w[j] / w[3] for j in range(3)]

        def terms(X):
            out = []
            for (o, u, v, c), Q in zip(obs, Qs):
                h = [sum(Q[r][j] * X[j] for j in range(3)) + Q[r][3] for r in range(3)]
                out.append((o, u, v, c, Q, h, h[0] / h[2], h[1] / h[2]))
            return out
        prev, cost_prev = X, 0.0
        for it in range(iters + 1 if iters > 0 else 0):
            T = terms(X)
            cost = sum((pu - u) ** 2 + (pv - v) ** 2 for _, u, v, _, _, _, pu, pv in T)
            if it > 0 and not cost < cost_prev:
                X = prev
                break
            if it == iters:
                break
            H, g = [[0.0] * 3 for _ in range(3)], [0.0] * 3
            for _, u, v, _, Q, h, pu, pv in T:
                for r, p, obsv in ((0, pu, u), (1, pv, v)):
                    J = [(Q[r][j] - p * Q[2][j]) / h[2] for j in range(3)]
                    for i in range(3):
                        g[i] += J[i] * (p - obsv)
                        for j in range(3):
                            H[i][j] += J[i] * J[j]
            d = [-x for x in np.linalg.solve(np.array(H), np.array(g))]
            Wn = math.sqrt(sum((S[j] + X[j]) ** 2 for j in range(3)))
            if math.sqrt(sum(x * x for x in d)) <= 1e-12 * (1 + Wn):
                break
            prev, cost_prev, X = X, cost, [X[j] + d[j] for j in range(3)]
        T = terms(X)
        es, behind, dirs = [], False, []
        for o, u, v, c, Q, h, pu, pv in T:
            e = math.hypot(pu - u, pv - v)
            nerr[o] = e
            es.append(e)
            behind |= c[2] * h[2] / c[3] <= 0
            a = [c[1][j] - S[j] - X[j] for j in range(3)]
            n = math.sqrt(sum(x * x for x in a))
            dirs.append([x / n for x in a])
        par = 0.0
        for i in range(len(dirs)):
            for j in range(i + 1, len(dirs)):
                dot = max(-1.0, min(1.0, sum(dirs[i][k] * dirs[j][k] for k in range(3))))
                par = max(par, math.degrees(math.acos(dot)))
        fl = (ref.BEHIND if behind else 0) | (ref.PARALLAX if par < min_par else 0) | (0 if max(es) <= max_e else ref.REPROJ)
        res.append(([S[j] + X[j] for j in range(3)], (math.sqrt(sum(e * e for e in es) / len(es)), max(es), par), fl))
    return res, nerr


def _compare(kps, P, off, nodes, min_par, max_e, iters):
    got = ref.triangulate(kps, P, off, nodes, min_par, max_e, iters)
    exp, nerr = loop_triangulate([np.stack([k["x"], k["y"]], 1) if k.dtype.names else k for k in kps], P, off, nodes, min_par,
                                 max_e, iters)
    near = ref.near_threshold(got, min_par, max_e)
    for t, (x, q, fl) in enumerate(exp):
        if not near[t]:
            assert got["flags"][t] == fl, t
        if x is None:
            assert np.isnan(got["xyz"][t]).all()
            continue
        scale = 1 + np.linalg.norm(np.asarray(x))
        assert np.abs(got["xyz"][t] - x).max() <= 1e-9 * scale, (t, got["xyz"][t], x)
        assert np.abs(got["quality"][t][:2] - q[:2]).max() <= 1e-6, t
        assert abs(got["quality"][t][2] - q[2]) <= 1e-6 * max(1.0, q[2]), t
    assert np.allclose(got["node_err"], nerr, rtol=0, atol=1e-6, equal_nan=True)
    assert (np.isnan(got["node_err"]) == np.isnan(np.asarray(nerr))).all()
    return got


@pytest.mark.parametrize("offset", [(0, 0, 0), (1e4, -5e3, 2e4)])
def test_yardstick_equals_the_literal_loop(offset):
    s = synth.make_scene(60, 7, seed=3, offset=offset)
    off, nodes, _ = ref.truth_tracks(s)
    P = s["P"].copy()
    P[4] = np.nan                       # a frame without a pose
    for iters in (0, 1, 10):
        for min_par, max_e in ((1.0, np.inf), (5.0, 0.4)):
            got = _compare(s["kps"], P, off, nodes, min_par, max_e, iters)
    assert got["summary"][7] == sum(1 for f, _ in nodes if f != 4)


def test_yardstick_flag_cases_equal_the_literal_loop():
    kps, P, tracks = ref.flag_cases()
    off = np.cumsum([0] + [len(t) for _, t in tracks])
    nodes = np.array([n for _, t in tracks for n in t])
    got = _compare(kps, P, off, nodes, 1.0, 3.0, 10)
    assert [int(f) for f in got["flags"]] == [b for b, _ in tracks]
    assert list(got["summary"]) == [5, 0, 1, 1, 1, 1, 1, 11]


@pytest.mark.parametrize("offset", [(0, 0, 0), (1e4, -5e3, 2e4)])
def test_yardstick_recovers_true_points_from_exact_projections(offset):
    s = synth.make_scene(400, 9, seed=5, offset=offset)
    off, nodes, pid = ref.truth_tracks(s)
    for iters in (0, 10):
        got = ref.triangulate(s["uv"], s["P"], off, nodes, 1.0, 1e-6, iters)
        truth = s["points"][pid]
        dist = np.linalg.norm(truth - np.asarray(offset), axis=1)
        assert (np.linalg.norm(got["xyz"] - truth, axis=1) <= 1e-9 * np.linalg.norm(truth, axis=1).clip(1.0)).all()
        assert (got["flags"] == 0).all() and got["summary"][1] == len(pid)
        assert dist.max() < 10
