"""numpy / scipy yardstick of the split track graph (include/pgx.h, "split mode": pgx_tracks_split_dev,
pgx_tracks_finish_split), shared by tests/test_tracks_split_ref.py, tests/test_gpu_tracks_split.py and tools/tracks_lab.py.

The rule: E_l = the edges pgx_tracks_dev uses at gate g_l (g_0 = max_dist, g_l = gates[l - 1]); C_l(x) = x's component in
(nodes, E_l); the level of x = the smallest l with C_l(x) consistent (at most one keypoint per frame); x's group = C_level(x);
tracks = groups of at least min_len nodes; nodes without a level are dropped (-2).  Three formulations that must agree:
  literal()     (a) scipy connected components of every E_l over ALL nodes, the level taken per node
  sequential()  (b) a plain union-find in list order, re-run at each gate over the still-unresolved nodes only
  arrays()      (c) vectorised, for the bench size, in pgx_tracks_split_dev's output layout
(a) and (b) return (tracks, track_of [F][max count], summary) like oracle.tracks_np.tracks; summary has the keys of
tracks_np plus per_level = [nodes in tracks of level l for l = 0 .. n_gates].  summary16() turns it into d_summary [16].
"""
import numpy as np

INT_MAX = 2**31 - 1
KEYS = ("n_tracks", "n_nodes", "dropped", "dropped_nodes", "edges", "longest", "largest_dropped")


def edges(counts, pair_list, lists, max_dist):
    """The gated edges as ((fa, k1), (fb, k2), dist), in list order: the filters of oracle.tracks_np.edges."""
    out = []
    for (a, b), rows in zip(pair_list, lists):
        rows = np.asarray(rows).reshape(-1, 3)[:int(counts[a])]
        for k1, k2, d in rows.tolist():
            if d > max_dist or d == INT_MAX or k1 < 0 or k2 < 0 or k1 >= counts[a] or k2 >= counts[b]:
                continue
            out.append(((int(a), int(k1)), (int(b), int(k2)), int(d)))
    return out


def check_gates(max_dist, gates):
    g = [int(x) for x in gates]
    assert len(g) <= 7 and all(x >= 0 for x in g) and all(x < y for x, y in zip(g, [max_dist] + g)), (max_dist, g)
    return [int(max_dist)] + g


def summary16(s):
    return [s[k] for k in KEYS] + [0] + list(s["per_level"]) + [0] * (8 - len(s["per_level"]))


def _finish(counts, groups, min_len, n_levels):
    """groups: list of (level or -1, node list), every node exactly once -> (tracks, track_of, summary)."""
    F = len(counts)
    stride = max([int(c) for c in counts] + [1])
    track_of = -np.ones((F, stride), dtype=np.int32)
    kept, per_level = [], [0] * n_levels
    dropped = dropped_nodes = largest_dropped = 0
    for lv, g in groups:
        g = sorted(g)
        if lv < 0:
            dropped += 1
            dropped_nodes += len(g)
            largest_dropped = max(largest_dropped, len(g))
            for f, k in g:
                track_of[f, k] = -2
        elif len(g) >= min_len:
            kept.append((g, lv))
    kept.sort()
    for t, (g, lv) in enumerate(kept):
        per_level[lv] += len(g)
        for f, k in g:
            track_of[f, k] = t
    summary = {"n_tracks": len(kept), "n_nodes": sum(len(g) for g, _ in kept), "dropped": dropped,
               "dropped_nodes": dropped_nodes, "longest": max([len(g) for g, _ in kept] + [0]),
               "largest_dropped": largest_dropped, "per_level": per_level}
    return [g for g, _ in kept], track_of, summary


def _consistent(nodes):
    frames = [f for f, _ in nodes]
    return len(set(frames)) == len(frames)


def literal(counts, pair_list, lists, max_dist, gates, min_len=2):
    """(a): the definition as written -- components of every E_l over all nodes, nested by construction."""
    from scipy.sparse import coo_matrix
    from scipy.sparse.csgraph import connected_components
    g = check_gates(max_dist, gates)
    counts = [int(c) for c in counts]
    base = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    n = int(base[-1])
    es = edges(counts, pair_list, lists, max_dist)
    nodes = [(f, k) for f, c in enumerate(counts) for k in range(c)]
    level = [-1] * n
    group = [None] * n
    for lv, gate in enumerate(g):
        sel = [(u, v) for u, v, d in es if d <= gate]
        u = np.array([base[f] + k for (f, k), _ in sel], dtype=np.int64)
        v = np.array([base[f] + k for _, (f, k) in sel], dtype=np.int64)
        lab = connected_components(coo_matrix((np.ones(len(sel), dtype=np.int8), (u, v)), shape=(n, n)), directed=False)[1] \
            if n else np.zeros(0, dtype=np.int64)
        comps = {}
        for i in range(n):
            comps.setdefault(int(lab[i]), []).append(i)
        for members in comps.values():
            if _consistent([nodes[i] for i in members]):
                for i in members:
                    if level[i] < 0:
                        level[i] = lv
                        group[i] = (lv, members[0])
    # unresolved nodes: grouped by their component at the last gate (lab of the last loop)
    groups = {}
    for i in range(n):
        key = group[i] if level[i] >= 0 else (-1, int(lab[i]))
        groups.setdefault(key, []).append(nodes[i])
    tr, tof, s = _finish(counts, [(k[0], v) for k, v in groups.items()], min_len, len(g))
    s["edges"] = len(es)
    return tr, tof, s


def sequential(counts, pair_list, lists, max_dist, gates, min_len=2):
    """(b): union-find in list order at g_0, then again at each tighter gate over the still-unresolved nodes only."""
    g = check_gates(max_dist, gates)
    counts = [int(c) for c in counts]
    es = edges(counts, pair_list, lists, max_dist)
    active = {(f, k) for f, c in enumerate(counts) for k in range(c)}
    groups = []
    for lv, gate in enumerate(g):
        parent = {x: x for x in active}

        def find(x):
            while parent[x] != x:
                parent[x] = parent[parent[x]]
                x = parent[x]
            return x

        for u, v, d in es:
            if d <= gate and u in active and v in active:
                ru, rv = find(u), find(v)
                if ru != rv:
                    parent[rv] = ru
        comps = {}
        for x in sorted(active):
            comps.setdefault(find(x), []).append(x)
        active = set()
        for members in comps.values():
            if _consistent(members):
                groups.append((lv, members))
            elif lv == len(g) - 1:
                groups.append((-1, members))
            else:
                active.update(members)
    tr, tof, s = _finish(counts, groups, min_len, len(g))
    s["edges"] = len(es)
    return tr, tof, s


def arrays(counts, pair_list, matches, stride, max_dist, gates, min_len=2):
    """(c): vectorised, in pgx_tracks_split_dev's layout.  counts [F]; pair_list [M][2]; matches [M][stride][3] int32.
    -> (offsets [n_tracks + 1], nodes [n_nodes][2], track_of [F][stride], summary dict)."""
    from scipy.sparse import coo_matrix
    from scipy.sparse.csgraph import connected_components
    g = check_gates(max_dist, gates)
    counts = np.asarray(counts, dtype=np.int64)
    pl = np.asarray(pair_list, dtype=np.int64).reshape(-1, 2)
    m = np.asarray(matches).reshape(len(pl), stride, 3)
    F = len(counts)
    N = F * stride
    ca, cb = counts[pl[:, 0]][:, None], counts[pl[:, 1]][:, None]
    e = np.arange(stride)[None, :]
    k1, k2, d = m[..., 0].astype(np.int64), m[..., 1].astype(np.int64), m[..., 2].astype(np.int64)
    ok = (e < ca) & (d <= max_dist) & (d != INT_MAX) & (k1 >= 0) & (k2 >= 0) & (k1 < ca) & (k2 < cb)
    u = (pl[:, 0][:, None] * stride + k1)[ok]
    v = (pl[:, 1][:, None] * stride + k2)[ok]
    d = d[ok]
    valid = (np.arange(stride)[None, :] < counts[:, None]).reshape(-1)
    active = valid.copy()
    level = np.full(N, -1, dtype=np.int64)
    root = np.arange(N, dtype=np.int64)          # final group name (its smallest node) of every valid node
    for lv, gate in enumerate(g):
        sel = (d <= gate) & active[u]
        _, lab = connected_components(coo_matrix((np.ones(int(sel.sum()), dtype=np.int8), (u[sel], v[sel])), shape=(N, N)),
                                      directed=False)
        ids = np.nonzero(active)[0]
        if len(ids) == 0:
            break
        first = np.full(lab.max() + 1, N, dtype=np.int64)
        np.minimum.at(first, lab[ids], ids)
        r = first[lab[ids]]
        key = r * F + ids // stride
        uniq, cnt = np.unique(key, return_counts=True)
        bad = np.zeros(N, dtype=bool)
        bad[np.unique(uniq[cnt > 1] // F)] = True
        root[ids] = r
        res = ids[~bad[r]]
        level[res] = lv
        active[res] = False
    vids = np.nonzero(valid)[0]
    size = np.bincount(root[vids], minlength=N)
    roots = np.nonzero(size > 0)[0]
    dropped_roots = roots[level[roots] < 0]
    kept_roots = roots[(level[roots] >= 0) & (size[roots] >= max(1, min_len))]
    tidx = np.full(N, -1, dtype=np.int64)
    tidx[kept_roots] = np.arange(len(kept_roots))
    offsets = np.concatenate([[0], np.cumsum(size[kept_roots])]).astype(np.int32)
    t_of_node = tidx[root[vids]]
    keep = t_of_node >= 0
    o = np.lexsort((vids[keep], t_of_node[keep]))
    kn = vids[keep][o]
    nodes = np.stack([kn // stride, kn % stride], axis=1).astype(np.int32)
    track_of = np.full(N, -1, dtype=np.int32)
    track_of[vids] = np.where(level[vids] < 0, -2, t_of_node).astype(np.int32)
    per_level = [int(size[kept_roots][level[kept_roots] == lv].sum()) for lv in range(len(g))]
    summary = {"n_tracks": int(len(kept_roots)), "n_nodes": int(offsets[-1]), "dropped": int(len(dropped_roots)),
               "dropped_nodes": int(size[dropped_roots].sum()), "edges": int(ok.sum()),
               "longest": int(size[kept_roots].max()) if len(kept_roots) else 0,
               "largest_dropped": int(size[dropped_roots].max()) if len(dropped_roots) else 0, "per_level": per_level}
    return offsets, nodes, track_of.reshape(F, stride), summary


def hand_built():
    """8 frames x 2 keypoints.  Tracks A = (f, 0) and B = (f, 1) over frames 0..3 (links at distance 5) are joined by one edge
    at distance 60: one inconsistent component at max_dist = 64, two tracks at the gate 40.  (4, 0) and (4, 1) both link to
    (5, 0) at distances 2 and 3: inconsistent at every gate (-2).  (6, 0) - (7, 0) at 5 and (6, 1) - (7, 0) at 50: at 40 the
    pair stays a track and (6, 1) splits off alone (-1).  -> (counts, pair_list, lists, stride, max_dist, gates, expected)."""
    counts = np.full(8, 2, dtype=np.int32)
    rows = {(0, 1): [[0, 0, 5], [1, 1, 5]], (1, 2): [[0, 0, 5], [1, 1, 5]], (2, 3): [[0, 0, 5], [1, 1, 5]],
            (0, 3): [[0, 0, INT_MAX], [1, 0, 60]], (4, 5): [[0, 0, 2], [1, 0, 3]], (6, 7): [[0, 0, 5], [1, 0, 50]]}
    pl = list(rows)
    m = np.array([rows[p] for p in pl], dtype=np.int32)
    exp = [[(0, 0), (1, 0), (2, 0), (3, 0)], [(0, 1), (1, 1), (2, 1), (3, 1)], [(6, 0), (7, 0)]]
    return counts, pl, m, 2, 64, [40], exp
