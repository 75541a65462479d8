"""Case builders for the track graph (csrc/k_tracks.hip: pgx_tracks_dev, pgx_tracks_split_dev) past its scan, grid-stride, chunk
and table limits, shared by tests/test_tracks_limits_cases.py (CPU: every case reaches the path it names) and
tests/test_gpu_tracks_limits.py (GPU: exact comparison with the oracles).  A plain helper module without a GPU: no test
module imports another.

The launch facts of k_tracks.hip that the cases rest on, stated once (tests/test_tracks_limits_cases.py holds them to the
source text):"""
import functools

import numpy as np

import tracks_split_ref
from oracle import tracks_np

INT_MAX = 2**31 - 1
TRK_NT = 256                    # threads per workgroup of the per-entry / per-node kernels: one chunk of a list or of a frame
SCAN_NT = 256                   # threads of the scan kernels ...
SCAN_ITEMS = 1024               # ... and node ids per scan block: k_trk_scan_sums takes SCAN_NT blocks per pass of its b0 loop
TRK_UNION_GRID = TRKS_UNION_GRID = 256   # workgroups of k_trk_union / k_trks_union: more work items are taken grid-stride
FL_SLOTS = 512                  # LDS table of trk_flatten, per workgroup
TRK_INIT_GRID_MAX = 4096        # cap of trk_init_grid: k_trk_init, k_trks_prep and k_trks_reset walk grid-stride beyond it
HASH_MUL = 2654435761           # trk_prio: a bijection on 32 bits

SCAN_PASS = SCAN_NT * SCAN_ITEMS            # node ids per pass of k_trk_scan_sums: 262 144
INIT_PASS = TRK_INIT_GRID_MAX * TRK_NT      # nodes / table entries per pass of the grid-stride kernels: 1 048 576


def table_size(stride):
    """T: entries of a frame's hash table = the smallest power of two >= max(64, 2 * stride)"""
    T = 64
    while T < 2 * stride:
        T <<= 1
    return T


def prio(ids):
    """(id * 2654435761) mod 2^32.  The larger hashed id always hooks under the smaller, so a component's root is its node
    with the smallest prio, id = frame_number * stride + keypoint."""
    return (np.asarray(ids).astype(np.uint64) * np.uint64(HASH_MUL)) & np.uint64(0xFFFFFFFF)


def lds_home(r):
    """home slot of root r in the 512-slot LDS table of trk_flatten"""
    return ((prio(r) >> np.uint64(9)) & np.uint64(FL_SLOTS - 1)).astype(np.int64)


def table_home(r, T):
    """home slot of root r in a frame's table of T entries"""
    return ((prio(r) >> np.uint64(7)) & np.uint64(T - 1)).astype(np.int64)


def wraps(homes, size):
    """From the home slots alone: an open-addressing table of `size` slots must probe from slot size - 1 on to slot 0 when, for
    some slot j, more keys have their home in [j, size) than the size - j slots there (whatever the order of the inserts)."""
    cnt = np.bincount(np.asarray(homes, dtype=np.int64), minlength=size)
    tail = np.cumsum(cnt[::-1])[::-1]
    return bool((tail > size - np.arange(size)).any())


def chunks_of(stride):
    return (stride + TRK_NT - 1) // TRK_NT


def n_union_items(M, stride):
    """work items of k_trk_union / k_trks_union: (image pair, chunk of its list)"""
    return M * chunks_of(stride)


class Case:
    """What a builder returns; unpacks into its four parts.
      dev    the slot-indexed device inputs: counts [F] by slot, pl [M][2] in slots, m [M][stride][3], frame_ids [F] or None
             (identity), n_frames, stride
      ora    the frame-indexed oracle inputs: counts [n_frames] dense, pl in frame numbers (pairs that name a slot outside the
             graph left out), m (their lists)
      gates  (max_dist, [tighter gates])
      reach  facts about the shape, computed on the host
    oracle(split, min_len) is computed once per case and handed out read-only."""

    def __init__(self, dev, ora, gates, reach):
        self.dev, self.ora, self.gates, self.reach = dev, ora, gates, reach
        self._oracle = {}

    def __iter__(self):
        return iter((self.dev, self.ora, self.gates, self.reach))

    def oracle(self, split, min_len=2):
        """-> (offsets, nodes [n][2], track_of [n_frames][stride], summary as the device writes it: 8 ints, or 16 in split mode)"""
        key = (bool(split), int(min_len))
        if key not in self._oracle:
            o, stride, (max_dist, gates) = self.ora, self.dev["stride"], self.gates
            if split:
                off, nodes, tof, s = tracks_split_ref.arrays(o["counts"], o["pl"], o["m"], stride, max_dist, gates, min_len)
                summ = [int(x) for x in tracks_split_ref.summary16(s)]
            else:
                off, nodes, tof, s = tracks_np.tracks_arrays(o["counts"], o["pl"], o["m"], stride, max_dist, min_len)
                summ = [int(s[k]) for k in tracks_split_ref.KEYS] + [0]
            for a in (off, nodes, tof):
                a.setflags(write=False)
            self._oracle[key] = (off, nodes, tof, summ)
        return self._oracle[key]


def make_case(n_frames, stride, counts, pl, m, frame_ids, max_dist, gates, reach=None):
    """The oracle's dense inputs from the sparse slots, and the shape facts every case has."""
    counts = np.asarray(counts, dtype=np.int32)
    pl = np.asarray(pl, dtype=np.int32).reshape(-1, 2)
    m = np.ascontiguousarray(m, dtype=np.int32).reshape(len(pl), stride, 3)
    F = len(counts)
    ids = np.arange(F, dtype=np.int64) if frame_ids is None else np.asarray(frame_ids, dtype=np.int64)
    assert len(ids) == F and (frame_ids is not None or n_frames == F)
    named = ids >= 0
    assert (ids[named] < n_frames).all() and len(set(ids[named].tolist())) == int(named.sum())   # inside the contract
    assert n_frames * stride <= 1 << 30 and (counts >= 0).all()
    dense = np.zeros(n_frames, dtype=np.int32)
    dense[ids[named]] = np.minimum(counts[named], stride)
    ok = ((pl >= 0) & (pl < F)).all(axis=1)
    ok[ok] = (ids[pl[ok]] >= 0).all(axis=1)
    ora = dict(counts=dense, pl=ids[pl[ok]].astype(np.int32).reshape(-1, 2), m=m[ok])
    dev = dict(counts=counts, pl=pl, m=m, frame_ids=None if frame_ids is None else ids.astype(np.int32), n_frames=n_frames,
               stride=stride)
    N, T = n_frames * stride, table_size(stride)
    facts = dict(N=N, nb=(N + SCAN_ITEMS - 1) // SCAN_ITEMS, T=T, table_entries=n_frames * T, M=len(pl),
                 union_items=n_union_items(len(pl), stride))
    facts.update(reach or {})
    return Case(dev, ora, (int(max_dist), [int(g) for g in gates]), facts)


def permuted(case, seed):
    """The same case with its image pairs in another order: the result must not change."""
    d = dict(case.dev)
    o = np.random.default_rng(seed).permutation(len(d["pl"]))
    d["pl"], d["m"] = d["pl"][o], np.ascontiguousarray(d["m"][o])
    c = Case(d, case.ora, case.gates, case.reach)
    c._oracle = case._oracle
    return c


def as_lists(offsets, nodes):
    return [[(int(f), int(k)) for f, k in nodes[offsets[t]:offsets[t + 1]]] for t in range(len(offsets) - 1)]


def node_ids(case, nodes):
    return nodes[:, 0].astype(np.int64) * case.dev["stride"] + nodes[:, 1]


def first_ids(case, split, min_len=2):
    """node id of every kept track's first node"""
    off, nodes, _, _ = case.oracle(split, min_len)
    return node_ids(case, nodes)[off[:-1]]


def late_tracks_beyond(case, boundary, min_len=2):
    """Tracks of the split oracle that lie wholly at node ids >= boundary (a track's first node is its smallest) and were
    resolved at a level >= 1: their nodes are dropped (-2) by the plain graph at max_dist.  -> their number"""
    off, nodes, _, s = case.oracle(True, min_len)
    tof0 = case.oracle(False, min_len)[2].reshape(-1)
    nid = node_ids(case, nodes)
    first = nid[off[:-1]]
    late = tof0[first] == -2
    assert sum(s[9:]) == int(np.diff(off)[late].sum())        # per_level[1:] counts exactly these tracks' nodes
    return int((late & (first >= boundary)).sum())


def level0_roots(case):
    """root[id] of every node at max_dist as the device's union-find leaves it (the component's node with the smallest prio);
    -1 beyond a frame's count.  The gating is tracks_np.tracks_arrays'."""
    from scipy.sparse import coo_matrix
    from scipy.sparse.csgraph import connected_components
    o, stride, (max_dist, _) = case.ora, case.dev["stride"], case.gates
    counts, pl, m = o["counts"].astype(np.int64), o["pl"].astype(np.int64), o["m"].astype(np.int64)
    N = len(counts) * stride
    ca, cb = counts[pl[:, 0]][:, None], counts[pl[:, 1]][:, None]
    k1, k2, d = m[..., 0], m[..., 1], m[..., 2]
    ok = (np.arange(stride)[None, :] < ca) & (d <= max_dist) & (d != INT_MAX) & (k1 >= 0) & (k2 >= 0) & (k1 < ca) & (k2 < cb)
    u, v = (pl[:, 0][:, None] * stride + k1)[ok], (pl[:, 1][:, None] * stride + k2)[ok]
    _, lab = connected_components(coo_matrix((np.ones(len(u), dtype=np.int8), (u, v)), shape=(N, N)), directed=False)
    ids = np.flatnonzero((np.arange(stride)[None, :] < counts[:, None]).reshape(-1))
    o = np.lexsort((prio(ids), lab[ids]))
    head = np.ones(len(o), dtype=bool)
    head[1:] = lab[ids][o][1:] != lab[ids][o][:-1]
    top = np.full(lab.max() + 1, -1, dtype=np.int64)
    top[lab[ids][o][head]] = ids[o][head]
    root = np.full(N, -1, dtype=np.int64)
    root[ids] = top[lab[ids]]
    return root


def wrapping_tables(case):
    """-> (frames whose table wraps at level 0, (frame, chunk) workgroups whose LDS table wraps): the keys are the distinct
    roots of the frame's / the chunk's nodes, whichever frame the root itself lies in"""
    stride, T = case.dev["stride"], case.reach["T"]
    root = level0_roots(case).reshape(-1, stride)
    glob, lds = [], []
    for f in np.flatnonzero(case.ora["counts"]):
        keys = np.unique(root[f][root[f] >= 0])
        if wraps(table_home(keys, T), T):
            glob.append(int(f))
        for ch in range(chunks_of(stride)):
            r = root[f, ch * TRK_NT:(ch + 1) * TRK_NT]
            if wraps(lds_home(np.unique(r[r >= 0])), FL_SLOTS):
                lds.append((int(f), ch))
    return glob, lds


def tail_lists(M, stride):
    m = np.zeros((M, stride, 3), dtype=np.int32)
    m[..., 2] = INT_MAX
    return m


def place_rows(rng, m, p, rows, n):
    """rows [(k1, k2, dist)] at random distinct positions among the first n entries of list p"""
    assert len(rows) <= n, (p, len(rows), n)
    if rows:
        m[p, np.sort(rng.choice(n, len(rows), replace=False))] = np.asarray(rows, dtype=np.int32)[rng.permutation(len(rows))]


@functools.lru_cache(maxsize=None)
def sparse_frames(n_frames, stride, frames, seed, max_dist=5, gates=(2, 0), dmax=60, dense=False):
    """A handful of slots naming frames spread over n_frames * stride node ids.  len(frames) slots plus one -1 padding slot in
    shuffled slot order (dense: F = n_frames slots, no frame ids, every other count 0).  Every pair a < b of the named frames
    has a random list as in geom_gpu.random_case (k1, k2 < stride, dist < dmax, one row in ten the (0, 0, INT_MAX) tail), the
    pairs in shuffled order; one more pair names the padding slot and carries perfect rows, which must not count."""
    rng = np.random.default_rng(seed)
    frames = list(frames)
    nfr = len(frames)
    if dense:
        F, ids, slot = n_frames, None, {f: f for f in frames}
        counts = np.zeros(F, dtype=np.int32)
    else:
        F = nfr + 1
        order = rng.permutation(F)
        slot = {f: int(order[i]) for i, f in enumerate(frames)}
        ids = np.full(F, -1, dtype=np.int32)
        counts = np.full(F, stride, dtype=np.int32)          # the padding slot's count is garbage and must not matter
        for f in frames:
            ids[slot[f]] = f
        pad = int(order[-1])
    for f in frames:
        counts[slot[f]] = rng.integers((stride + 1) // 2, stride + 1)
    pl = [(slot[a], slot[b]) for i, a in enumerate(frames) for b in frames[i + 1:]]
    pl = [pl[i] for i in rng.permutation(len(pl))]
    m = np.zeros((len(pl), stride, 3), dtype=np.int32)
    m[..., 0] = rng.integers(0, stride, m.shape[:2])
    m[..., 1] = rng.integers(0, stride, m.shape[:2])
    m[..., 2] = rng.integers(0, dmax, m.shape[:2])
    m[rng.random(m.shape[:2]) < 0.1] = [0, 0, INT_MAX]
    if not dense:
        at = int(rng.integers(0, len(pl) + 1))
        pl.insert(at, (slot[frames[-1]], pad))
        extra = np.zeros((1, stride, 3), dtype=np.int32)
        extra[0, :, 0] = extra[0, :, 1] = np.arange(stride)
        m = np.concatenate([m[:at], extra, m[at:]])
    return make_case(n_frames, stride, counts, pl, m, ids, max_dist, gates, dict(frames=tuple(frames)))


HARD, SOFT = 3, 30          # distances of the hand-placed edges: HARD passes every gate, SOFT only max_dist
CONFLICT_GATES = (50, (20, 5))


def conflict_rows(k, k2, j, soft):
    """{(a, k), (a, k2), (b, j)}: two keypoints of frame a in one component; soft: the second joins only at max_dist"""
    return [(k, j, HARD), (k2, j, SOFT if soft else HARD)]


@functools.lru_cache(maxsize=None)
def conflicts(stride):
    """Hand-placed three-node components {(a, k), (a, k'), (b, j)} with k, k' (i) in one wave, (ii) in one chunk but different
    waves, (iii) in different chunks -- there the frame's hash table is the only witness -- and on a chunk edge (255 | 256, and
    0 | stride - 1), each once joined at every gate ("hard": dropped in both modes, flagged again at every level) and once
    through an edge that only max_dist lets in ("soft": dropped by the plain graph, a two-node track and a single node at
    level 1 of the split graph).  Consistent neighbours stand beside them.  8 frames with counts stride, stride, 0, 1, 255, 256,
    257, stride: the chunk-edge counts carry chains (4, e) - (5, e) - (6, e), and the single node of frame 6's second chunk,
    (6, 256), conflicts with (6, 0) through frame 3's only keypoint."""
    assert stride >= 512
    rng = np.random.default_rng(stride)
    counts = np.array([stride, stride, 0, 1, 255, 256, 257, stride], dtype=np.int32)
    forms = {"wave": (5, 40), "chunk": (3, 200), "chunks": (10, 300), "edge": (255, 256), "ends": (0, stride - 1)}
    rows = {p: [] for p in [(0, 1), (1, 7), (0, 7), (7, 0), (4, 5), (5, 6), (6, 3), (3, 0), (2, 0), (0, 2)]}
    hard, soft, kept = {}, {}, []
    for i, (name, (k, k2)) in enumerate(forms.items()):
        j = 100 + 2 * i
        rows[(0, 1)] += conflict_rows(k, k2, j, False)
        hard[name] = [(0, k), (0, k2), (1, j)]
        ks, k2s = (k + 1, k2 + 1) if name != "ends" else (1, stride - 2)
        if name == "edge":
            ks, k2s = 254, 257
        rows[(0, 1)] += conflict_rows(ks, k2s, j + 1, True)
        soft[name] = [(0, ks), (0, k2s), (1, j + 1)]
    # consistent neighbours of the conflicts' keypoints: two-node tracks, one of them joined by a SOFT edge alone, a three-node track
    for k, j, d in ((42, 20, HARD), (202, 21, HARD), (258, 23, SOFT), (302, 22, HARD)):
        rows[(0, 1)].append((k, j, d))
        kept.append([(0, k), (1, j)])
    rows[(1, 7)].append((22, 302, HARD))
    kept[-1].append((7, 302))
    # the hard (iii) component grows a node in a third frame
    rows[(1, 7)].append((104, 100, HARD))
    hard["chunks"].append((7, 100))
    # a conflict closed through another frame and two different lists: (0, 50) - (7, 60) - (0, 400)
    rows[(0, 7)].append((50, 60, HARD))
    rows[(7, 0)].append((60, 400, HARD))
    hard["path"] = [(0, 50), (0, 400), (7, 60)]
    # chunk-edge counts: chains over frames 4 (255), 5 (256) and 6 (257 keypoints)
    rows[(4, 5)] = [(e, e, HARD) for e in range(255)]
    rows[(5, 6)] = [(e, e, HARD) for e in range(256)]
    rows[(6, 3)] = [(0, 0, HARD), (256, 0, SOFT)]
    rows[(3, 0)] = [(0, 500, HARD)]
    soft["count_edge"] = [(6, 0), (6, 256), (3, 0), (0, 500), (4, 0), (5, 0)]
    pl = list(rows)
    m = tail_lists(len(pl), stride)
    for p, (a, b) in enumerate(pl):
        place_rows(rng, m, p, rows[(a, b)], int(counts[a]))
    m[pl.index((3, 0)), 1] = [0, 501, 0]                      # a stale row beyond frame 3's count of 1
    for p in (pl.index((2, 0)), pl.index((0, 2))):           # frame 2 has no keypoints: perfect rows that never link
        m[p, :, 0] = m[p, :, 1] = np.arange(stride)
        m[p, :, 2] = 0
    o = rng.permutation(len(pl))
    return make_case(8, stride, counts, [pl[i] for i in o], m[o], None, *CONFLICT_GATES,
                     dict(hard=hard, soft=soft, kept=kept, forms=forms))


def conflict_block(a, b, c, stride, second_chunk):
    """A few of the conflicts' components between frames a, b (and c): rows by pair, for table_wrap"""
    rows = {(a, b): conflict_rows(1, 20, 3, False) + conflict_rows(2, 21, 4, True) + [(5, 5, HARD), (6, 6, HARD)],
            (b, a): conflict_rows(10, 25, 12, False) + conflict_rows(11, 26, 13, True),
            (b, c): [(6, 6, HARD)],
            (c, a): conflict_rows(1, 18, 27, False) + conflict_rows(2, 19, 28, True)}
    if stride > 64:
        rows[(a, b)] += conflict_rows(3, 200, 7, False) + conflict_rows(8, 201, 9, True)
    if second_chunk:
        rows[(a, b)] += conflict_rows(14, stride - 10, 15, False) + conflict_rows(16, stride - 9, 17, True)
    return rows


@functools.lru_cache(maxsize=None)
def table_wrap(kind, stride=None, n_wrap=6, search=64):
    """Frames of single nodes at min_len = 1 (every node is a track: a false flag cannot hide) whose hash table's probe sequence
    wraps from its last slot to slot 0.  kind "global": the per-frame table, stride 32 (T = 64), full counts.  kind "lds": the
    512-slot table of a frame's first 256 keypoints, stride 256 or 300.  The first n_wrap wrapping frame numbers below
    `search` are found here from the home slots of the single nodes; two frames that do not wrap and a padding slot stand
    beside them.  A few of the conflicts' components then link the wrapping frames in threes, so that flagged and unflagged
    roots probe past each other (reach: which tables still wrap with those components' roots, by wrapping_tables)."""
    stride = stride or {"global": 32, "lds": 256}[kind]
    T = table_size(stride)
    first = min(stride, TRK_NT)

    def single_wrap(f):
        ids = f * stride + np.arange(first)
        return wraps(table_home(f * stride + np.arange(stride), T), T) if kind == "global" else wraps(lds_home(ids), FL_SLOTS)

    found = [f for f in range(search) if single_wrap(f)]
    wrap, plain = found[:n_wrap], [f for f in range(search) if f not in found][:2]
    assert len(wrap) == n_wrap, found
    rng = np.random.default_rng(stride)
    frames = wrap + plain
    n_frames = max(frames) + 1
    F = len(frames) + 1
    order = rng.permutation(F)
    slot = {f: int(order[i]) for i, f in enumerate(frames)}
    ids = np.full(F, -1, dtype=np.int32)
    for f in frames:
        ids[slot[f]] = f
    counts = np.full(F, stride, dtype=np.int32)
    rows = {}
    for i in range(0, n_wrap - 2, 3):
        rows.update(conflict_block(wrap[i], wrap[i + 1], wrap[i + 2], stride, stride > TRK_NT))
    rows[(wrap[-1], plain[0])] = [(7, 7, HARD)]
    pl = list(rows)
    m = tail_lists(len(pl), stride)
    for p, key in enumerate(pl):
        place_rows(rng, m, p, rows[key], stride)
    o = rng.permutation(len(pl))
    return make_case(n_frames, stride, counts, [(slot[pl[i][0]], slot[pl[i][1]]) for i in o], m[o], ids, *CONFLICT_GATES,
                     dict(kind=kind, single_wrap=tuple(found), wrap=tuple(wrap), plain=tuple(plain)))


@functools.lru_cache(maxsize=None)
def long_tracks(n_frames=300, stride=8, n_long=150, seed=11):
    """Tracks with one node in every frame: track t sits at keypoint perm_f[t] of frame f.  Consecutive-frame edges (in either
    direction) plus n_long random long-range pairs with edges of the same tracks, lists and pairs shuffled.  Tracks 0 .. 4 are
    whole; track 5 misses a fifth of the frames (its gaps bridged by pairs of their own); tracks 6 and 7 are joined by one SOFT
    edge into a component with two keypoints in every frame: dropped by the plain graph, two tracks of n_frames nodes at level
    1 of the split graph."""
    assert stride >= 8
    rng = np.random.default_rng(seed)
    perm = np.stack([rng.permutation(stride) for _ in range(n_frames)])
    present = np.ones((n_frames, 8), dtype=bool)
    present[rng.choice(np.arange(1, n_frames - 1), n_frames // 5, replace=False), 5] = False
    pairs = [(f, f + 1) for f in range(n_frames - 1)]
    pairs += [tuple(int(x) for x in rng.choice(n_frames, 2, replace=False)) for _ in range(n_long)]
    here = np.flatnonzero(present[:, 5])
    bridges = [(int(p), int(q)) for p, q in zip(here[:-1], here[1:]) if q > p + 1]
    pl, rowsets = [], []
    for i, (a, b) in enumerate(pairs + bridges):
        if rng.random() < 0.5:
            a, b = b, a
        ts = [t for t in range(8) if present[a, t] and present[b, t]]
        if len(pairs) <= i:
            ts = [5]
        elif i >= n_frames - 1:
            ts = [t for t in ts if rng.random() < 0.5]
        pl.append((a, b))
        rowsets.append([(perm[a, t], perm[b, t], HARD) for t in ts])
    pl.append((n_frames // 3, 2 * n_frames // 3))
    rowsets.append([(perm[n_frames // 3, 6], perm[2 * n_frames // 3, 7], SOFT)])
    m = tail_lists(len(pl), stride)
    for p, rows in enumerate(rowsets):
        place_rows(rng, m, p, rows, stride)
    o = rng.permutation(len(pl))
    return make_case(n_frames, stride, np.full(n_frames, stride, dtype=np.int32), [pl[i] for i in o], m[o], None, 50, (20,),
                     dict(gap_track_len=int(present[:, 5].sum())))


@functools.lru_cache(maxsize=None)
def union_items(M, stride, F=24, seed=5):
    """M image pairs = M * ceil(stride / 256) work items for the 256 workgroups of k_trk_union / k_trks_union, random lists.
    The LAST work item -- the last chunk of the last pair's list -- carries edges that decide tracks: (a, k) - (b, k) at distance
    0 for every k of that chunk (reach: `last_item`, the rows' range)."""
    assert M <= F * (F - 1)
    rng = np.random.default_rng(seed + M)
    pl = [(a, b) for a in range(F) for b in range(F) if a != b]
    pl = [pl[i] for i in rng.permutation(len(pl))[:M]]
    counts = rng.integers((stride + 1) // 2, stride + 1, F).astype(np.int32)
    counts[list(pl[-1])] = stride
    m = np.zeros((M, stride, 3), dtype=np.int32)
    m[..., 0] = rng.integers(0, stride, m.shape[:2])
    m[..., 1] = rng.integers(0, stride, m.shape[:2])
    m[..., 2] = rng.integers(0, 60, m.shape[:2])
    m[rng.random(m.shape[:2]) < 0.1] = [0, 0, INT_MAX]
    lo = (chunks_of(stride) - 1) * TRK_NT
    m[-1, lo:, 0] = m[-1, lo:, 1] = np.arange(lo, stride)
    m[-1, lo:, 2] = 0
    return make_case(F, stride, counts, pl, m, None, 3, (1,), dict(last_item=(lo, stride)))


def without_rows(case, p, lo, hi):
    """The oracle inputs of a dense case with rows [lo, hi) of list p turned into tail entries -> a case of its own"""
    d = case.dev
    assert d["frame_ids"] is None
    m = d["m"].copy()
    m[p, lo:hi] = [0, 0, INT_MAX]
    return make_case(d["n_frames"], d["stride"], d["counts"], d["pl"], m, None, *case.gates)


# The shapes of tests/test_gpu_tracks_limits.py, by the limit they cross (sparse_frames arguments; the second entry of each is
# the different case that runs between the two calls of the first)
SCAN_CARRY = {
    "260": dict(n_frames=260, stride=1024, frames=(0, 255, 256, 257, 258, 259), seed=1),
    "260-dense": dict(n_frames=260, stride=1024, frames=(0, 255, 256, 257, 258, 259), seed=2, dense=True),
    "514": dict(n_frames=514, stride=1024, frames=(0, 255, 256, 511, 512, 513), seed=3),
}
NODE_PASSES = dict(n_frames=1030, stride=1024, frames=(0, 1, 1023, 1024, 1025, 1029), seed=4)
# 24 nodes at most: seed, dmax and gates chosen so that the ORACLE keeps tracks on both sides of frame 16384 and resolves one
# beyond it at level 1 (tests/test_tracks_limits_cases.py asserts it)
TABLE_PASSES = dict(n_frames=16500, stride=4, frames=(0, 7, 16383, 16384, 16385, 16499), seed=57, max_dist=4, gates=(2, 0), dmax=8)
TABLE_PASSES_SEEDS = (57, 42, 47)      # ... and two more seeds that do the same


def table_passes(seed):
    return dict(TABLE_PASSES, seed=seed)


UNION_SETS = ((255, 64), (256, 64), (257, 64), (513, 64), (129, 300))     # (M, stride): 255, 256, 257, 513 and 258 work items
WRAP_SETS = (("global", 32), ("lds", 256), ("lds", 300))
CONFLICT_STRIDES = (512, 513)


def other(kw):
    """the different case of the same shape that runs between a case's two calls"""
    return sparse_frames(**dict(kw, seed=kw["seed"] + 100))
