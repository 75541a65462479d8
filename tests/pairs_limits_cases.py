"""Cases and CPU helpers of tests/test_gpu_vocab_limits.py, tests/test_gpu_select_limits.py and tests/test_gpu_consensus_limits.py
(no torch, no GPU): the launch rules of csrc/k_vocab.hip and csrc/k_consensus.hip restated (tests/test_pairs_limits_cases.py
holds them to the sources' text), the data builders the GPU tests share, and the tiling of the consensus yardstick: a graph of
16400 tracks is a few dozen distinct patterns, each evaluated once by tests/consensus_ref.py and laid out over the track
indices; a sampled track is evaluated on its own under the seed that gives index 0 the stream of its index.  The CPU tests hold
the tiling to the yardstick, bit for bit."""
import numpy as np

import consensus_ref as cref
import pairs_ref as R

# ---- the launch rules ---------------------------------------------------------------------------------------------------------------
VOC_BM, F4_CHUNK = 256, 4096                      # k_vocab.hip, pgx_fp4.h
SEL_T, SEL_WC, SEL_MAXF = 16, 256, 4096           # k_vocab.hip
SCAN_NT = 256                                     # scan_array's step: the workgroup of k_voc_slots, k_voc_scan_words, k_sel_scan
CNS_GRID_MAX, CNS_NT = 1024, 256                  # k_consensus.hip
CNS_LANES = {0: 4, 1: 16, 2: 64}                  # lanes per track of the three length classes


def nrb(S):
    """row blocks per slot of k_vocab_fp4 (pgx_launch_vocab_quantize)"""
    return (S + VOC_BM - 1) // VOC_BM


def xcd_map(lin, nblk, F):
    """pgx_xcd_map (pgx_internal.h): workgroup lin of nblk * F -> (slot f, row block b)"""
    F8 = (F >> 3) << 3
    if lin < nblk * F8:
        j = lin >> 3
        return (j // nblk) * 8 + (lin & 7), j % nblk
    r = lin - nblk * F8
    return F8 + r // nblk, r % nblk


def score_split(F, V):
    """pgx_launch_select_pairs' split of the words over the workgroups of k_sel_scores
    -> (tri, chunks, wpb, nz, words in the last z-slice)"""
    T = (F + SEL_T - 1) // SEL_T
    tri, chunks = T * (T + 1) // 2, (V + SEL_WC - 1) // SEL_WC
    want = max(2048 // tri, 1)
    nz0 = min(want, chunks)
    wpb = (chunks + nz0 - 1) // nz0 * SEL_WC
    nz = (V + wpb - 1) // wpb
    return tri, chunks, wpb, nz, V - (nz - 1) * wpb


def scan_passes(n):
    """passes of scan_array over n values; every pass after the first adds the carry"""
    return (n + SCAN_NT - 1) // SCAN_NT


def cns_grid(max_tracks):
    want = (max_tracks + 3) // 4
    return 1 if want < 1 else min(want, CNS_GRID_MAX)


def cns_class(n):
    return 2 if n > 32 else (1 if n > 8 else 0)


def second_pass_start(max_tracks, cls):
    """PGX_TRACK_LOOP: the first track index that a lane group of length class cls meets in its second pass"""
    return cns_grid(max_tracks) * CNS_NT // CNS_LANES[cls]


# ---- slots of descriptors -------------------------------------------------------------------------------------------------------------

def slots(sets, stride, seed=0):
    """per-slot descriptor sets -> (desc [F][stride][8] with random rows behind every set, counts [F])"""
    rng = np.random.default_rng(len(sets) * 1000 + stride + seed)
    desc = R.random_desc(rng, len(sets) * stride).reshape(len(sets), stride, 8)
    for f, d in enumerate(sets):
        desc[f, :len(d)] = d
    return desc, np.array([len(d) for d in sets], dtype=np.int32)


# ---- the quantiser ----------------------------------------------------------------------------------------------------------------------
QUANT_F, QUANT_S, QUANT_V = (8, 9, 15, 17), (260, 515), (33, 4097)


def quantiser_counts(F, S):
    """counts that differ per slot: above the stride, 0, 257, negative, 256, the stride, 255, 1, the stride less one; the last
    slot is full, so that the slots behind the last group of 8 have row blocks past the first"""
    base = [S + 40, 0, 257, -3, 256, S, 255, 1, S - 1]
    c = np.array([base[f % len(base)] for f in range(F)], dtype=np.int32)
    c[F - 1] = S
    return c


def quantiser_case(F, S, V):
    """distinct random data per slot -> (desc [F][S][8], counts [F], vocab [V][8])"""
    rng = np.random.default_rng(F * 100000 + S * 10 + V)
    desc = R.random_desc(rng, F * S).reshape(F, S, 8)
    vocab = R.random_desc(rng, V)
    desc[F - 1, S - 1] = vocab[V - 1]
    desc[0, VOC_BM] = vocab[0]
    return desc, quantiser_counts(F, S), vocab


def working_blocks(F, S, counts):
    """the (slot, row block) pairs of k_vocab_fp4 that have a row: row block b of slot f starts below the clamped count"""
    n = R.clamp_counts(counts, S)
    return {(f, b) for f in range(F) for b in range(nrb(S)) if b * VOC_BM < n[f]}


STRIDE_LIMIT = 65535
STRIDE_LIMIT_ROWS = ((0, 65534, 4), (0, 65279, 0), (0, 65280, 1), (0, 65281, 2), (1, 65280, 3), (2, 65534, 1))   # (slot, row, word)


def stride_limit_case():
    """S = 65535 (nrb = 256), F = 3, V = 5: a full slot, a slot that ends one row into the last row block and a count above the
    stride; the rows of STRIDE_LIMIT_ROWS equal their word"""
    rng = np.random.default_rng(65535)
    desc = R.random_desc(rng, 3 * STRIDE_LIMIT).reshape(3, STRIDE_LIMIT, 8)
    vocab = R.random_desc(rng, 5)
    for f, i, w in STRIDE_LIMIT_ROWS:
        desc[f, i] = vocab[w]
    return desc, np.array([STRIDE_LIMIT, 65281, 70000], dtype=np.int32), vocab


# ---- training with more than 256 slots ------------------------------------------------------------------------------------------------
TRAIN_F, TRAIN_STRIDE = 600, 3
TRAIN_EMPTY = ((0, 10), (250, 263), (590, 600))       # runs of empty slots: at the front, across the index 256, at the end


def train_case():
    """-> (desc [600][3][8], counts [600] in 0..3, with the runs of TRAIN_EMPTY empty and their neighbours not)"""
    rng = np.random.default_rng(600)
    counts = rng.integers(0, 4, TRAIN_F).astype(np.int32)
    for a, b in TRAIN_EMPTY:
        counts[a:b] = 0
        if a > 0:
            counts[a - 1] = 2
        if b < TRAIN_F:
            counts[b] = 3
    desc = R.random_desc(rng, TRAIN_F * TRAIN_STRIDE).reshape(TRAIN_F, TRAIN_STRIDE, 8)
    return desc, counts


def restride(desc, counts, stride):
    """the same valid rows at another stride, other random rows behind them"""
    n = R.clamp_counts(counts, desc.shape[1])
    return slots([desc[f, :n[f]] for f in range(len(n))], stride, seed=7)


# ---- several histogram chunks per workgroup ---------------------------------------------------------------------------------------------
# (F, V) -> the planted words, each held by the two frames beside it alone
CHUNK_SHAPES = {
    # wpb = 512, 7 slices, the last of 257 words: slice 1's first chunk ends at word 767, slice 2's second chunk starts at 1280,
    # the ragged chunk of the last slice is word 3328 alone
    (257, 3329): ((767, (3, 252)), (1280, (20, 130)), (3328, (100, 256))),
    # wpb = 768, 3 slices, the last of one word: first chunk of slice 0 ends at 255, second and third chunk of slice 1 start at
    # 1024 and 1280, the last slice is word 1536 alone
    (529, 1537): ((255, (3, 520)), (1024, (40, 300)), (1280, (17, 528)), (1536, (250, 251))),
}
CHUNK_STRIDE, CHUNK_COPIES = 48, 3


def chunk_collection(F, V, with_planted=True):
    """F frames whose descriptors ARE words of the vocabulary: most from every 8th word (so that frames share words in every
    chunk of every slice), some from anywhere, never a planted word; frames 50 and F - 2 are empty.  The planted words go, in
    CHUNK_COPIES copies, to their two frames alone (with_planted = False: to none).  -> (desc, counts, vocab)"""
    planted = CHUNK_SHAPES[(F, V)]
    rng = np.random.default_rng(F * 7 + V)
    vocab = R.random_desc(rng, V)
    taken = {w for w, _ in planted}
    hot = np.array([w for w in range(0, V, 8) if w not in taken])
    rest = np.array([w for w in range(V) if w not in taken])
    sets = []
    for f in range(F):
        k = int(rng.integers(30, 41))
        words = np.concatenate([rng.choice(hot, 28), rng.choice(rest, k - 28)])
        if f in (50, F - 2):
            words = words[:0]
        if with_planted:
            for w, pair in planted:
                if f in pair:
                    words = np.concatenate([words, [w] * CHUNK_COPIES])
        sets.append(vocab[words.astype(np.int64)])
    desc, counts = slots(sets, CHUNK_STRIDE)
    return desc, counts, vocab


def chunk_place(w, wpb):
    """word w -> (z-slice, chunk within the slice, word within the chunk)"""
    return w // wpb, (w % wpb) // SEL_WC, w % SEL_WC


# ---- the uint16 halves of the histogram ---------------------------------------------------------------------------------------------------
# (V, word of slot 0, word of slot 1): words 2 and 3 of V = 6 share a 32-bit cell, 3 in its high half; word 6 of V = 7 is the low
# half of the row's last cell, whose high half is padding
HALVES = ((6, 3, 2), (6, 3, 3), (6, 2, 2), (7, 6, 5), (7, 6, 6), (7, 5, 5))


def halves_case(V, w0, w1):
    """F = 3, S = 65535: slot 0 is 65535 copies of word w0, slot 1 of word w1, slot 2 is spread over all words"""
    S = STRIDE_LIMIT
    vocab = R.random_desc(np.random.default_rng(V), V)
    desc = np.stack([np.repeat(vocab[w0:w0 + 1], S, 0), np.repeat(vocab[w1:w1 + 1], S, 0), vocab[np.arange(S) % V]])
    return desc, np.full(3, S, dtype=np.int32), vocab


def half_of(f, V, w):
    """k_sel_hist: entry e = f * Vp + w of the uint16 histogram -> (32-bit cell, 1 for the high half)"""
    e = f * ((V + 1) & ~1) + w
    return e >> 1, e & 1


# ---- long tied rows -------------------------------------------------------------------------------------------------------------------------
TIED_F = 600
TIED_EMPTY = (7, 255, 256, 300, 599)


def tied_case(empty=()):
    """600 identical frames of four descriptors (under weighting 0 every score is 2^20), the slots of `empty` without any"""
    vocab = R.random_desc(np.random.default_rng(16), 16)
    desc = np.tile(vocab[[1, 5, 5, 9]][None], (TIED_F, 1, 1))
    counts = np.full(TIED_F, 4, dtype=np.int32)
    counts[list(empty)] = 0
    return desc, counts, vocab


# ---- a collection with pairs of score 0 -------------------------------------------------------------------------------------------------------
GROUPED_F = 300


def grouped_case():
    """300 frames of 1 to 3 descriptors, frame f from the 16 words of group f % 4 (frames of two groups share no word and score
    0), a few frames empty.  -> (desc, counts, vocab)"""
    rng = np.random.default_rng(300)
    vocab = R.random_desc(rng, 64)
    sets = []
    for f in range(GROUPED_F):
        k = 0 if f in (5, 257, 299) else int(rng.integers(1, 4))
        sets.append(vocab[16 * (f % 4) + rng.integers(0, 16, k)])
    desc, counts = slots(sets, 4)
    return desc, counts, vocab


# ---- consensus: a graph past the grid-stride of the two longer classes ----------------------------------------------------------------------
CNS_TRACKS = 16400
CNS_LONG_AT = (100, 101, 102, 103, 104, 105, 4095, 4096, 4097, 4098, 4099, 4100, 4101, 8190, 8191, 8192, 8193, 8194, 8195, 12288, 12289)
CNS_MID_AT = (200, 201, 202, 203, 204, 205) + tuple(range(16382, 16394)) + (16398, 16399)
CNS_PAT7 = (True, False, True, True, False, False, True)


def consensus_graph(n_tracks=CNS_TRACKS, long_at=CNS_LONG_AT, mid_at=CNS_MID_AT):
    """A graph of n_tracks tracks over the 65 frames of a synthetic scene.  Track t is a two-node track over frames (t % 32,
    t % 32 + 32), consistent or not by CNS_PAT7[t % 7], except at the indices of long_at (33 and 65 nodes) and mid_at (9 and 32
    nodes), where the six patterns of the class take turns: each length clean, with a wrong observation in the middle, and with
    one in the last position.  Every track has keypoints of its own, copies of its pattern's.
    -> dict(kps [65] of [n][2] int64, P, off, nodes, pattern [n_tracks] (an index into patterns), patterns, stride)"""
    from photogrammetry_amd import synth
    s = synth.make_scene(40, 65, seed=3, arc_deg=120.0)
    off, nodes, pts = synth.scene_tracks(s)
    full = [t for t in range(len(off) - 1) if off[t + 1] - off[t] == 65]
    assert len(full) >= 5
    where = [dict(zip(s["point_id"][f].tolist(), range(len(s["point_id"][f])))) for f in range(65)]

    def px(f, p):
        k = s["kps"][f][where[f][int(p)]]
        return int(k["x"]), int(k["y"])

    p3, q = [pts[full[i]] for i in range(3)], pts[full[4]]

    def several(L):
        frames = np.unique(np.linspace(0, 64, L).round().astype(int))
        assert len(frames) == L
        out = []
        for pos in (None, L // 2, L - 1):
            tr = [(int(f), px(f, p3[0])) for f in frames]
            if pos is not None:
                tr[pos] = (tr[pos][0], px(tr[pos][0], q))
            out.append(tr)
        return out

    patterns = []
    for j in range(32):
        p = p3[j % 3]
        patterns.append([(j, px(j, p)), (j + 32, px(j + 32, p))])       # 2 j: consistent
        patterns.append([(j, px(j, p)), (j + 32, px(j + 32, q))])       # 2 j + 1: not
    long_first = len(patterns)
    patterns += several(33) + several(65)
    mid_first = len(patterns)
    patterns += several(9) + several(32)
    pattern = np.array([2 * (t % 32) + (0 if CNS_PAT7[t % 7] else 1) for t in range(n_tracks)])
    for i, t in enumerate(long_at):
        pattern[t] = long_first + i % 6
    for i, t in enumerate(mid_at):
        pattern[t] = mid_first + i % 6
    kps = [[] for _ in range(65)]
    g_nodes, lens = [], []
    for t in range(n_tracks):
        tr = patterns[pattern[t]]
        for f, uv in tr:
            g_nodes.append((f, len(kps[f])))
            kps[f].append(uv)
        lens.append(len(tr))
    kps = [np.array(k, np.int64).reshape(-1, 2) for k in kps]
    return dict(kps=kps, P=s["P"], off=np.concatenate([[0], np.cumsum(lens)]).astype(np.int32),
                nodes=np.array(g_nodes, np.int32).reshape(-1, 2), pattern=pattern, patterns=patterns,
                stride=max(len(k) for k in kps))


def graph_track_of(g, fill=-9):
    """the table track_of [65][stride] of the graph's own tracks; entries no node names hold `fill`"""
    to = np.full((65, g["stride"]), fill, np.int32)
    to[g["nodes"][:, 0], g["nodes"][:, 1]] = np.repeat(np.arange(len(g["off"]) - 1), np.diff(g["off"]))
    return to


def probe_seed(seed, t):
    """the seed under which track 0 runs the sampler's stream of track t of a call under `seed` (ransac_stream)"""
    return seed ^ ((t & 0xFFFFFFFF) << 32)


def consensus_expected(g, in_summary, track_of=None, **kw):
    """consensus_ref.consensus of the graph g, from one call of the yardstick per distinct pattern (exhaustive tracks: the result
    does not depend on the index) and one per sampled track under probe_seed.  -> consensus_ref.consensus's dict, and `sampled`
    [n] bool: the track was evaluated on its own"""
    off, nodes, pattern = g["off"], g["nodes"], g["pattern"]
    kps = [np.asarray(k, np.float64) for k in g["kps"]]
    nt, nf, stride = len(off) - 1, len(kps), g["stride"]
    seed, max_hyp = kw.get("seed", 0), kw.get("max_hyp", 256)
    memo = {}
    stats, keep = np.zeros((nt, 4), np.int32), np.zeros(len(nodes), bool)
    kept, point = np.zeros(nt, np.int64), np.full((nt, 3), np.nan)
    near, sampled = np.zeros(nt, bool), np.zeros(nt, bool)
    rep = np.zeros(8, np.int64)
    for t in range(nt):
        r = memo.get(pattern[t])
        if r is None:
            o = cref.consensus(kps, g["P"], [0, off[t + 1] - off[t]], nodes[off[t]:off[t + 1]], stride=stride,
                               **dict(kw, seed=probe_seed(seed, t)))
            surv = o["map"][0] >= 0
            n_k = int(o["stats"][0, 0])
            r = (o["stats"][0], o["keep"], int(o["offsets"][-1]) if surv else 0, o["xyz"][0] if surv else np.full(3, np.nan),
                 bool(o["near"][0]), o["report"].astype(np.int64), n_k * (n_k - 1) // 2 > max_hyp)
            if not r[6]:
                memo[pattern[t]] = r
        stats[t], keep[off[t]:off[t + 1]], kept[t], point[t], near[t], sampled[t] = r[0], r[1], r[2], r[3], r[4], r[6]
        rep[[2, 4, 5, 6, 7]] += r[5][[2, 4, 5, 6, 7]]
    surv = kept > 0
    tmap = np.where(surv, np.cumsum(surv) - 1, -1).astype(np.int32)
    node_track = np.repeat(np.arange(nt), np.diff(off))
    sel = keep & surv[node_track]
    summary = np.zeros(8, np.int32)
    summary[[2, 3, 4, 6]] = np.asarray(in_summary)[[2, 3, 4, 6]]
    summary[0], summary[1], summary[5] = surv.sum(), sel.sum(), kept.max(initial=0)
    rep[0], rep[1], rep[3] = nt, surv.sum(), sel.sum()
    und = (stats[surv, 3] & (cref.FEWVIEWS | cref.LOWPARALLAX)) != 0
    out = dict(offsets=np.concatenate([[0], np.cumsum(kept[surv])]).astype(np.int32), nodes=nodes[sel].astype(np.int32),
               summary=summary, map=tmap, xyz=point[surv], flags=np.where(und, cref.TRI_FEWVIEWS, 0).astype(np.int32), stats=stats,
               report=rep.astype(np.int32), near=near, keep=keep, track_of=None, sampled=sampled)
    if track_of is not None:
        to = np.array(track_of, dtype=np.int32).reshape(nf, -1)
        val = np.where(surv[node_track], np.where(keep, tmap[node_track], -3), -1)
        to[nodes[:, 0], nodes[:, 1]] = val
        out["track_of"] = to
    return out
