"""The numpy yardstick of image-pair selection on a binary visual vocabulary (include/pgx.h: pgx_vocab_quantize_dev,
pgx_vocab_train_dev, pgx_select_pairs_dev): the three rules restated in integers, so that every GPU output is compared bit for
bit, and the planted scene the tests share.  A plain helper module; tests/test_pairs_ref.py ties it to a second, independent
formulation of each rule."""
import numpy as np

MASK64 = (1 << 64) - 1
_POP8 = np.array([bin(i).count("1") for i in range(256)], dtype=np.uint8)


def popcount32(x):
    """Set bits of every uint32 of x."""
    if hasattr(np, "bitwise_count"):
        return np.bitwise_count(x)
    b = np.ascontiguousarray(x).view(np.uint8).reshape(x.shape + (4,))
    return _POP8[b].sum(axis=-1, dtype=np.uint8)


def clamp_counts(counts, stride):
    return np.clip(np.asarray(counts, dtype=np.int64), 0, stride)


def valid_rows(desc, counts):
    """The valid descriptors by rank: (f, i) ascending -> [N][8] uint32."""
    desc = np.asarray(desc, dtype=np.uint32)
    n = clamp_counts(counts, desc.shape[1])
    return np.concatenate([desc[f, :n[f]] for f in range(desc.shape[0])] + [np.zeros((0, 8), np.uint32)])


def quantize_rows(X, vocab, budget=1 << 22):
    """word [n], dist [n] of the rows X [n][8]: argmin over j of (popcount(x ^ vocab[j]), j), a tie to the smaller j."""
    X = np.ascontiguousarray(X, dtype=np.uint32)
    vocab = np.ascontiguousarray(vocab, dtype=np.uint32)
    n, V = len(X), len(vocab)
    word, dist = np.zeros(n, dtype=np.int64), np.full(n, 1 << 30, dtype=np.int64)
    cw = min(V, 4096)
    rw = max(1, budget // (cw * 8))
    for r0 in range(0, n, rw):
        xs = X[r0:r0 + rw]
        for c0 in range(0, V, cw):   # ascending chunks and a strict comparison: the smaller word keeps a tie
            d = popcount32(xs[:, None, :] ^ vocab[None, c0:c0 + cw, :]).sum(axis=2, dtype=np.int64)
            j = d.argmin(axis=1)     # the first minimum
            dj = d[np.arange(len(xs)), j]
            better = dj < dist[r0:r0 + rw]
            dist[r0:r0 + rw][better] = dj[better]
            word[r0:r0 + rw][better] = c0 + j[better]
    return word, dist


def quantize(desc, counts, vocab, word, wdist=None):
    """pgx_vocab_quantize_dev on copies of word / wdist [F][stride]: entries i < n_f are written, the others are left alone."""
    desc = np.asarray(desc, dtype=np.uint32)
    n = clamp_counts(counts, desc.shape[1])
    word = np.array(word, dtype=np.int32)
    wdist = None if wdist is None else np.array(wdist, dtype=np.int32)
    for f in range(desc.shape[0]):
        if n[f]:
            w, d = quantize_rows(desc[f, :n[f]], vocab)
            word[f, :n[f]] = w
            if wdist is not None:
                wdist[f, :n[f]] = d
    return word, wdist


def splitmix64(state):
    """-> (value, new state), the splitmix64 of the RANSAC stages."""
    state = (state + 0x9E3779B97F4A7C15) & MASK64
    z = state
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & MASK64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & MASK64
    return z ^ (z >> 31), state


def unpack_bits(X):
    """[n][8] uint32 -> [n][256] uint8, bit t = bit t % 32 of word t / 32."""
    X = np.ascontiguousarray(X, dtype="<u4")
    return np.unpackbits(X.view(np.uint8).reshape(len(X), 32), axis=1, bitorder="little")


def pack_bits(B):
    return np.ascontiguousarray(np.packbits(B.astype(np.uint8), axis=1, bitorder="little")).view("<u4").astype(np.uint32)


def train_init(X, V, seed):
    N = len(X)
    assert N >= V
    ranks = []
    for j in range(V):
        lo, hi = j * N // V, (j + 1) * N // V
        z, _ = splitmix64((seed ^ (j * 0xD1B54A32D192ED03)) & MASK64)
        ranks.append(lo + z % (hi - lo))
    return X[np.array(ranks, dtype=np.int64)].copy()


def train_step(X, vocab):
    """One k-majority iteration -> (new vocab, words without a member, bits changed)."""
    V = len(vocab)
    word, _ = quantize_rows(X, vocab)
    c = np.bincount(word, minlength=V).astype(np.int64)
    order = np.argsort(word, kind="stable")
    bits = unpack_bits(X[order]).astype(np.int32)
    nz = np.flatnonzero(c)
    starts = (np.cumsum(c) - c)[nz]
    ones = np.zeros((V, 256), dtype=np.int64)
    if len(nz):
        ones[nz] = np.add.reduceat(bits, starts, axis=0)
    old = unpack_bits(vocab)
    new = np.where(2 * ones > c[:, None], 1, np.where(2 * ones < c[:, None], 0, old)).astype(np.uint8)
    return pack_bits(new), int((c == 0).sum()), int((new != old).sum())


def train(desc, counts, V, iters, seed):
    """pgx_vocab_train_dev -> (vocab [V][8] uint32, report [4])."""
    X = valid_rows(desc, counts)
    vocab = train_init(X, V, seed)
    empty = changed = -1
    for _ in range(iters):
        vocab, empty, changed = train_step(X, vocab)
    return vocab, np.array([len(X), empty, changed, 0], dtype=np.int32)


def histograms(desc, counts, vocab):
    desc = np.asarray(desc, dtype=np.uint32)
    n = clamp_counts(counts, desc.shape[1])
    V = len(vocab)
    h = np.zeros((desc.shape[0], V), dtype=np.int64)
    for f in range(desc.shape[0]):
        if n[f]:
            h[f] = np.bincount(quantize_rows(desc[f, :n[f]], vocab)[0], minlength=V)
    return h


def weight(Fv, df):
    """q of one word under weighting 1."""
    if df == 0:
        return 0
    x = (int(Fv) << 16) // int(df)
    e = x.bit_length() - 1
    return 256 * (e - 16) + ((x << 8) >> e) - 256


def weights(h, weighting):
    """-> (q [V] int64, Fv, df [V])"""
    Fv = int((h.sum(axis=1) > 0).sum())
    df = (h > 0).sum(axis=0)
    if weighting == 0:
        return np.ones(h.shape[1], dtype=np.int64), Fv, df
    assert weighting == 1
    return np.array([weight(Fv, d) for d in df], dtype=np.int64), Fv, df


def score_matrix(h, q):
    """d_scores [F][F] int64: the normalised score of non-empty a != b, -1 elsewhere."""
    F = len(h)
    nonempty = h.sum(axis=1) > 0
    self_ = h @ q
    sc = np.full((F, F), -1, dtype=np.int64)
    for a in range(F):
        if not nonempty[a]:
            continue
        s = np.minimum(h[a][None, :], h) @ q
        den = np.maximum(1, np.minimum(self_[a], self_))
        row = (s << 20) // den
        row[~nonempty] = -1
        row[a] = -1
        sc[a] = row
    return sc


def select_from_scores(sc, top_k, window, min_score, max_pairs):
    """The selection and output rules on a score matrix -> dict(pairlist, pair_score, summary[0], [4], [5] as n, n_window,
    min_nominated, capacity)."""
    F = len(sc)
    nom = np.zeros((F, F), dtype=bool)
    b = np.arange(F)
    for a in range(F):
        cand = np.flatnonzero((sc[a] >= 0) & (sc[a] >= min_score))
        order = cand[np.lexsort((cand, -sc[a][cand]))]
        nom[a, order[:top_k]] = True
    either = nom | nom.T
    pair_ok = (sc >= 0) & (b[None, :] > b[:, None])
    sel = pair_ok & (either | ((b[None, :] - b[:, None]) <= window))
    aa, bb = np.nonzero(sel)   # row-major: lexicographic (a, b)
    n = len(aa)
    pl = np.full((max_pairs, 2), -1, dtype=np.int32)
    ps = np.full(max_pairs, -1, dtype=np.int32)
    m = min(n, max_pairs)
    pl[:m, 0], pl[:m, 1], ps[:m] = aa[:m], bb[:m], sc[aa[:m], bb[:m]]
    nominated = sc[pair_ok & either]
    return dict(pairlist=pl, pair_score=ps, n=n, n_window=int((sel & ~either).sum()),
                min_nominated=int(nominated.min()) if len(nominated) else -1, capacity=n > max_pairs)


def select(desc, counts, vocab, weighting, top_k, window, min_score, max_pairs):
    """pgx_select_pairs_dev -> dict(pairlist [max_pairs][2], pair_score [max_pairs], scores [F][F], summary [8], capacity)."""
    h = histograms(desc, counts, vocab)
    q, Fv, df = weights(h, weighting)
    sc = score_matrix(h, q)
    r = select_from_scores(sc, top_k, window, min_score, max_pairs)
    summary = np.array([r["n"], Fv, int((df == 0).sum()), int((df == Fv).sum()), r["n_window"], r["min_nominated"], 0, 0],
                       dtype=np.int32)
    return dict(pairlist=r["pairlist"], pair_score=r["pair_score"], scores=sc.astype(np.int32), summary=summary,
                capacity=r["capacity"])


# ---- the planted scene ---------------------------------------------------------------------------------------------------

def random_desc(rng, n):
    return rng.integers(0, 1 << 32, size=(n, 8), dtype=np.uint64).astype(np.uint32)


def planted_scene(seed, groups=4, per_group=6, n_desc=512, shared=0.7, flips=8):
    """groups x per_group frames of n_desc descriptors.  Within a group, `shared` of a frame's descriptors are the group's base
    descriptors with `flips` random bits flipped, the rest are fresh random; rows are shuffled per frame.
    -> (desc [F][n_desc][8] uint32, counts [F], group [F])"""
    rng = np.random.default_rng(seed)
    n_sh = int(round(shared * n_desc))
    frames, group = [], []
    for g in range(groups):
        base = random_desc(rng, n_sh)
        for _ in range(per_group):
            bits = unpack_bits(base)
            for i in range(n_sh):
                bits[i, rng.choice(256, size=flips, replace=False)] ^= 1
            d = np.concatenate([pack_bits(bits), random_desc(rng, n_desc - n_sh)])
            frames.append(d[rng.permutation(n_desc)])
            group.append(g)
    return np.stack(frames), np.full(len(frames), n_desc, dtype=np.int32), np.array(group)


def within_group_pairs(group):
    F = len(group)
    return np.array([(a, b) for a in range(F) for b in range(a + 1, F) if group[a] == group[b]], dtype=np.int32).reshape(-1, 2)
