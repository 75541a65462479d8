"""Cases and CPU helpers of tests/test_gpu_verify_limits.py and tests/test_gpu_init_pair_limits.py (no torch, no GPU): the launch
rules of csrc/k_verify.hip and csrc/k_initpair.hip restated (tests/test_verify_limits_cases.py holds them to the sources'
text), the yardstick's predicate broadcast over samples, a vectorised sampler, and the data whose first all-good sample
lies late in the call.  Python's loop over the 65536 samples of a call at the API limit takes seconds; the batch forms here
take a fraction of one and are held to verify_ref's, bit for bit, by the CPU tests."""
import numpy as np

import verify_ref as ref
from ransac_ref import M64, STREAM_MUL, stream_seed

# ---- the launch rules --------------------------------------------------------------------------------------------------------------
VER_NT, VER_SNT, VER_CHUNK_CELLS = 256, 64, 1 << 16      # k_verify.hip
MAX_SAMPLES, MAX_REFITS = 65536, 8                       # pgx_api.hip: samples_ok, ver_args
INIT_NT, INIT_ROWS, INIT_SLICE = 256, 2048, 65535        # k_initpair.hip


def verify_chunk(M, n_samples):
    """pgx_verify_chunk (ransac_chunk of pgx_ransac.h): the samples per chunk of a call of M pairs (M <= the pairs per
    workspace): 2^16 cells over M pairs in whole scoring workgroups, never below one, never above n_samples rounded up"""
    g = VER_NT
    ch = VER_CHUNK_CELLS // max(M, 1)
    ch = g if ch < g else ch & ~(g - 1)
    return min(ch, (n_samples + g - 1) & ~(g - 1))


def pick_place(s, chunk):
    """where k_ver_pick meets the key of sample s -> (chunk index, scoring workgroup within the chunk, wave of the thread that
    reads that workgroup's key, pass of that thread's loop)"""
    b = (s % chunk) // VER_NT
    return s // chunk, b, (b % VER_NT) // 64, b // VER_NT


def init_split(stride):
    """the scoring workgroups per pair of k_init_score"""
    return (stride + INIT_ROWS - 1) // INIT_ROWS


def probe_seed(seed, s):
    """the seed under which sample 0 of the same slots runs the stream of sample s of a call under `seed` (include/pgx.h)"""
    return (seed ^ ((s * STREAM_MUL) & M64)) & M64


# ---- the predicate over many samples -----------------------------------------------------------------------------------------------

def predicate_many(Fs, pa, pb, inlier_px):
    """verify_ref.predicate for every row of Fs [S][9] at once, the same operations in the same order -> bool [S][n]"""
    F = np.asarray(Fs, np.float64).reshape(-1, 9)[:, :, None]
    x, y, u, v = (np.asarray(c, np.float64)[None, :] for c in (pa[:, 0], pa[:, 1], pb[:, 0], pb[:, 1]))
    with np.errstate(all="ignore"):
        m0 = (F[:, 0] * u + F[:, 1] * v) + F[:, 2]
        m1 = (F[:, 3] * u + F[:, 4] * v) + F[:, 5]
        m2 = (F[:, 6] * u + F[:, 7] * v) + F[:, 8]
        e = (x * m0 + y * m1) + m2
        l0 = (F[:, 0] * x + F[:, 3] * y) + F[:, 6]
        l1 = (F[:, 1] * x + F[:, 4] * y) + F[:, 7]
        d = ((l0 * l0 + l1 * l1) + m0 * m0) + m1 * m1
        T = np.float64(inlier_px) * np.float64(inlier_px)
        return (d > 0) & (e * e <= T * d)


# ---- the sampler over many samples -------------------------------------------------------------------------------------------------

def _splitmix(state):
    """ransac_ref.splitmix64 on uint64 arrays (which wrap modulo 2^64) -> (new state, output)"""
    with np.errstate(over="ignore"):
        state = state + np.uint64(0x9E3779B97F4A7C15)
        z = state
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        return state, z ^ (z >> np.uint64(31))


VECTOR_DRAWS = 64       # draws per sample in numpy; a sample still short of 8 positions by then goes to verify_ref.sample


def first_positions(seed, a, b, S, n):
    """verify_ref.sample(seed, a, b, s, n) for s = 0 .. S-1 -> int64 [S][8].  The first 8 draws of all samples at once; the
    samples with a repeated draw go on drawing, together, up to VECTOR_DRAWS draws, and what is still short then is
    verify_ref.sample's own loop."""
    assert n >= 8 and 0 <= S <= 1 << 32
    with np.errstate(over="ignore"):
        state = (np.uint64(stream_seed(seed, a, 0)) ^ np.arange(S, dtype=np.uint64) * np.uint64(STREAM_MUL)
                 ^ np.uint64(((b & 0xFFFFFFFF) * 0x9E3779B97F4A7C15) & M64))
    ids = np.full((S, 8), -1, np.int64)
    have = np.zeros(S, np.int64)
    rows = np.arange(S)
    for _ in range(VECTOR_DRAWS):
        if not len(rows):
            break
        state[rows], z = _splitmix(state[rows])
        c = (z % np.uint64(n)).astype(np.int64)
        new = ~(ids[rows] == c[:, None]).any(1)
        r = rows[new]
        ids[r, have[r]] = c[new]
        have[r] += 1
        rows = rows[have[rows] < 8]
    for s in rows:
        ids[s] = ref.sample(seed, a, b, int(s), n)
    return ids


def first_all_good(seed, a, b, S, n, g):
    """the first sample s < S of slots (a, b) whose 8 positions are all < g; -1 when there is none"""
    hit = np.flatnonzero((first_positions(seed, a, b, S, n) < g).all(1))
    return int(hit[0]) if len(hit) else -1


# ---- a winner late in the call -----------------------------------------------------------------------------------------------------

LATE_N, LATE_G, LATE_DATA_SEED, LATE_IP = 40, 14, 99, 1.5
# call seed -> the first all-good sample of slots (0, 1) at n = 40, g = 14: scoring workgroups 90, 156 and 199 of a one-chunk
# call, which threads 90, 156 and 199 of k_ver_pick read: waves 1, 2 and 3
LATE_ONE = {4: 23158, 6: 40149, 5: 51091}
# two pairs (chunks of 32768 samples): slots (0, 1) win in the second chunk, slots (2, 3) in the first and keep it
LATE_TWO = dict(seed=29, slots=((0, 1), (2, 3)), first=(37447, 17977))
# three pairs (chunks of 21760, 21760, 21760 and 256 samples): slots (2, 3), (0, 1) and (4, 5) win in the first, second and
# third chunk
LATE_THREE = dict(seed=29, slots=((0, 1), (2, 3), (4, 5)), first=(37447, 17977, 45554))


def on_relation(rng, n):
    """n integer correspondences exactly on 2x + y - 2u - v + 37 = 0 (test_gpu_verify.relation's) -> (pa [n][2], pb [n][2])"""
    x, y, u = rng.integers(0, 1920, n), rng.integers(0, 1080, n), rng.integers(0, 1920, n)
    return np.stack([x, y], 1), np.stack([u, 2 * x + y - 2 * u + 37], 1)


def late_winner_case(slots=((0, 1),), n=LATE_N, g=LATE_G, data_seed=LATE_DATA_SEED):
    """One pair per entry of slots: candidates 0 .. g-1 in list order lie exactly on the relation, the other n - g have a
    random v at least 100 px off it (21 thresholds of 1.5 px: sqrt(10) px in v per px of distance).  Eight exact points fix
    the relation's F, so a sample of good candidates alone counts the g good ones and none of the junk; a sample with a junk
    point fits its own eight.  The list is the identity (k1 = k2 = position, dist 5), stride = n.
    -> (kp [F][n][4], counts [F], pl, ml [M][n][3], pts: per pair (pa, pb) float64)"""
    rng = np.random.default_rng(data_seed)
    F = max(max(p) for p in slots) + 1
    kp, counts = np.zeros((F, n, 4), np.int32), np.zeros(F, np.int32)
    ml = np.zeros((len(slots), n, 3), np.int32)
    pts = []
    for m, (a, b) in enumerate(slots):
        pa, pb = on_relation(rng, n)
        off = rng.integers(100, 3000, n - g) * rng.choice([-1, 1], n - g)
        pb[g:, 1] += off
        kp[a, :, :2], kp[b, :, :2] = pa, pb
        counts[a] = counts[b] = n
        ml[m] = np.stack([np.arange(n), np.arange(n), np.full(n, 5)], 1)
        pts.append((pa.astype(np.float64), pb.astype(np.float64)))
    return kp, counts, [tuple(p) for p in slots], ml, pts


def yardstick_counts(seed, a, b, S, pa, pb, inlier_px=LATE_IP):
    """verify_ref's count of samples 0 .. S-1 of slots (a, b) on the candidates (pa, pb) -> int64 [S], -1 = no model"""
    n, out = len(pa), np.full(S, -1, np.int64)
    ids = first_positions(seed, a, b, S, n)
    for s in range(S):
        Fs = ref.fit(pa[ids[s]], pb[ids[s]])
        if Fs is not None:
            out[s] = int(ref.predicate(Fs, pa, pb, inlier_px).sum())
    return out
