"""Helpers shared by tests/test_pose_ref.py (CPU) and the GPU tests of RANSAC and pose (tests/test_gpu_pose.py,
tests/test_gpu_pose_limits.py, tests/test_gpu_chain.py): the two-view scene with exact entry counts, the per-sample stream seed, the conditioning of a sample's 8-point system, and the inlier-count interval.

The interval.  k_fund_score's inlier test is `res <= threshold` with res = sum_ij F_ij ha_i hb_j, ha = (x1, y1, 1),
hb = (x2, y2, 1): nine products and eight additions of which the ones with a homogeneous 1 are exact, i.e. 12 float32
operations.  On any evaluation order, fused or not, a term passes through at most 5 roundings; taken as 8, every float32
evaluation differs from the exact value by at most g = 8 * 2^-24 * mag, mag = sum_ij |F_ij ha_i hb_j|.  The exact value is
computed here in float64 (integer pixel coordinates below 2^12 and float32 matrix entries: each product is exact in float64
and the sum is good to 2^-50 mag).  So  #(res <= thr - g)  <=  count  <=  #(res <= thr + g)  for the float32 threshold thr."""
import numpy as np

from oracle import pose_np
from photogrammetry_amd import synth
# stream_seed(seed, m, s): the seed under which slot 0 / sample 0 of a call runs the stream of sample s of image pair m
from ransac_ref import M64 as MASK, STREAM_MUL, stream_seed

CH = 1024            # k_fund_score's LDS tile: list entries per chunk


def two_views(n_true, n_out, seed, dup=1, exact=True):
    """True correspondences (rounded pixels) of synth.two_view_pixels' scene seen by two cameras with the reference's K, then
    n_out random wrong ones -> (p1, p2, R, t) with p1, p2 int32 [true + n_out][2].  exact: 2 n_true + 64 points are drawn and
    exactly n_true of those seen in both views kept; otherwise n_true are drawn and what is seen is kept.  dup > 1 repeats
    every entry."""
    rng = np.random.default_rng(seed)
    R, t = synth.rot_y(0.07), np.array([0.6, 0.05, 0.1])
    p1, p2 = synth.two_view_pixels(rng, 2 * n_true + 64 if exact else n_true, pose_np.K.astype(np.float64), R, t)
    if exact:
        p1, p2 = p1[:n_true], p2[:n_true]
        assert len(p1) == n_true
    o1 = np.stack([rng.integers(0, 3000, n_out), rng.integers(0, 4000, n_out)], 1).astype(np.int32)
    o2 = np.stack([rng.integers(0, 3000, n_out), rng.integers(0, 4000, n_out)], 1).astype(np.int32)
    p1, p2 = np.concatenate([p1, o1]), np.concatenate([p2, o2])
    if dup > 1:
        p1, p2 = np.repeat(p1, dup, 0), np.repeat(p2, dup, 0)
    return p1, p2, R, t


def system(p1, p2):
    """The 8-point system of pose_np.estimate_fundamental (centred coordinates), for its conditioning only."""
    c1, c2 = p1.astype(np.float64).mean(0), p2.astype(np.float64).mean(0)
    x1, y1 = p1[:, 0] - c1[0], p1[:, 1] - c1[1]
    x2, y2 = p2[:, 0] - c2[0], p2[:, 1] - c2[1]
    return np.stack([x1 * x2, x1 * y2, x1, y1 * x2, y1 * y2, y1, x2, y2, np.ones_like(x1)], 1)


def clear_null_vector(p1, p2):
    """tests/test_gpu_chain.py's gate: the subset's system has one clear null vector, so two solvers must agree on it."""
    sv = np.linalg.svd(system(p1, p2), compute_uv=False)
    return bool(sv[-2] > 50 * sv[-1] and sv[-2] > 1e-6 * sv[0])


def normed(F):
    F = np.asarray(F, dtype=np.float64).reshape(3, 3)
    return F / np.linalg.norm(F)


def residuals(F, p1, p2):
    """Exact residuals and magnitudes of a float32 matrix over a list -> (res, mag), float64 [n]."""
    F = np.asarray(F, dtype=np.float32).reshape(3, 3).astype(np.float64)
    ha = np.concatenate([p1.astype(np.float64), np.ones((len(p1), 1))], 1)
    hb = np.concatenate([p2.astype(np.float64), np.ones((len(p2), 1))], 1)
    terms = F[None, :, :] * ha[:, :, None] * hb[:, None, :]
    return terms.sum((1, 2)), np.abs(terms).sum((1, 2))


def count_interval(F, p1, p2, threshold):
    """(lo, hi): every float32 evaluation of the inlier test over the list counts between lo and hi entries."""
    res, mag = residuals(F, p1, p2)
    g = 8.0 * 2.0 ** -24 * mag
    thr = float(np.float32(threshold))
    return int((res <= thr - g).sum()), int((res <= thr + g).sum())


# ---- the scenes both test files use: the CPU file confirms their conditions with the oracle's matrices, the GPU file runs them

THR = 0.001                                  # the reference's commented call (Program.cs:229)
REAL_SCENES = ((1025, 0), (1025, 50), (2049, 0), (2049, 20), (4097, 50))     # (true entries, % outliers on top)
REAL_PS = (8, 32, 64)
REAL_SLOTS, REAL_SEED = 300, 5


def real_scene(n_true, pct):
    return two_views(n_true, n_true * pct // 100, 100 + n_true + pct)[:2]


RANK_TOL = 3.0 * 1.1920929e-7                # MathNet's Svd().Rank: singular values above eps32 * 3 * s_max
RANK_SLOTS, RANK_SEED = 300, 9


def rank_verdict(F):
    """(numerical rank as pose_np.numerical_rank computes it, clear): clear when every singular value is above 4 tol or
    below tol / 4, so that a float64 Jacobi solver and numpy's SVD must count the same ones."""
    s = np.linalg.svd(np.asarray(F, dtype=np.float32).reshape(3, 3).astype(np.float64), compute_uv=False)
    tol = s.max() * RANK_TOL
    return int((s > tol).sum()), bool(((s > 4 * tol) | (s < tol / 4)).all())


def window_list(n, w, seed):
    """n random entries inside a w x w pixel window at the origin: without the large translations of real image coordinates
    a subset's matrix has three singular values of comparable size, i.e. numerical rank 3"""
    rng = np.random.default_rng(seed)
    return rng.integers(0, w, (n, 2)).astype(np.int32), rng.integers(0, w, (n, 2)).astype(np.int32)


def rank_lists():
    """name -> (p1, p2, P): clean subsets of 8 and 12, a list no subset of which has rank 2, and a mixed one"""
    c1, c2 = two_views(300, 0, 201)[:2]
    w1, w2 = window_list(400, 32, 3)
    m1, m2 = window_list(300, 32, 4)
    return {"clean8": (c1, c2, 8), "clean12": (c1, c2, 12), "window": (w1, w2, 8),
            "mixed": (np.concatenate([c1, m1]), np.concatenate([c2, m2]), 8)}


def last_sample_list():
    """200 clean entries followed by 400 window entries: with rank_check, a subset of 8 is accepted only when (nearly) all of
    it is clean, which one sample in several thousand is."""
    c1, c2 = two_views(200, 0, 201)[:2]
    w1, w2 = window_list(400, 32, 6)
    return np.concatenate([c1, w1]), np.concatenate([c2, w2]), 200


def last_sample_seed(S, P=8):
    """A seed under which the LAST sample of an S-sample call on last_sample_list() draws clean entries only, has a clear
    rank-2 matrix and at least 590 of the 600 entries as inliers, all by the oracle (candidate 39570 of the search: 594).  The
    other samples of such a call are fresh draws: about 1 % of them are accepted with rank_check, with 30 .. 560 inliers by the
    oracle, so the last sample wins (the caller checks that on the probes)."""
    p1, p2, n_clean = last_sample_list()
    k = 0
    while True:
        k += 1
        X = (k * 0x9E3779B97F4A7C15) & MASK
        idx = pose_np.sample_indices(X, 0, 0, P, len(p1))
        if max(idx) >= n_clean:
            continue
        F = pose_np.estimate_fundamental(p1[idx], p2[idx])
        rank, clear = rank_verdict(F)
        if rank == 2 and clear and pose_np.score(F, p1, p2, THR).sum() >= 590:
            return stream_seed(X, 0, S - 1)
