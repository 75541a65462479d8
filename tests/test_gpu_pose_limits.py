"""GPU tests of the RANSAC and pose kernels (photogrammetry_amd/csrc/k_pose.hip) past their chunk and grid limits, as exact
statements wherever one exists (helpers and derivations: tests/pose_ref.py, conditions confirmed on the CPU by
tests/test_pose_ref.py):

  * a sample is a pure function of (seed, m, s): a call with M = 1, n_samples = 1 and seed ^ (m << 32) ^ (s * C) lays sample s
    of image pair m open, and the same sample must give the same bits in any call shape (`probe`);
  * a threshold of +3e38 makes every entry an inlier of every sample (count == n, sample 0 wins), -3e38 none;
  * at the real threshold the count lies in the interval obtained by scoring the GPU's own float32 matrix in float64.

What stays at a tolerance: a sample's matrix against oracle/pose_np.py (2e-3 after normalisation, subsets with a clear null
vector only) and pgx_pose_dev against pose_np.estimate_pose (the tolerances of tests/test_gpu_pose.py).  Every test asserts
on the host that its shape reaches the path it names.  Wall time on an MI355X: 3.8 s for the file, at most 0.41 s per test."""
import numpy as np
import pytest
import torch

import pose_ref as pr
from oracle import pose_np
import photogrammetry_amd as pg

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
I32 = dict(dtype=torch.int32, device=DEV)
F32 = dict(dtype=torch.float32, device=DEV)
SENT_F, SENT_I = 7.5, 77                      # what the output buffers hold before a call


@pytest.fixture(scope="module")
def engine():
    e = pg.Engine(0)
    yield e
    e.close()


class Lists:
    """Device buffers of a batch: image pair (slot) m = frames pl[m]; keypoint k of frame a is correspondence k, frame b holds
    them permuted, so that k2 != k1 and the indirection through the list is exercised."""

    def __init__(self, sets, stride, slots=None, counts=None):
        """sets: [(p1, p2)], slot m = frames (2m, 2m + 1); with `slots`, that many slots all name frames (0, 1) and hold copies
        of the one list.  counts: overrides counts[] (the rows of the list past n are (0, 0, 0): valid indices)."""
        nset = len(sets)
        kp = np.zeros((2 * nset, stride), dtype=pg.KEYPOINT_DTYPE)
        ml = np.zeros((nset, stride, 3), dtype=np.int32)
        cnt = np.zeros(2 * nset, dtype=np.int32)
        for m, (p1, p2) in enumerate(sets):
            n = len(p1)
            assert n <= stride and len(p2) == n
            perm = np.random.default_rng(1000 + m).permutation(n)
            kp["x"][2 * m, :n], kp["y"][2 * m, :n] = p1[:, 0], p1[:, 1]
            kp["x"][2 * m + 1, perm], kp["y"][2 * m + 1, perm] = p2[:, 0], p2[:, 1]
            ml[m, :n, 0], ml[m, :n, 1] = np.arange(n), perm
            assert n < 2 or (ml[m, :n, 0] != ml[m, :n, 1]).any()
            cnt[2 * m] = cnt[2 * m + 1] = n
        if counts is not None:
            cnt[:] = counts
        pl = np.array([[2 * m, 2 * m + 1] for m in range(nset)], dtype=np.int32)
        self.sets, self.stride = sets, stride
        self.kp = torch.from_numpy(kp.view(np.int32).reshape(2 * nset, stride, 4)).to(DEV)
        self.ml = torch.from_numpy(ml).to(DEV)
        self.pl = torch.from_numpy(pl).to(DEV)
        self.counts = torch.from_numpy(cnt).to(DEV)
        self.M = nset
        if slots is not None:
            assert nset == 1
            self.ml = self.ml.repeat(slots, 1, 1).contiguous()
            self.pl = self.pl.repeat(slots, 1).contiguous()
            self.M = slots


def ransac(engine, d, S, P, thr, seed, rank_check=False, M=None, pad=2):
    """One pgx_fundamental_ransac_dev call over the first M slots -> (F [M][9] float32, inliers [M], best_sample [M]); the `pad`
    rows behind them must keep their sentinel."""
    M = d.M if M is None else M
    dF = torch.full((M + pad, 9), SENT_F, **F32)
    din, dbs = torch.full((M + pad,), SENT_I, **I32), torch.full((M + pad,), SENT_I, **I32)
    torch.cuda.synchronize()
    engine.fundamental_ransac_dev(d.kp, d.ml, d.counts, d.pl, M, d.stride, S, P, thr, dF, din, dbs, rank_check=rank_check, seed=seed)
    engine.check_status()
    F, inl, bs = dF.cpu().numpy(), din.cpu().numpy(), dbs.cpu().numpy()
    assert (F[M:] == np.float32(SENT_F)).all() and (inl[M:] == SENT_I).all() and (bs[M:] == SENT_I).all()
    return F[:M], inl[:M], bs[:M]


def probe(engine, d, P, thr, keys, rank_check=False):
    """keys: [(seed, m, s)] -> (F [K][9], inliers [K], best_sample [K]) of K one-sample calls (M = 1, n_samples = 1) on slot m's
    list under the seed that runs the stream of sample s of image pair m.  One synchronisation for all of them."""
    K = len(keys)
    dF = torch.full((K + 1, 9), SENT_F, **F32)
    din, dbs = torch.full((K + 1,), SENT_I, **I32), torch.full((K + 1,), SENT_I, **I32)
    torch.cuda.synchronize()
    for k, (seed, m, s) in enumerate(keys):
        engine.fundamental_ransac_dev(d.kp, d.ml[m:], d.counts, d.pl[m:], 1, d.stride, 1, P, thr, dF[k:], din[k:], dbs[k:],
                                      rank_check=rank_check, seed=pr.stream_seed(seed, m, s))
    engine.check_status()
    F, inl, bs = dF.cpu().numpy(), din.cpu().numpy(), dbs.cpu().numpy()
    assert F[K, 0] == np.float32(SENT_F) and inl[K] == SENT_I and bs[K] == SENT_I
    return F[:K], inl[:K], bs[:K]


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def assert_none(F, inl, bs, m):
    assert inl[m] == -1 and bs[m] == -1 and (bits(F[m]) == 0).all(), (m, inl[m], bs[m], F[m])


# ------------------------------------------------------------------------------------------------------------ chunk edges

EDGE_N = (8, 255, 256, 257, 1023, 1024, 1025, 2048, 2049, 4097)
EDGE_S = (1, 64, 65, 256, 257, 1000)
EDGE_CASES = [(n, EDGE_S[(i + k) % 6]) for i, n in enumerate(EDGE_N) for k in (0, 3)]


def test_edge_cases_cover_every_size_twice():
    """(not a kernel test: the pairing below) every n with two sample counts, every sample count with two n or more; lists of
    1, 2, 3 and 5 chunks of k_fund_score; grid.y > 0 in k_fund_samples (> 64 samples) and k_fund_score (> 256)."""
    for n in EDGE_N:
        assert len({s for nn, s in EDGE_CASES if nn == n}) == 2
    for s in EDGE_S:
        assert len({n for n, ss in EDGE_CASES if ss == s}) >= 2
    assert {-(-n // pr.CH) for n in EDGE_N} == {1, 2, 3, 5}
    assert any(n > pr.CH and s > 256 for n, s in EDGE_CASES) and any(n % pr.CH == 1 and n > pr.CH for n in EDGE_N)


@pytest.mark.parametrize("n,S", EDGE_CASES)
def test_every_entry_counted_once_at_chunk_edges(engine, n, S):
    """Threshold +3e38: every entry is an inlier of every sample, so the count is n exactly (one entry lost or counted twice at
    a chunk edge changes it), all samples tie, sample 0 wins and its matrix has the bits of the one-sample call.  -3e38: no
    inlier, so -1 / -1 / zeros.  Two slots on one list (slot 1 runs its own stream), stride > n."""
    stride = 4160
    p1, p2 = pr.two_views(n, 0, 400 + n)[:2]
    d = Lists([(p1, p2)], stride, slots=2)
    assert len(p1) == n < stride
    F1, in1, bs1 = ransac(engine, d, 1, 8, 3e38, 17)
    F, inl, bs = ransac(engine, d, S, 8, 3e38, 17)
    for m in range(2):
        assert in1[m] == n and bs1[m] == 0
        assert inl[m] == n and bs[m] == 0, (m, inl[m], bs[m])
        assert (bits(F[m]) == bits(F1[m])).all() and np.isfinite(F[m]).all() and np.abs(F[m]).max() > 0
    assert n == 8 or (bits(F[0]) != bits(F[1])).any()             # slot 1 drew another subset (n == P: both hold the whole list)
    F, inl, bs = ransac(engine, d, S, 8, -3e38, 17)
    for m in range(2):
        assert_none(F, inl, bs, m)


# ----------------------------------------------------------------------------------------------- real threshold, per sample

@pytest.mark.parametrize("n_true,pct", pr.REAL_SCENES)
def test_real_threshold_counts_lie_in_their_interval(engine, n_true, pct):
    """Threshold 0.001, 300 samples per subset size laid open as 300 slots on the same two frames (slot j runs the stream
    (seed, j, 0)).  The matrix equals the oracle's on the same subset to 2e-3 where the subset has a clear null vector
    (tests/test_gpu_chain.py's gate); the count lies in the interval computed from the GPU's own matrix.  Conditions on the
    intervals (not measurements): at least 75 % one number, none wider than 4; tests/test_pose_ref.py confirms both for these
    scenes with the oracle's matrices (82 .. 100 %, at most 3)."""
    p1, p2 = pr.real_scene(n_true, pct)
    n = len(p1)
    assert -(-n // pr.CH) > 1                                      # second and later chunks of k_fund_score
    d = Lists([(p1, p2)], 6208, slots=pr.REAL_SLOTS)
    compared = 0
    for P in pr.REAL_PS:
        F, inl, bs = ransac(engine, d, 1, P, pr.THR, pr.REAL_SEED)
        one, widest = 0, 0
        for j in range(pr.REAL_SLOTS):
            idx = pose_np.sample_indices(pr.REAL_SEED, j, 0, P, n)
            if inl[j] == -1:                                       # no inlier at all: the matrix is not reported
                assert_none(F, inl, bs, j)
                continue
            assert bs[j] == 0
            if pr.clear_null_vector(p1[idx], p2[idx]):
                Fo = pose_np.estimate_fundamental(p1[idx], p2[idx])
                assert np.abs(pr.normed(F[j]) - pr.normed(Fo)).max() < 2e-3, (P, j)
                compared += 1
            lo, hi = pr.count_interval(F[j], p1, p2, pr.THR)
            assert lo <= inl[j] <= hi, (P, j, lo, int(inl[j]), hi)
            one += lo == hi
            widest = max(widest, hi - lo)
        print("n %d P %d: one-number intervals %d / %d, widest %d" % (n, P, one, pr.REAL_SLOTS, widest))
        assert one >= 0.75 * pr.REAL_SLOTS and widest <= 4, (P, one, widest)
    print("matrices compared with the oracle: %d" % compared)
    assert compared >= 30          # the gate passes 34 .. 79 of 300 subsets of 8 on these scenes (CPU), more with outliers


# --------------------------------------------------------------------------------------------------- the winner, bit for bit

WIN_S = (96, 300, 1000)


def test_winner_is_the_first_best_sample_bit_for_bit(engine):
    """Two lists in one call, S = 96, 300, 1000 samples; every sample s < 1000 of both laid open by a one-sample call.  Inliers
    == max_s c_s, best_sample == the first argmax, the matrix has that probe's bits.  Slot 0: 1500 true entries + 750
    outliers (three chunks; by the oracle the winner of 1000 samples is sample 752, 15 entries clear of the runner-up).  Slot 1:
    20 true + 10 wrong entries, where by the oracle 4, 4 and 16 samples reach the maximum of 28: a real tie that is not the
    all-tie of the +3e38 test."""
    big, small = pr.two_views(1500, 750, 311)[:2], pr.two_views(20, 10, 305)[:2]
    d = Lists([big, small], 2304)
    assert len(big[0]) == 2250 > 2 * pr.CH and len(small[0]) == 30
    seed, P = 33, 8
    keys = [(seed, m, s) for m in range(2) for s in range(max(WIN_S))]
    Fp, cp, bp = probe(engine, d, P, pr.THR, keys)
    Fp, cp = Fp.reshape(2, max(WIN_S), 9), cp.reshape(2, max(WIN_S))
    late, tied = 0, 0
    for S in WIN_S:
        F, inl, bs = ransac(engine, d, S, P, pr.THR, seed)
        for m in range(2):
            c = cp[m, :S]
            assert c.max() > 0 and inl[m] == c.max(), (S, m, int(inl[m]), int(c.max()))
            assert bs[m] == int(np.argmax(c)), (S, m, int(bs[m]), int(np.argmax(c)))
            assert (bits(F[m]) == bits(Fp[m, bs[m]])).all(), (S, m)
            late += bs[m] >= 256
            if m == 1 and (c == c.max()).sum() >= 2:
                assert c.max() < 30
                tied += 1
    assert late >= 1                      # a winner past blockIdx.y = 0 of all three kernels
    assert tied == len(WIN_S)             # 'first' held on a real tie at every S


# ------------------------------------------------------------------------------------------------------------- rank_check

def test_rank_check_rejects_exactly_the_matrices_not_of_rank_2(engine):
    """Per-sample probes with rank_check = 1 on clean subsets of 8 and 12, on a list whose subsets all have rank 3 and on a mixed
    one (300 slots each).  The verdict must equal pose_np.numerical_rank of the sample's own float32 matrix wherever its
    singular values are clear of 3 * eps32 * s_max by a factor 4 on both sides.  A rejected sample reports -1 / -1 / zeros, an
    accepted one the bits it has with rank_check = 0.  At most 10 % of the samples may be unclear and both verdicts must occur 5
    times (tests/test_pose_ref.py: 75 of 1200 unclear, 543 and 582 with the oracle's matrices)."""
    unclear, accepted, rejected, total = 0, 0, 0, 0
    for name, (p1, p2, P) in pr.rank_lists().items():
        d = Lists([(p1, p2)], 640, slots=pr.RANK_SLOTS)
        F0, c0, b0 = ransac(engine, d, 1, P, pr.THR, pr.RANK_SEED)
        F1, c1, b1 = ransac(engine, d, 1, P, pr.THR, pr.RANK_SEED, rank_check=True)
        for j in range(pr.RANK_SLOTS):
            total += 1
            same = c1[j] == c0[j] and b1[j] == b0[j] and (bits(F1[j]) == bits(F0[j])).all()
            none = c1[j] == -1 and b1[j] == -1 and (bits(F1[j]) == 0).all()
            assert same or none, (name, j)
            if c0[j] == -1:               # no inlier even unchecked: the matrix is not reported, nothing to judge
                unclear += 1
                continue
            rank, clear = pr.rank_verdict(F0[j])
            assert rank == pose_np.numerical_rank(F0[j].reshape(3, 3))
            if not clear:
                unclear += 1
            elif rank == 2:
                assert same, (name, j)
                accepted += 1
            else:
                assert none, (name, j, rank)
                rejected += 1
    print("rank_check: %d accepted, %d rejected, %d unclear of %d" % (accepted, rejected, unclear, total))
    assert unclear <= 0.10 * total and accepted >= 5 and rejected >= 5


def test_rank_check_in_multi_sample_calls(engine):
    """A call whose samples are all rejected reports -1; a call with mixed verdicts picks the first best among the accepted
    only.  The verdict of every sample comes from its one-sample probe with rank_check = 1."""
    lists = pr.rank_lists()
    w1, w2, P = lists["window"]
    d = Lists([(w1, w2)], 640)
    S, seed = 64, pr.RANK_SEED
    Fp, cp, bp = probe(engine, d, P, pr.THR, [(seed, 0, s) for s in range(S)], rank_check=True)
    Fu, cu, bu = probe(engine, d, P, pr.THR, [(seed, 0, s) for s in range(S)])
    assert (cp == -1).all() and (cu > 0).any()        # every sample rejected, and not for want of inliers
    F, inl, bs = ransac(engine, d, S, P, pr.THR, seed, rank_check=True)
    assert_none(F, inl, bs, 0)
    m1, m2, P = lists["mixed"]
    d = Lists([(m1, m2)], 640)
    S = 300
    Fp, cp, bp = probe(engine, d, P, pr.THR, [(seed, 0, s) for s in range(S)], rank_check=True)
    Fu, cu, bu = probe(engine, d, P, pr.THR, [(seed, 0, s) for s in range(S)])
    acc = cp > 0
    assert acc.sum() >= 2 and ((cu > 0) & ~acc).sum() >= 2                       # both verdicts in one call
    assert (cp[acc] == cu[acc]).all() and (bits(Fp[acc]) == bits(Fu[acc])).all()
    F, inl, bs = ransac(engine, d, S, P, pr.THR, seed, rank_check=True)
    assert inl[0] == cp.max() and bs[0] == int(np.argmax(cp)) and (bits(F[0]) == bits(Fp[bs[0]])).all()
    F, inl, bs = ransac(engine, d, S, P, pr.THR, seed)
    assert inl[0] == cu.max() and bs[0] == int(np.argmax(cu)) and (bits(F[0]) == bits(Fu[bs[0]])).all()


@pytest.mark.parametrize("S", [512, 768, 1024])
def test_last_sample_of_a_full_grid_row_wins(engine, S):
    """S a multiple of 256: the last sample is the last thread of the last workgroup row of k_fund_score (and of k_fund_samples).
    The seed is built so that sample S - 1 is a known good one (pose_ref.last_sample_seed) and rank_check rejects nearly every
    other sample; the probes say which sample wins, and it must be the last for the shape to count."""
    p1, p2, n_clean = pr.last_sample_list()
    d = Lists([(p1, p2)], 640)
    seed = pr.last_sample_seed(S)
    Fp, cp, bp = probe(engine, d, 8, pr.THR, [(seed, 0, s) for s in range(S)], rank_check=True)
    assert int(np.argmax(cp)) == S - 1 and (cp == cp.max()).sum() == 1 and S % 256 == 0
    F, inl, bs = ransac(engine, d, S, 8, pr.THR, seed, rank_check=True)
    assert bs[0] == S - 1 and inl[0] == cp[S - 1] and (bits(F[0]) == bits(Fp[S - 1])).all()


# ------------------------------------------------------------------------------------------------------------ count edges

def test_count_edges_and_argument_errors(engine):
    seed = 3
    for P in (8, 64):                                              # n == P: every sample is a permutation of the whole list
        p1, p2 = pr.two_views(P, 0, 500 + P)[:2]
        d = Lists([(p1, p2)], 128)
        assert sorted(pose_np.sample_indices(seed, 0, 1, P, P)) == list(range(P))
        F, inl, bs = ransac(engine, d, 4, P, pr.THR, seed)
        Fp, cp, bp = probe(engine, d, P, pr.THR, [(seed, 0, s) for s in range(4)])
        assert inl[0] == cp.max() and bs[0] == int(np.argmax(cp)) and (bits(F[0]) == bits(Fp[bs[0]])).all()
        for s in range(4):
            if cp[s] > 0:
                lo, hi = pr.count_interval(Fp[s], p1, p2, pr.THR)
                assert lo <= cp[s] <= hi
        F, inl, bs = ransac(engine, d, 4, P, 3e38, seed)
        assert inl[0] == P and bs[0] == 0
        if P == 8:                                                 # 8 x 9 system: an exact null vector
            Fo = pose_np.estimate_fundamental(*[p[pose_np.sample_indices(seed, 0, 0, P, P)] for p in (p1, p2)])
            assert np.abs(pr.normed(F[0]) - pr.normed(Fo)).max() < 2e-3
        d = Lists([(p1[:P - 1], p2[:P - 1])], 128)                 # n == P - 1 (CameraPoseEstimation.cs:31-32)
        F, inl, bs = ransac(engine, d, 4, P, 3e38, seed)
        assert_none(F, inl, bs, 0)
    # counts[a] > stride behaves exactly like counts[a] == stride (the list fills its stride: 2 chunks)
    stride = 1100
    p1, p2 = pr.two_views(stride, 0, 600)[:2]
    outs = []
    for cnt in (stride, stride + 1000, 2 ** 31 - 1):
        d = Lists([(p1, p2)], stride, counts=[cnt, cnt])
        outs.append(ransac(engine, d, 70, 8, pr.THR, seed) + ransac(engine, d, 70, 8, 3e38, seed))
    assert outs[0][4][0] == stride
    for o in outs[1:]:
        for a, b in zip(outs[0], o):
            assert a.tobytes() == b.tobytes()
    for cnt in (0, -5):                                            # counts[a] <= 0
        d = Lists([(p1, p2)], stride, counts=[cnt, stride])
        F, inl, bs = ransac(engine, d, 4, 8, 3e38, seed)
        assert_none(F, inl, bs, 0)
    d = Lists([(p1, p2)], stride)
    dF, di = torch.full((1, 9), SENT_F, **F32), torch.full((2,), SENT_I, **I32)
    for S, P in ((4, 65), (0, 8), (65535 * 64 + 1, 8), (4, 7)):
        with pytest.raises(pg.ArgumentException):
            engine.fundamental_ransac_dev(d.kp, d.ml, d.counts, d.pl, 1, stride, S, P, pr.THR, dF, di[:1], di[1:])
    engine.fundamental_ransac_dev(d.kp, d.ml, d.counts, d.pl, 0, stride, 4, 8, pr.THR, dF, di[:1], di[1:])     # M = 0
    engine.check_status()
    assert (dF.cpu().numpy() == np.float32(SENT_F)).all() and (di.cpu().numpy() == SENT_I).all()


# ------------------------------------------------------------------------------------------------------- many image pairs

def pose_call(engine, d, F, M=None, points=True):
    M = d.M if M is None else M
    dF = torch.from_numpy(np.ascontiguousarray(F, dtype=np.float32).reshape(M, 9)).to(DEV)
    dRt = torch.full((M + 1, 12), SENT_F, **F32)
    dv, db = torch.full((M + 1, 4), SENT_I, **I32), torch.full((M + 1,), SENT_I, **I32)
    dpts = torch.full((M, d.stride, 3), SENT_F, **F32) if points else None
    torch.cuda.synchronize()
    engine.pose_dev(d.kp, d.ml, d.counts, d.pl, M, d.stride, dF, dRt, dv, db, dpts)
    engine.check_status()
    Rt, v, b = dRt.cpu().numpy(), dv.cpu().numpy(), db.cpu().numpy()
    assert (Rt[M] == np.float32(SENT_F)).all() and (v[M] == SENT_I).all() and b[M] == SENT_I
    return Rt[:M], v[:M], b[:M], (dpts.cpu().numpy() if points else None)


def test_seventy_thousand_image_pairs(engine):
    """M = 70000 slots (grid.x > 65535) of a 40-entry list at stride 64, one sample each: every slot's count lies in its
    interval, slots 0, 65535, 65536 and 69999 have the bits of their M = 1 probes.  pgx_pose_dev on the same slots with one
    matrix gives the same bits in every slot (the votes are integer atomics, everything else is one thread's work)."""
    M, n, stride, P, seed = 70000, 40, 64, 8, 41
    assert M > 65535
    scene = pr.two_views(200, 0, 700)
    p1, p2 = scene[0][:n], scene[1][:n]
    d = Lists([(p1, p2)], stride, slots=M)
    F, inl, bs = ransac(engine, d, 1, P, pr.THR, seed)
    assert len(np.unique(bits(F), axis=0)) > M // 2                # the slots run different streams
    res_ok = 0
    for m0 in range(0, M, 7000):                                   # the interval of tests/pose_ref.py, vectorised over slots
        Fm = F[m0:m0 + 7000].reshape(-1, 3, 3).astype(np.float64)
        ha = np.concatenate([p1.astype(np.float64), np.ones((n, 1))], 1)
        hb = np.concatenate([p2.astype(np.float64), np.ones((n, 1))], 1)
        terms = Fm[:, None, :, :] * ha[None, :, :, None] * hb[None, :, None, :]
        res, mag = terms.sum((2, 3)), np.abs(terms).sum((2, 3))
        g, thr = 8.0 * 2.0 ** -24 * mag, float(np.float32(pr.THR))
        lo, hi = (res <= thr - g).sum(1), (res <= thr + g).sum(1)
        c = inl[m0:m0 + 7000]
        none = c == -1
        # a sample without any inlier reports no matrix (zeros), so there is nothing to score: about 1.5 % of these subsets by
        # the oracle (the matrix as returned is the transpose of the fitting one, tests/test_pose_ref.py)
        assert (bs[m0:m0 + 7000][none] == -1).all() and (bits(F[m0:m0 + 7000][none]) == 0).all()
        assert (bs[m0:m0 + 7000][~none] == 0).all()
        assert ((lo <= c) & (c <= hi))[~none].all()
        res_ok += int((~none).sum())
    assert res_ok > 0.9 * M
    slots = [0, 65535, 65536, 69999]
    Fp, cp, bp = probe(engine, d, P, pr.THR, [(seed, m, 0) for m in slots])
    lo, hi = pr.count_interval(Fp[0], p1, p2, pr.THR)              # the scalar helper agrees with the vectorised form
    assert cp[0] == -1 or lo <= cp[0] <= hi
    for k, m in enumerate(slots):
        assert (bits(F[m]) == bits(Fp[k])).all() and inl[m] == cp[k] and bs[m] == bp[k], m
    Fo = pose_np.estimate_fundamental(scene[0], scene[1])
    Rt, v, b, pts = pose_call(engine, d, np.tile(Fo.reshape(1, 9), (M, 1)))
    bo, Ro, to, vo, _ = pose_np.estimate_pose(Fo, p1, p2)
    assert np.abs(v[0] - np.array(vo)).max() <= 3 and b[0] == bo and np.abs(Rt[0, :9].reshape(3, 3) - Ro).max() < 2e-3
    assert (bits(Rt) == bits(Rt[0])).all() and (v == v[0]).all() and (b == b[0]).all()
    assert (bits(pts) == bits(pts[0])).all() and (pts[0, n:] == np.float32(SENT_F)).all()


# -------------------------------------------------------------------------------------------------------- pgx_pose_dev shapes

POSE_N = (1, 255, 256, 257, 1025, 4097)


def test_pose_shapes_and_exact_properties(engine):
    """Lists of 1, 255, 256, 257, 1025 and 4097 entries (the 256-thread stride loop of k_pose: 1 to 17 passes) in one batch,
    a tenth of each longer list wrong entries, against pose_np.estimate_pose at the tolerances of tests/test_gpu_pose.py.
    Exact: d_points = NULL changes no bit elsewhere; rows of d_points at and past counts[a] keep their sentinel; d_best is the
    first maximum of d_votes; d_votes[best] is the number of cloud points with z >= 0; reordering the slots permutes the
    outputs.  The z band: z = R[2] . X + t[2] is 3 products and 3 additions, two float32 evaluations of it (the vote pass
    and the cloud pass) differ by at most 8 * 2^-24 * (|R[2]| . |X| + |t[2]|) (bounded as in tests/pose_ref.py's interval),
    X recovered from the cloud in float64; points inside the band may vote either way and must be fewer than 1 %."""
    stride = 4160
    sets, Fs = [], []
    for n in POSE_N:
        p1, p2 = pr.two_views(max(n, 200), 0, 800 + n)[:2]
        Fs.append(pose_np.estimate_fundamental(p1[:200], p2[:200]))
        p1, p2 = p1[:n].copy(), p2[:n].copy()
        if n >= 255:
            o1, o2 = pr.two_views(0, n // 10, 900 + n)[:2]
            p1[-len(o1):], p2[-len(o2):] = o1, o2
        sets.append((p1, p2))
    assert max(POSE_N) > 16 * 256 and max(POSE_N) < stride
    d = Lists(sets, stride)
    M = len(sets)
    Rt, v, b, pts = pose_call(engine, d, np.stack(Fs))
    Rt0, v0, b0, _ = pose_call(engine, d, np.stack(Fs), points=False)
    assert Rt0.tobytes() == Rt.tobytes() and (v0 == v).all() and (b0 == b).all()
    for m, (p1, p2) in enumerate(sets):
        n = len(p1)
        bo, Ro, to, vo, cloud = pose_np.estimate_pose(Fs[m], p1, p2)
        assert np.abs(v[m] - np.array(vo)).max() <= max(3, n // 50), (n, v[m], vo)
        assert (v[m] >= 0).all() and v[m].max() <= n and b[m] == int(np.argmax(v[m]))
        if sorted(vo)[-1] - sorted(vo)[-2] > max(3, n // 50):
            assert b[m] == bo
            assert np.abs(Rt[m, :9].reshape(3, 3) - Ro).max() < 2e-3 and np.abs(Rt[m, 9:] - to).max() < 2e-3
            good = np.abs(cloud).max(1) < 1e3
            assert np.abs(pts[m, :n][good] - cloud[good]).max() < 5e-2 * max(1.0, np.abs(cloud[good]).max())
        else:
            assert n == 1                                          # only the one-entry list has no clear winner
        assert (pts[m, n:] == np.float32(SENT_F)).all() and not (pts[m, :n] == np.float32(SENT_F)).all(1).any()
        R, t = Rt[m, :9].reshape(3, 3).astype(np.float64), Rt[m, 9:].astype(np.float64)
        X = (pts[m, :n].astype(np.float64) - t) @ R                # R^T (p - t)
        z = pts[m, :n, 2].astype(np.float64)
        band = 8.0 * 2.0 ** -24 * (np.abs(X) @ np.abs(R[2]) + abs(t[2]))
        fin = np.isfinite(z) & np.isfinite(band)
        near = fin & (np.abs(z) <= band)
        assert near.sum() <= 0.01 * n and (~fin).sum() <= 0.01 * n, (n, int(near.sum()), int((~fin).sum()))
        sure = int((fin & (z > band)).sum())
        assert sure <= v[m, b[m]] <= sure + int(near.sum()) + int((~fin).sum()), (n, sure, v[m])
    # the slots reordered: same frames, the lists and the matrices move with their slot
    order = [3, 5, 0, 4, 1, 2]
    d2 = Lists(sets, stride)
    d2.ml, d2.pl = d.ml[order].contiguous(), d.pl[order].contiguous()
    Rt2, v2, b2, pts2 = pose_call(engine, d2, np.stack(Fs)[order])
    assert Rt2.tobytes() == Rt[order].tobytes() and (v2 == v[order]).all() and (b2 == b[order]).all()
    assert bits(pts2).tobytes() == bits(pts[order]).tobytes()
    Fr2, ir2, br2 = ransac(engine, d2, 70, 8, pr.THR, 5)
    Fp, cp, bp = probe(engine, d2, 8, pr.THR, [(5, 1, int(br2[1]))])   # RANSAC too: slot 1 runs stream 1 on the list now in it
    assert ir2[1] == cp[0] and (bits(Fr2[1]) == bits(Fp[0])).all() and len(d2.sets[order[1]][0]) == 4097
