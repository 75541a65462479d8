"""GPU tests of two-view verification by epipolar RANSAC (pgx_verify_pairs_dev / pgx_verify_pair; include/pgx.h).  None of
them relies on the device's Jacobi solver and numpy's eigh agreeing on an eigenvector's last bits: the counts, the winner,
the inlier flags and the output lists are held to the yardstick's predicate (tests/verify_ref.py) evaluated on the F the
DEVICE wrote, as integers; the minimal solver is held to what a fundamental matrix is (its own 8 points, det, norm); the
refit to the yardstick's refit at 1e-8; and everything to itself, bit for bit, across runs, pair orders, chunkings, aliasing,
the host form and the optional outputs.

Data.  `mixed(n)`: n integer correspondences of which 70 % satisfy 2x + y - 2u - v + 37 = 0 exactly (an affine epipolar
geometry, F = [[0, 0, 2], [0, 0, 1], [-2, -1, 37]], rank 2) with half of those moved by up to 8 px in v (the
threshold of 1.5 px is 4.74 in v: the gradient of the relation has length sqrt(10)), and 30 % random: the counts of the
samples differ and many residuals sit near the threshold.  `exact(n)`: all n satisfy the relation exactly.
The minimal-solver test runs on `exact` data for a reason that is a property of the algorithm, not of the device: 8 points
in general position fix the null vector of G exactly, but only correspondences of one two-view geometry make it rank 2;
otherwise step 8 of the fit (rank 2 enforced) moves F off its own 8 points by the third singular value (measured with the
yardstick on 8 rounded true matches of a synth scene: up to 8e-5 |h_a| |h_b|).  On exactly consistent points the step
changes nothing and the residual is the solver's rounding (yardstick: below 1e-9 |h_a| |h_b| over 12000 samples)."""
import ctypes as C

import numpy as np
import pytest
import torch

import photogrammetry_amd as pg
import tracks_split_ref as ts
import verify_ref as ref
from geom_gpu import DEV, F64, I32, bits, run_tracks, summary_dict
from photogrammetry_amd import synth

pytestmark = pytest.mark.gpu

NONE = ref.DIST_NONE
F32 = dict(dtype=torch.float32, device=DEV)
KEYS = ("out", "F", "F32", "stats", "inlier", "sample_F", "sample_count", "report")
REQUIRED = ("out", "F", "stats", "report")
MAXD, IP, MIN_IN, SEED = 64, 1.5, 24, 7


def kp_array(kps, stride):
    """per slot [n][2] (x, y) -> int32 [F][stride][4]"""
    kp = np.zeros((len(kps), stride, 4), np.int32)
    for f, k in enumerate(kps):
        kp[f, :len(k), :2] = np.asarray(k).reshape(-1, 2)
    return kp


def run(engine, kp, counts, pl, ml, max_dist=MAXD, ns=256, ip=IP, mi=MIN_IN, it=2, seed=SEED, alias=False, optional=True):
    """pgx_verify_pairs_dev on the context's stream, one sync -> dict of host arrays (outputs pre-filled with sentinels)"""
    M, stride = len(pl), kp.shape[1]
    M1 = max(M, 1)
    d_kp = torch.from_numpy(np.ascontiguousarray(kp, np.int32)).to(DEV)
    d_c = torch.tensor(np.asarray(counts, np.int32), **I32)
    d_pl = torch.tensor(np.asarray(pl, np.int32).reshape(-1, 2) if M else np.zeros((1, 2), np.int32), **I32)
    d_ml = torch.from_numpy(np.ascontiguousarray(ml, np.int32).reshape(M1, stride, 3)).to(DEV)
    out = d_ml if alias else torch.full((M1, stride, 3), 77, **I32)
    Fd, Ff = torch.full((M1, 9), 5.0, **F64), torch.full((M1, 9), 5.0, **F32)
    stats, inl, rep = torch.full((M1, 8), 9, **I32), torch.full((M1, stride), 9, **I32), torch.full((8,), 7, **I32)
    sF, sc = torch.full((M1, ns, 9), 5.0, **F64), torch.full((M1, ns), 9, **I32)
    torch.cuda.synchronize()
    engine.verify_pairs_dev(d_kp, d_ml, d_c, d_pl, M, stride, max_dist, out, Fd, stats, rep, ns, ip, mi, it, seed,
                            d_F32=Ff if optional else None, d_inlier=inl if optional else None,
                            d_sample_F=sF if optional else None, d_sample_count=sc if optional else None)
    engine.check_status()
    return dict(out=out.cpu().numpy(), F=Fd.cpu().numpy(), F32=Ff.cpu().numpy(), stats=stats.cpu().numpy(),
                inlier=inl.cpu().numpy(), sample_F=sF.cpu().numpy(), sample_count=sc.cpu().numpy(), report=rep.cpu().numpy())


def relation(rng, n, consistent, jitter):
    """n integer correspondences: a fraction `consistent` on 2x + y - 2u - v + 37 = 0, half of those moved by up to 8 px in v
    when jitter; the rest random -> (pa [n][2], pb [n][2])"""
    x, y, u = rng.integers(0, 1920, n), rng.integers(0, 1080, n), rng.integers(0, 1920, n)
    v = 2 * x + y - 2 * u + 37
    if jitter:
        v = v + np.where(rng.random(n) < 0.5, rng.integers(-8, 9, n), 0)
    junk = rng.random(n) >= consistent
    v = np.where(junk, rng.integers(-3000, 5000, n), v)
    return np.stack([x, y], 1), np.stack([u, v], 1)


def pairs_case(ns_list, seed, consistent=0.7, jitter=True):
    """One image pair per entry n of ns_list, in slots (2m, 2m + 1): n candidates in shuffled rows -> (kp, counts, pl, ml)"""
    rng = np.random.default_rng(seed)
    stride = max(ns_list)
    kps, counts, pl, ml = [], [], [], np.zeros((len(ns_list), stride, 3), np.int32)
    ml[:, :, 2] = NONE
    for m, n in enumerate(ns_list):
        pa, pb = relation(rng, n, consistent, jitter)
        perm = rng.permutation(n)
        kb = np.zeros_like(pb)
        kb[perm] = pb
        kps += [pa, kb]
        counts += [n, n]
        pl.append((2 * m, 2 * m + 1))
        order = rng.permutation(n)
        ml[m, :n] = np.stack([order, perm[order], rng.integers(0, MAXD + 1, n)], 1)
    return kp_array(kps, stride), np.array(counts, np.int32), pl, ml


def cand_points(kp, counts, pl, ml, m, max_dist=MAXD):
    a, b = pl[m]
    return ref.candidates(kp[a, :, :2], kp[b, :, :2], counts[a], counts[b], ml[m], kp.shape[1], max_dist)


# ---- 1. scoring is exact -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("ns,sizes", [(1, (8, 256, 1025)), (255, (9, 255, 513)), (256, (256, 257, 8)), (257, (257, 513, 9)),
                                      (1000, (1025, 255, 8))])
def test_sample_counts_are_the_predicate_on_the_device_F(engine, ns, sizes):
    kp, counts, pl, ml = pairs_case(sizes, seed=ns)
    got = run(engine, kp, counts, pl, ml, ns=ns)
    valid = 0
    for m, n in enumerate(sizes):
        e, pa, pb, rows = cand_points(kp, counts, pl, ml, m)
        assert got["stats"][m, 0] == n == len(e)
        for s in range(ns):
            Fs, c = got["sample_F"][m, s], got["sample_count"][m, s]
            if np.isfinite(Fs).all():
                assert c == ref.predicate(Fs, pa, pb, IP).sum(), (m, s)
                valid += 1
            else:
                assert np.isnan(Fs).all() and c == -1, (m, s)
        assert got["stats"][m, 6] == (got["sample_count"][m] >= 0).sum()
    assert valid >= 0.9 * ns * len(sizes)
    print("ns", ns, "sizes", sizes, "valid samples", valid, "winner counts", got["stats"][:, 1].tolist())


# ---- 2. the minimal solver ------------------------------------------------------------------------------------------------------

def test_minimal_solver_on_exact_correspondences(engine):
    sizes, ns = (8, 9, 257), 300
    kp, counts, pl, ml = pairs_case(sizes, seed=11, consistent=1.0, jitter=False)
    got = run(engine, kp, counts, pl, ml, ns=ns, mi=8)
    worst = [0.0, 0.0, 0.0]
    for m, n in enumerate(sizes):
        e, pa, pb, rows = cand_points(kp, counts, pl, ml, m)
        a, b = pl[m]
        nvalid = 0
        for s in range(ns):
            Fs = got["sample_F"][m, s]
            if not np.isfinite(Fs).all():
                continue
            nvalid += 1
            ids = ref.sample(SEED, a, b, s, n)
            ha, hb = np.c_[pa[ids], np.ones(8)], np.c_[pb[ids], np.ones(8)]
            F = Fs.reshape(3, 3)
            r = np.abs(((ha @ F) * hb).sum(1)) / (np.linalg.norm(ha, axis=1) * np.linalg.norm(hb, axis=1))
            worst = [max(worst[0], r.max()), max(worst[1], abs(np.linalg.det(F))), max(worst[2], abs(np.sqrt((F * F).sum()) - 1))]
            assert r.max() <= 1e-7, (m, s, r.max())
            assert abs(np.linalg.det(F)) <= 1e-9, (m, s)
            assert abs(np.sqrt((F * F).sum()) - 1.0) <= 1e-12, (m, s)
            assert got["sample_count"][m, s] == n       # every candidate lies on the geometry the 8 fix
        assert nvalid >= 0.9 * ns, (m, nvalid)
    print("own-8 residual / (|ha| |hb|), |det F|, | |F| - 1 |: worst", worst)


def test_minimal_solver_on_general_correspondences(engine):
    """Inconsistent data (`mixed`): det and norm hold on every valid sample (rank 2 is enforced, the norm is divided out), and
    the residuals of a sample's own 8 points -- not zero here, see the module's docstring -- are the yardstick's fit of the
    same 8 points to the 1e-7 |h_a| |h_b| of the exact case.  That comparison is made where both of the fit's eigenvectors
    are well conditioned: an eigenvector computed in float64 by two different solvers agrees to about 100 eps / gap (gap =
    distance of the two smallest eigenvalues over the largest; 100 for the rotations of a Jacobi run), which is 1e-9 at a gap
    of 1e-5 and leaves the bound a factor of 100.  The yardstick puts 97 % of this data's samples above that gap; the test
    wants 90 %.  F is compared up to its sign (the sign rule can tie)."""
    ns, n = 300, 300
    kp, counts, pl, ml = pairs_case((n,), seed=12)
    got = run(engine, kp, counts, pl, ml, ns=ns)
    ok = np.isfinite(got["sample_F"][0]).all(1)
    Fs = got["sample_F"][0][ok].reshape(-1, 3, 3)
    assert len(Fs) >= 0.9 * ns
    assert np.abs(np.linalg.det(Fs)).max() <= 1e-9 and np.abs(np.sqrt((Fs * Fs).sum((1, 2))) - 1.0).max() <= 1e-12
    e, pa, pb, rows = cand_points(kp, counts, pl, ml, 0)
    compared, worst, largest = 0, 0.0, 0.0
    for s in np.flatnonzero(ok):
        ids = ref.sample(SEED, pl[0][0], pl[0][1], int(s), n)
        gaps = []
        Fy = ref.fit(pa[ids], pb[ids], gaps)
        if Fy is None or min(gaps) < 1e-5:
            continue
        compared += 1
        ha, hb = np.c_[pa[ids], np.ones(8)], np.c_[pb[ids], np.ones(8)]
        sc = np.linalg.norm(ha, axis=1) * np.linalg.norm(hb, axis=1)
        rd, ry = ((ha @ got["sample_F"][0, s].reshape(3, 3)) * hb).sum(1) / sc, ((ha @ Fy) * hb).sum(1) / sc
        d = min(np.abs(rd - ry).max(), np.abs(rd + ry).max())
        worst, largest = max(worst, d), max(largest, np.abs(rd).max())
        assert d <= 1e-7, (s, d, gaps)
    print("compared", compared, "of", int(ok.sum()), "worst residual difference", worst, "largest own-8 residual", largest)
    assert compared >= 0.9 * ns


# ---- 3. winner and outputs follow from the device's own numbers ---------------------------------------------------------------

def check_outputs(got, kp, counts, pl, ml, ns, ip=IP, mi=MIN_IN, max_dist=MAXD):
    stride = kp.shape[1]
    for m, (a, b) in enumerate(pl):
        e, pa, pb, rows = cand_points(kp, counts, pl, ml, m, max_dist)
        st, sc = got["stats"][m], got["sample_count"][m]
        assert st[0] == len(e) and st[7] == 0
        flags = 0
        if len(e) < 8:
            flags = ref.FEWMATCHES
        elif not (sc >= 0).any():
            flags = ref.NOMODEL
        if flags:
            assert st[3] == -1 and st[1] == 0 and st[2] == 0 and np.isnan(got["F"][m]).all()
        else:
            assert st[3] == int(np.argmax(sc)) and st[1] == sc.max()      # the first maximum
            if st[2] < mi:
                flags |= ref.FEWINLIERS
        assert st[4] == flags, (m, st)
        inl = np.full(stride, 9)
        inl[:rows] = -1
        inl[e] = ref.predicate(got["F"][m], pa, pb, ip)
        assert (got["inlier"][m] == inl).all(), m
        assert st[2] == (got["inlier"][m][:rows] == 1).sum() * (st[3] >= 0)
        want = np.full((stride, 3), 77)
        want[:rows] = ml[m, :rows]
        rej = ~((inl[:rows] == 1) & (flags == 0))
        want[:rows][rej, 1] = -1
        want[:rows][rej, 2] = NONE
        assert (got["out"][m] == want).all(), m
    assert np.array_equal(got["F32"], got["F"].astype(np.float32), equal_nan=True)
    assert (got["report"] == ref.report(got["stats"])).all(), (got["report"], ref.report(got["stats"]))


def test_winner_flags_lists_and_report_follow_from_the_device_numbers(engine):
    sizes = (600, 257, 40, 7, 1025)
    kp, counts, pl, ml = pairs_case(sizes, seed=21)
    got = run(engine, kp, counts, pl, ml, ns=300)
    check_outputs(got, kp, counts, pl, ml, 300)
    assert got["stats"][[0, 1, 3, 4], 4].tolist() == [0, 0, ref.FEWMATCHES, 0], got["stats"]
    assert (got["stats"][[0, 1, 4], 2] >= 0.35 * np.array([600, 257, 1025])).all(), got["stats"]    # the exact rows alone
    g2 = run(engine, kp, counts, pl, ml, ns=300, mi=10000)
    check_outputs(g2, kp, counts, pl, ml, 300, mi=10000)
    assert (g2["stats"][[0, 1, 2, 4], 4] == ref.FEWINLIERS).all() and np.isfinite(g2["F"][[0, 1, 2, 4]]).all()
    assert bits(g2["F"]) == bits(got["F"]) and bits(g2["inlier"]) == bits(got["inlier"])    # kept for FEWINLIERS
    assert (g2["out"][:, :, 1][g2["out"][:, :, 1] != 77] == -1).all() and g2["report"][1] == 0 and g2["report"][6] == 0


# ---- 4. refit ----------------------------------------------------------------------------------------------------------------------

def test_refit(engine):
    sizes = (600, 300, 1025)
    kp, counts, pl, ml = pairs_case(sizes, seed=31)
    g0 = run(engine, kp, counts, pl, ml, it=0)
    g2 = run(engine, kp, counts, pl, ml, it=2)
    assert bits(g0["sample_F"]) == bits(g2["sample_F"]) and bits(g0["sample_count"]) == bits(g2["sample_count"])
    for m in range(len(sizes)):
        win = g0["stats"][m, 3]
        assert win >= 0 and bits(g0["F"][m]) == bits(g0["sample_F"][m, win])
        assert g0["stats"][m, 5] == 0 and g0["stats"][m, 2] == g0["stats"][m, 1]
        st = g2["stats"][m]
        assert st[3] == win and st[1] == g0["stats"][m, 1] and st[2] >= st[1] and 0 <= st[5] <= 2
        assert (st[5] > 0) == (st[2] > st[1]) == (bits(g2["F"][m]) != bits(g0["F"][m]))
        e, pa, pb, rows = cand_points(kp, counts, pl, ml, m)
        Fr, cr, kr = ref.refit(g0["F"][m].reshape(3, 3), int(st[1]), pa, pb, IP, 2)
        Fr = np.asarray(Fr).reshape(9)
        d = min(np.abs(g2["F"][m] - Fr).max(), np.abs(g2["F"][m] + Fr).max())
        print("pair", m, "winner", st[1], "final", st[2], "kept", st[5], "yardstick", cr, kr, "|dF|", d)
        assert st[5] == kr and st[2] == cr
        assert d <= 1e-8
    assert (g2["stats"][:, 5] > 0).any()


# ---- 5. candidates and flags -----------------------------------------------------------------------------------------------------

def test_candidates_and_flags(engine):
    rng = np.random.default_rng(41)
    n, stride = 40, 64
    pa, pb = relation(rng, n, 1.0, False)
    xe = rng.integers(0, 1920, stride - n)          # 24 more keypoints for slot 2, on the geometry with b's keypoints 0 .. 23
    pa2 = np.concatenate([pa, np.stack([xe, pb[:stride - n, 1] - 2 * xe + 2 * pb[:stride - n, 0] - 37], 1)])
    kps = [pa, pb, pa2, pb, pa, pb, pa[:7], pb, pa[:8], pb, np.tile([[100, 200]], (20, 1)), np.tile([[300, 400]], (20, 1))]
    counts = np.array([n, n, stride + 5, n, -3, n, 7, n, 8, n, 20, 20], np.int32)
    pl = [(0, 1), (2, 3), (4, 5), (3, 4), (6, 7), (8, 9), (10, 11)]
    ml = np.zeros((len(pl), stride, 3), np.int32)
    ml[:, :, 2] = NONE                                        # the (0, 0, PGX_DIST_NONE) tail
    ident = np.stack([np.arange(n), np.arange(n), np.full(n, 5)], 1)
    ml[:, :n] = ident
    # pair 0: rows that are not candidates; their keypoints, where valid, are off the geometry (k2 = k1 + 1)
    ml[0, 3] = [3, -1, NONE]                                  # a rejected row of an NN list
    ml[0, 5] = [n, 5, 5]                                      # k1 out of range
    ml[0, 6] = [-1, 6, 5]
    ml[0, 7] = [7, n, 5]                                      # k2 out of range
    ml[0, 8] = [8, 9, MAXD + 1]                               # beyond max_dist
    ml[0, 9] = [9, 9, MAXD]                                   # at max_dist: a candidate
    ml[0, 10] = [10, 11, NONE]
    not_cand = [3, 5, 6, 7, 8, 10]
    ml[1, n:stride] = np.stack([np.arange(n, stride), np.arange(stride - n), np.full(stride - n, 5)], 1)   # counts > stride
    ml[4, :7], ml[5, :8] = ident[:7], ident[:8]
    ml[4, 7:n], ml[5, 8:n] = [0, 0, NONE], [0, 0, NONE]
    ml[6, :20], ml[6, 20:n] = ident[:20], [0, 0, NONE]
    kp = kp_array(kps, stride)
    got = run(engine, kp, counts, pl, ml, ns=64, mi=8)
    check_outputs(got, kp, counts, pl, ml, 64, mi=8)
    st = got["stats"]
    assert st[0, 0] == n - len(not_cand) and (got["inlier"][0, not_cand] == -1).all() and got["inlier"][0, 9] == 1
    assert st[0, 4] == 0 and (got["sample_count"][0][got["sample_count"][0] >= 0] == st[0, 0]).all()   # none entered a sample
    assert (got["inlier"][0, n:] == 9).all() and (got["out"][0, n:] == 77).all()                       # beyond counts[a]
    assert st[1, 0] == stride and st[1, 4] == 0 and (got["inlier"][1] == 1).all()    # counts[a] above stride: stride rows, k1 < stride
    assert tuple(st[2]) == (0, 0, 0, -1, ref.FEWMATCHES, 0, 0, 0) and (got["out"][2] == 77).all() and (got["inlier"][2] == 9).all()
    assert tuple(st[3]) == (0, 0, 0, -1, ref.FEWMATCHES, 0, 0, 0) and (got["inlier"][3, :n] == -1).all()   # counts[b] negative
    assert (got["out"][3, :n, 1] == -1).all() and (got["out"][3, :n, 0] == np.arange(n)).all()
    assert tuple(st[4]) == (7, 0, 0, -1, ref.FEWMATCHES, 0, 0, 0) and np.isnan(got["F"][4]).all()
    assert (got["out"][4, :7, 1] == -1).all() and (got["out"][4, :7, 2] == NONE).all() and (got["inlier"][4, :7] == 0).all()
    assert st[5, 0] == 8 and st[5, 4] == 0 and st[5, 2] == 8 and (got["out"][5, :8] == ident[:8]).all()
    assert tuple(st[6]) == (20, 0, 0, -1, ref.NOMODEL, 0, 0, 0) and np.isnan(got["F"][6]).all() and (got["sample_count"][6] == -1).all()
    assert got["report"].tolist() == [7, 3, 3, 1, 0, int(st[:, 0].sum()), int(st[[0, 1, 5], 2].sum()), 0]


# ---- 6. invariance, bit for bit ---------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def scene40():
    """8 frames of a synth scene, 40 of its ordered pairs, 30 % of the true rows relinked"""
    nf = 8
    pairs = [(a, b) for a in range(nf) for b in range(nf) if a != b][:40]
    s = synth.make_scene(260, nf, seed=5, pairs=pairs, wrong_rate=0.3)
    stride = int(s["counts"].max()) + 3
    ml = np.zeros((len(pairs), stride, 3), np.int32)
    ml[:, :, 2] = NONE
    for m, l in enumerate(s["lists"]):
        ml[m, :len(l)] = np.stack([l["k1"], l["k2"], l["dist"]], 1)
    kp = kp_array([np.stack([k["x"], k["y"]], 1) for k in s["kps"]], stride)
    return s, kp, s["counts"].astype(np.int32), pairs, ml


def test_identical_bits_across_runs_orders_chunks_alias_host_and_null_outputs(engine, scene40):
    s, kp, counts, pl, ml = scene40
    ns = 2000                                   # two chunks of samples at 40 pairs per workspace, one at 16
    a = run(engine, kp, counts, pl, ml, ns=ns)
    assert (a["stats"][:, 4] == 0).sum() >= 30 and (a["stats"][:, 5] > 0).any(), a["stats"]
    b = run(engine, kp, counts, pl, ml, ns=ns)
    for k in KEYS:
        assert bits(a[k]) == bits(b[k]), k
    perm = np.random.default_rng(1).permutation(len(pl))
    c = run(engine, kp, counts, [pl[i] for i in perm], ml[perm], ns=ns)
    for k in KEYS[:-1]:
        assert bits(a[k][perm]) == bits(c[k]), k
    assert bits(a["report"]) == bits(c["report"])
    other = pg.Engine(0)                        # a context of its own: the shared one keeps its chunking
    try:
        other.set_match_chunk(16)
        d = run(other, kp, counts, pl, ml, ns=ns)
    finally:
        other.close()
    for k in KEYS:
        assert bits(a[k]) == bits(d[k]), k
    e = run(engine, kp, counts, pl, ml, ns=ns, alias=True)
    for k in KEYS[1:]:
        assert bits(a[k]) == bits(e[k]), k
    for m, (fa, fb) in enumerate(pl):           # in place: the rows the stage writes, the input behind them
        assert (e["out"][m, :counts[fa]] == a["out"][m, :counts[fa]]).all() and (e["out"][m, counts[fa]:] == ml[m, counts[fa]:]).all()
    f = run(engine, kp, counts, pl, ml, ns=ns, optional=False)
    for k in REQUIRED:
        assert bits(a[k]) == bits(f[k]), k
    assert (f["inlier"] == 9).all() and (f["sample_count"] == 9).all() and (f["F32"] == 5.0).all()
    m = pl.index((1, 2))                        # the host form runs its pair in slots (1, 2)
    n1, n2 = counts[1], counts[2]
    h = engine.verify_pair(s["kps"][1], s["kps"][2], ml[m, :n1], MAXD, ns, IP, MIN_IN, 2, SEED)
    assert bits(h["F"]) == bits(a["F"][m]) and bits(h["stats"]) == bits(a["stats"][m])
    assert bits(h["inlier"]) == bits(a["inlier"][m, :n1])
    assert (np.stack([h["out"]["k1"], h["out"]["k2"], h["out"]["dist"]], 1) == a["out"][m, :n1]).all()


def test_a_shorter_last_chunk_of_pairs_fits_the_workspace(engine):
    """257 pairs in chunks of 129: the last chunk has 128 pairs, for which 2^16 cells are 512 samples per pair against 256
    for the 129 of the first.  Every launch must use the chunking the workspace was sized for; the results are those of one
    chunk of 257 pairs."""
    kp, counts, pl, ml = pairs_case([24 + m % 17 for m in range(257)], seed=61)
    a = run(engine, kp, counts, pl, ml, ns=512)
    other = pg.Engine(0)
    try:
        other.set_match_chunk(129)
        b = run(other, kp, counts, pl, ml, ns=512)
    finally:
        other.close()
    for k in KEYS:
        assert bits(a[k]) == bits(b[k]), k
    check_outputs(b, kp, counts, pl, ml, 512)


# ---- 7. truth and the chain --------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("seed", [0, 3])        # the seeds tests/test_verify_ref.py records for the yardstick
def test_recall_junk_and_true_epipolar_lines(engine, seed):
    c = ref.scene_pair(seed, 400, 170)
    kp = kp_array(c["kps"], c["stride"])
    got = run(engine, kp, c["counts"], [(c["a"], c["b"])], c["ml"][None], ns=256, it=2)
    inl = got["inlier"][0]
    t_in, j_in = (inl[c["true"]] == 1).sum(), (inl[c["junk"]] == 1).sum()
    da, db = ref.epipolar_distance(got["F"][0], c["uv_a"], c["uv_b"])
    print("seed", seed, "stats", got["stats"][0].tolist(), "true kept", t_in, "junk kept", j_in, "line distance", da.max(), db.max())
    assert got["stats"][0, 4] == 0
    assert t_in >= 0.99 * 400 and j_in <= 0.03 * 170
    assert max(da.max(), db.max()) <= 1.0       # the lines of F at the true (unrounded) matches
    cj = ref.scene_pair(seed, 0, 300)
    gj = run(engine, kp_array(cj["kps"], cj["stride"]), cj["counts"], [(cj["a"], cj["b"])], cj["ml"][None], ns=256, it=2)
    assert gj["stats"][0, 4] == ref.FEWINLIERS and (gj["out"][0, :cj["counts"][cj["a"]], 1] == -1).all(), gj["stats"]


def chain_case():
    """6 frames of a synth scene, the lists of consecutive frames with 30 % of the true rows relinked to a wrong keypoint"""
    nf = 6
    pairs = [(a, a + 1) for a in range(nf - 1)]
    s = synth.make_scene(400, nf, seed=3, pairs=pairs, wrong_rate=0.3)
    stride = int(s["counts"].max())
    ml = np.zeros((len(pairs), stride, 3), np.int32)
    ml[:, :, 2] = NONE
    for m, l in enumerate(s["lists"]):
        ml[m, :len(l)] = np.stack([l["k1"], l["k2"], l["dist"]], 1)
    return s, pairs, stride, ml


def test_verified_lists_give_a_better_track_graph(engine):
    s, pairs, stride, ml = chain_case()
    counts = s["counts"].astype(np.int32)
    kps = [np.stack([k["x"], k["y"]], 1).astype(np.float64) for k in s["kps"]]
    # the yardstick first
    res, _ = ref.verify(kps, counts, pairs, ml, stride, MAXD, 256, IP, MIN_IN, 2, SEED)
    yout = ml.copy()
    for m, r in enumerate(res):
        yout[m, :len(r["out"])] = r["out"]
    y_raw, y_ver = ts.arrays(counts, pairs, ml, stride, MAXD, [])[3], ts.arrays(counts, pairs, yout, stride, MAXD, [])[3]
    assert y_ver["dropped"] < y_raw["dropped"] and y_ver["n_nodes"] >= y_raw["n_nodes"], (y_raw, y_ver)
    got = run(engine, kp_array(kps, stride), counts, pairs, ml, ns=256, it=2)
    assert (got["stats"][:, 4] == 0).all()
    raw = summary_dict(run_tracks(engine, counts, pairs, ml, stride, MAXD)[3])
    ver = summary_dict(run_tracks(engine, counts, pairs, got["out"], stride, MAXD)[3])
    print("raw", raw, "verified", ver)
    assert ver["dropped"] < raw["dropped"] and ver["n_nodes"] >= raw["n_nodes"]
    wrong = sum(int(((got["inlier"][m, :len(w)] == 1) & w).sum()) for m, w in enumerate(s["wrong"]))
    assert wrong <= 0.03 * sum(int(w.sum()) for w in s["wrong"])


def test_F32_guides_the_matcher_to_the_true_matches(engine):
    """match_nn -> verify -> match_guided (d_F32, 2 px band): every true match is found again.  Descriptors: one random
    256-bit word per scene point, 20 bits flipped per view.  A winner that already holds every candidate gets no refit (no
    count is strictly greater), so F is an 8-point fit and a match at 1.5 px Sampson distance lies up to 2.1 px from its
    line; the scene's seed is one for which the yardstick's float32 F keeps every true match within 1.75 px (seeds 8 .. 23:
    1.4 to 2.2 px), which is checked first."""
    nf, words = 3, 8
    pairs = [(0, 1), (1, 2)]
    s = synth.make_scene(500, nf, seed=12, pairs=pairs)
    kf = [np.stack([k["x"], k["y"]], 1).astype(np.float64) for k in s["kps"]]
    for (a, b), l in zip(pairs, s["lists"]):
        y = ref.verify_pair(kf[a], kf[b], s["counts"][a], s["counts"][b], np.stack([l["k1"], l["k2"], l["dist"]], 1), a, b,
                            int(s["counts"].max()), 80, 256, IP, MIN_IN, 2, SEED)
        t = l["k2"] >= 0
        assert ref.epipolar_distance(y["F"].astype(np.float32).astype(np.float64), kf[a][l["k1"][t]], kf[b][l["k2"][t]])[1].max() <= 1.75
    rng = np.random.default_rng(2)
    base = rng.integers(0, 2**32, size=(500, words), dtype=np.uint32)
    stride, M = int(s["counts"].max()), len(pairs)
    desc = np.zeros((nf, stride, words), np.uint32)
    for f in range(nf):
        desc[f, :len(s["point_id"][f])] = synth.flip_bits(rng, base[s["point_id"][f]], 20)
    kp = kp_array([np.stack([k["x"], k["y"]], 1) for k in s["kps"]], stride)
    d_desc = torch.from_numpy(desc.view(np.int32)).to(DEV)
    d_kp, d_c = torch.from_numpy(kp).to(DEV), torch.tensor(s["counts"].astype(np.int32), **I32)
    d_pl = torch.tensor(np.asarray(pairs, np.int32), **I32)
    nn, ver, gd = (torch.full((M, stride, 3), 77, **I32) for _ in range(3))
    Fd, Ff, st, rep = torch.zeros((M, 9), **F64), torch.zeros((M, 9), **F32), torch.zeros((M, 8), **I32), torch.zeros(8, **I32)
    torch.cuda.synchronize()
    engine.match_nn_batch_dev(d_desc, d_c, stride, words, d_pl, M, nn, 80)
    engine.verify_pairs_dev(d_kp, nn, d_c, d_pl, M, stride, 80, ver, Fd, st, rep, 256, IP, MIN_IN, 2, SEED, d_F32=Ff)
    engine.match_guided_batch_dev(d_desc, d_kp, d_c, stride, words, d_pl, M, Ff, 2.0, gd, 80)
    engine.check_status()
    assert rep.cpu().tolist()[1] == M
    for m, l in enumerate(s["lists"]):
        true = l["k2"] >= 0
        g = gd.cpu().numpy()[m, :len(l)]
        assert (g[true, 1] == l["k2"][true]).all(), (m, (g[true, 1] != l["k2"][true]).sum())
        v = ver.cpu().numpy()[m, :len(l)]
        assert (v[true, 1] == l["k2"][true]).mean() >= 0.99


# ---- 8. immediate errors -----------------------------------------------------------------------------------------------------------

def test_errors(engine):
    bufs = {k: torch.zeros(n, **I32) for k, n in dict(kp=2 * 16 * 4, ml=16 * 3, c=2, pl=2, out=16 * 3, F=18, st=8, rep=8).items()}
    bufs["pl"][1] = 1
    t = bufs["kp"]
    L, h = engine._L, engine._h

    def raw(M=1, stride=16, ns=16, ip=1.5, mi=8, it=2, null=None):
        a = {k: C.c_void_p(v.data_ptr()) for k, v in bufs.items()}
        if null:
            a[null] = None
        return L.pgx_verify_pairs_dev(h, a["kp"], a["ml"], a["c"], a["pl"], M, stride, 64, ns, ip, mi, it, 1, a["out"], a["F"], None,
                                      a["st"], None, None, None, a["rep"])
    BAD = 5
    assert raw() == 0
    for kw in (dict(ns=0), dict(ns=65537), dict(ip=0.0), dict(ip=-1.0), dict(ip=float("nan")), dict(ip=float("inf")), dict(mi=7),
               dict(it=-1), dict(it=9), dict(M=-1), dict(stride=0), dict(stride=(1 << 20) + 1), dict(null="kp"), dict(null="ml"),
               dict(null="c"), dict(null="pl"), dict(null="out"), dict(null="F"), dict(null="st"), dict(null="rep")):
        assert raw(**kw) == BAD, kw
    torch.cuda.synchronize()
    engine.check_status()
    with pytest.raises(pg.ArgumentException):
        engine.verify_pairs_dev(t, bufs["ml"], bufs["c"], bufs["pl"], 1, 16, 64, bufs["out"], bufs["F"], bufs["st"], bufs["rep"], n_samples=0)
    with pytest.raises(pg.ArgumentException):
        engine.verify_pair(np.zeros(4, pg.KEYPOINT_DTYPE), np.zeros(4, pg.KEYPOINT_DTYPE), np.zeros((4, 3), np.int32), 64, min_inliers=3)
    # M = 0: nothing but the report
    kp, counts, pl, ml = pairs_case((16,), seed=1)
    g = run(engine, kp, counts, [], ml[:1], ns=16)
    assert g["report"].tolist() == [0] * 8 and (g["out"] == 77).all() and (g["stats"] == 9).all()
