"""GPU tests of two-view verification (csrc/k_verify.hip: pgx_verify_pairs_dev) past its chunk and grid limits: n_samples at the
API limit of 65536 and just under it (256 scoring workgroups, a partial last one, a partial last workgroup of k_ver_samples), all
four waves of k_ver_pick's merge with the winner's key in each of waves 1, 2 and 3, the running best across chunks of samples
with the winner in a later chunk and in an earlier one, the fourth chunk of a three-pair call whose other workgroups lie past
nblk, refit_iters at its limit of 8, the refit loop's exit below 8 inliers, min_inliers at equality, and slot numbers far
above the small ones of tests/test_gpu_verify.py.  The cases, the launch rules they restate and the host-side proof that the
late winners are where the sampler puts them are tests/verify_limits_cases.py and tests/test_verify_limits_cases.py; every
test asserts on the host, from those rules, that its shape reaches the path it names.  Every comparison is an integer or
bit-for-bit statement against the yardstick's predicate on the F the device wrote (verify_limits_cases.predicate_many, the
batch form of verify_ref.predicate), except the refit's F against verify_ref.refit, which keeps test_gpu_verify.test_refit's
1e-8.

Wall time on an MI355X: 2.2 s of pytest time for the file's 17 tests; the slowest is test_the_winner_in_the_third_chunk at
0.30 s (two calls of 3 x 65536 samples and the host's count of all of them), a one-pair call of 65536 samples with its host
check takes 0.09 to 0.15 s."""
import numpy as np
import pytest
import torch

import verify_limits_cases as vc
import verify_ref as ref
from geom_gpu import DEV, F64, I32, bits
from test_gpu_verify import IP, KEYS, MAXD, MIN_IN, REQUIRED, SEED, cand_points, check_outputs, pairs_case, run

pytestmark = pytest.mark.gpu

NS = vc.MAX_SAMPLES
N = 40                          # candidates per pair: they hardly matter to these paths and keep the host checks cheap


def count_check(got, kp, counts, pl, ml, ns, ip=IP):
    """every sample of every pair: a finite F has the yardstick's count of the device's F, a NaN F has -1; stats[6] counts the
    former -> the number of valid samples"""
    valid = 0
    for m in range(len(pl)):
        e, pa, pb, rows = cand_points(kp, counts, pl, ml, m)
        sF, sc = got["sample_F"][m], got["sample_count"][m]
        assert sF.shape == (ns, 9) and sc.shape == (ns,)
        fin = np.isfinite(sF).all(1)
        assert np.isnan(sF[~fin]).all() and (sc[~fin] == -1).all()
        want = vc.predicate_many(sF[fin], pa, pb, ip).sum(1)
        assert (sc[fin] == want).all(), (m, np.flatnonzero(sc[fin] != want)[:5])
        assert got["stats"][m, 6] == fin.sum() == (sc >= 0).sum()
        valid += int(fin.sum())
    return valid


# ---- 1. a sample is a pure function of (seed, a, b, s) ---------------------------------------------------------------------------

def probes(engine, kp, counts, pl, ml, seed, ss):
    """one call of one sample per s of ss, under the seed that makes sample 0 run the stream of sample s, back to back on the
    context's stream with one sync -> (sample_F [len(ss)][M][9], sample_count [len(ss)][M])"""
    M, stride, P = len(pl), kp.shape[1], len(ss)
    d_kp, d_c = torch.from_numpy(np.ascontiguousarray(kp, np.int32)).to(DEV), torch.tensor(np.asarray(counts, np.int32), **I32)
    d_pl, d_ml = torch.tensor(np.asarray(pl, np.int32), **I32), torch.from_numpy(np.ascontiguousarray(ml, np.int32)).to(DEV)
    out, Fd, st, rep = torch.zeros((M, stride, 3), **I32), torch.zeros((M, 9), **F64), torch.zeros((M, 8), **I32), torch.zeros(8, **I32)
    sF, sc = torch.full((P, M, 9), 5.0, **F64), torch.full((P, M), 9, **I32)
    torch.cuda.synchronize()
    for i, s in enumerate(ss):
        engine.verify_pairs_dev(d_kp, d_ml, d_c, d_pl, M, stride, MAXD, out, Fd, st, rep, 1, IP, MIN_IN, 0, vc.probe_seed(seed, s),
                                d_sample_F=sF[i], d_sample_count=sc[i])
    engine.check_status()
    return sF.cpu().numpy(), sc.cpu().numpy()


@pytest.mark.parametrize("M,chunk", [(1, 65536), (2, 32768), (3, 21760)])
def test_a_sample_is_a_pure_function_of_seed_slots_and_index(engine, M, chunk):
    """sample s of a call of 65536 samples against sample 0 of a one-sample call under seed ^ s * 0xD1B54A32D192ED03, at both
    sides of every edge: scoring workgroups (256), the waves of k_ver_pick (64 workgroups = 16384 samples), the chunks of
    samples (65536, 32768 or 21760 by the number of pairs) and, at three pairs, the fourth chunk of 256 samples, of whose 85
    scoring workgroups 84 lie past nblk."""
    assert vc.verify_chunk(M, NS) == chunk
    ss = {0, 63, 64, 255, 256, 16383, 16384, 32767, 32768, 49151, 49152, 65279, 65280, 65535}
    ss |= {k * chunk + d for k in range(1, 4) for d in (-1, 0) if k * chunk + d < NS}
    ss = sorted(ss)
    if M == 3:
        assert {21759, 21760, 43519, 43520, 65279, 65280} <= set(ss) and vc.pick_place(65280, chunk)[:2] == (3, 0)
        assert NS - 3 * chunk == vc.VER_NT and chunk // vc.VER_NT == 85 and (3 * chunk) // vc.VER_NT + 1 == -(-NS // vc.VER_NT)
    kp, counts, pl, ml = pairs_case((N,) * M, seed=70 + M)
    got = run(engine, kp, counts, pl, ml, ns=NS)
    pF, pc = probes(engine, kp, counts, pl, ml, SEED, ss)
    for i, s in enumerate(ss):
        for m in range(M):
            assert bits(got["sample_F"][m, s]) == bits(pF[i, m]) and got["sample_count"][m, s] == pc[i, m], (s, m)
    assert (pc >= 0).mean() >= 0.9
    check_outputs(got, kp, counts, pl, ml, NS)


# ---- 2. counts at the limit -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("ns", [65536, 65535, 65281])
def test_counts_at_the_sample_limit(engine, ns):
    """256 scoring workgroups of one pair in one chunk: all four waves of k_ver_pick hold keys.  65535 leaves the last scoring
    workgroup 255 samples and the last workgroup of k_ver_samples 63; 65281 leaves them one each."""
    assert vc.verify_chunk(1, ns) == 65536 and -(-ns // vc.VER_NT) == 256
    assert (ns % vc.VER_NT, ns % vc.VER_SNT) == {65536: (0, 0), 65535: (255, 63), 65281: (1, 1)}[ns]
    kp, counts, pl, ml = pairs_case((N,), seed=81)
    got = run(engine, kp, counts, pl, ml, ns=ns)
    valid = count_check(got, kp, counts, pl, ml, ns)
    assert valid >= 0.9 * ns
    sc, st = got["sample_count"][0], got["stats"][0]
    assert st[3] == int(np.argmax(sc)) and st[1] == sc.max() and st[0] == N
    check_outputs(got, kp, counts, pl, ml, ns)
    print("ns", ns, "valid", valid, "winner", st[3], "in workgroup", st[3] // vc.VER_NT, "count", st[1], "final", st[2])


# ---- 3. a late winner in every wave of the merge and in a later chunk -------------------------------------------------------------

def late(engine, slots, seed, chunk, places):
    """the late-winner data in `slots` under `seed`; places[m] = (chunk index, wave) the winner of pair m must be met in, None
    for any -> the winning samples"""
    M = len(slots)
    assert vc.verify_chunk(M, NS) == chunk
    first = [vc.first_all_good(seed, a, b, NS, vc.LATE_N, vc.LATE_G) for a, b in slots]
    for f, (want_chunk, want_wave) in zip(first, places):
        assert f >= 0
        c, b, wave, _ = vc.pick_place(f, chunk)
        assert c == want_chunk and want_wave in (None, wave), (f, c, b, wave)
    kp, counts, pl, ml, pts = vc.late_winner_case(slots)
    got = run(engine, kp, counts, pl, ml, ns=NS, mi=8, it=0, seed=seed, ip=vc.LATE_IP)
    st = got["stats"]
    print("slots", slots, "seed", seed, "first all-good", first, "stats", st.tolist())
    for m in range(M):
        assert st[m, 3] == first[m] and st[m, 1] >= vc.LATE_G and st[m, 0] == vc.LATE_N
        assert bits(got["F"][m]) == bits(got["sample_F"][m, first[m]]) and st[m, 4] == 0 and st[m, 5] == 0
        assert (got["inlier"][m, :vc.LATE_G] == 1).all()
    count_check(got, kp, counts, pl, ml, NS, ip=vc.LATE_IP)
    check_outputs(got, kp, counts, pl, ml, NS, ip=vc.LATE_IP, mi=8)
    bare = run(engine, kp, counts, pl, ml, ns=NS, mi=8, it=0, seed=seed, ip=vc.LATE_IP, optional=False)
    for k in REQUIRED:
        assert bits(got[k]) == bits(bare[k]), k
    assert (bare["sample_count"] == 9).all() and (bare["sample_F"] == 5.0).all()
    return first


@pytest.mark.parametrize("seed,wave", [(4, 1), (6, 2), (5, 3)])
def test_the_winner_in_each_later_wave_of_the_merge(engine, seed, wave):
    """One pair, one chunk of 256 scoring workgroups: the only key of its count sits in workgroup 90, 156 or 199, which thread
    90, 156 or 199 of k_ver_pick reads: s_key[1], s_key[2] or s_key[3] carries the winner to thread 0."""
    first = late(engine, ((0, 1),), seed, 65536, [(0, wave)])
    assert first == [vc.LATE_ONE[seed]] and wave * 64 <= first[0] // vc.VER_NT < (wave + 1) * 64


def test_the_winner_in_the_second_chunk_and_one_that_survives_it(engine):
    """Two pairs, chunks of 32768 samples: slots (0, 1) win in the second chunk (key > a.run[m] with s0 = 32768, the hypothesis
    at (s - s0) * 9), slots (2, 3) in the first chunk, in wave 1 of its merge, and the second chunk must not replace it."""
    L = vc.LATE_TWO
    first = late(engine, L["slots"], L["seed"], 32768, [(1, None), (0, 1)])
    assert first == list(L["first"]) and first[0] >= 32768 > first[1] >= 16384


def test_the_winner_in_the_third_chunk(engine):
    """Three pairs, chunks of 21760 samples and a fourth of 256: one winner in each of the first three chunks."""
    L = vc.LATE_THREE
    first = late(engine, L["slots"], L["seed"], 21760, [(1, None), (0, None), (2, None)])
    assert first == list(L["first"]) and 2 * 21760 <= first[2] < 3 * 21760


# ---- 4. threshold extremes as exact statements -----------------------------------------------------------------------------------

def test_a_threshold_that_admits_everything(engine):
    """inlier_px = 1e150 (T = 1e300, T d overflows to +inf for the larger d and e e <= +inf holds): every candidate with d > 0
    is an inlier of every valid sample, so each valid count is n, the winner is the first valid sample, no refit has a
    strictly greater count and the final count is n."""
    sizes, ns = (N, 300, 8, 1025), 300
    kp, counts, pl, ml = pairs_case(sizes, seed=91)
    got = run(engine, kp, counts, pl, ml, ns=ns, ip=1e150, mi=8)
    count_check(got, kp, counts, pl, ml, ns, ip=1e150)
    check_outputs(got, kp, counts, pl, ml, ns, ip=1e150, mi=8)
    for m, n in enumerate(sizes):
        sc, st = got["sample_count"][m], got["stats"][m]
        assert (sc[sc >= 0] == n).all() and (sc >= 0).any()
        assert st.tolist() == [n, n, n, int(np.flatnonzero(sc >= 0)[0]), 0, 0, int((sc >= 0).sum()), 0]
        assert bits(got["F"][m]) == bits(got["sample_F"][m, st[3]]) and (got["inlier"][m, :n] == 1).all()


@pytest.mark.parametrize("ip,consistent", [(1e-9, 0.3), (0.3, 0.0)])
def test_a_threshold_that_admits_next_to_nothing(engine, ip, consistent):
    """inlier_px = 1e-9 on junk-heavy data: a sample's own 8 points are off their rank-2 F by far more, so winners fall below 8
    inliers and the refit loop leaves at `cur < 8` before its first fit: no refit kept, the final count is the winner's, the
    pair is FEWINLIERS (min_inliers >= 8) and F is the winning sample's, bit for bit.  The same at 0.3 px on data with no
    consistent row at all, where the winners count a few inliers and not none (verify_ref on these lists: 4, 6, 6, 5 and 1; all 0 at 1e-9 px)."""
    sizes, ns = (N, 64, 300, 257, 9), 300
    kp, counts, pl, ml = pairs_case(sizes, seed=92, consistent=consistent)
    g8 = run(engine, kp, counts, pl, ml, ns=ns, ip=ip, mi=8, it=vc.MAX_REFITS)
    count_check(g8, kp, counts, pl, ml, ns, ip=ip)
    check_outputs(g8, kp, counts, pl, ml, ns, ip=ip, mi=8)
    st = g8["stats"]
    few = np.flatnonzero((st[:, 3] >= 0) & (st[:, 1] < 8))
    print("winner counts at", ip, "px", st[:, 1].tolist(), "pairs below 8 inliers:", len(few), "of", len(sizes))
    assert len(few) >= 1 and (ip != 0.3 or (st[few, 1] > 0).any())
    for m in few:
        assert st[m, 5] == 0 and st[m, 2] == st[m, 1] and st[m, 4] == ref.FEWINLIERS
        assert bits(g8["F"][m]) == bits(g8["sample_F"][m, st[m, 3]])
        assert (g8["out"][m, :sizes[m], 1] == -1).all()
    g0 = run(engine, kp, counts, pl, ml, ns=ns, ip=ip, mi=8, it=0)
    for k in KEYS[:-1]:                                     # all but the report: the refits did nothing
        assert bits(g0[k][few]) == bits(g8[k][few]), k


# ---- 5. refit at its limit ----------------------------------------------------------------------------------------------------------

def test_eight_refits(engine):
    """refit_iters = 8, the API's limit, on test_refit's sizes and one pair of more than 2048 candidates (the refit's lanes take
    more than 8 candidates each).  Count and refits kept are the yardstick's refit from the device's winner, F agrees at
    test_refit's 1e-8 up to sign, and over refit_iters = 0 .. 8 the final count never falls and a run whose loop left early
    (kept < k) is the next run bit for bit."""
    sizes = (600, 300, 1025, 2500)
    assert max(sizes) > 2048 and vc.MAX_REFITS == 8
    kp, counts, pl, ml = pairs_case(sizes, seed=31)
    g = [run(engine, kp, counts, pl, ml, it=k) for k in range(vc.MAX_REFITS + 1)]
    g0, g8 = g[0], g[8]
    check_outputs(g8, kp, counts, pl, ml, 256)
    worst = 0.0
    for m in range(len(sizes)):
        win = g0["stats"][m, 3]
        assert win >= 0 and bits(g0["F"][m]) == bits(g0["sample_F"][m, win]) and g0["stats"][m, 5] == 0
        st = g8["stats"][m]
        e, pa, pb, rows = cand_points(kp, counts, pl, ml, m)
        Fr, cr, kr = ref.refit(g0["F"][m].reshape(3, 3), int(st[1]), pa, pb, IP, vc.MAX_REFITS)
        Fr = np.asarray(Fr).reshape(9)
        d = min(np.abs(g8["F"][m] - Fr).max(), np.abs(g8["F"][m] + Fr).max())
        worst = max(worst, d)
        print("pair", m, "n", sizes[m], "winner", st[1], "final", st[2], "kept", st[5], "yardstick", cr, kr, "|dF|", d,
              "final by refit_iters", [int(x["stats"][m, 2]) for x in g], "kept", [int(x["stats"][m, 5]) for x in g])
        assert st[3] == win and st[1] == g0["stats"][m, 1] and 0 <= st[5] <= vc.MAX_REFITS
        assert st[5] == kr and st[2] == cr
        assert d <= 1e-8
        for k in range(vc.MAX_REFITS):
            a, b = g[k], g[k + 1]
            assert a["stats"][m, 2] <= b["stats"][m, 2] and a["stats"][m, 5] <= k
            assert bits(a["sample_F"][m]) == bits(b["sample_F"][m]) and bits(a["sample_count"][m]) == bits(b["sample_count"][m])
            if a["stats"][m, 5] < k:
                for key in ("out", "F", "F32", "stats", "inlier"):
                    assert bits(a[key][m]) == bits(b[key][m]), (m, k, key)
    print("worst |dF| at 8 refits", worst)
    assert (g8["stats"][:, 5] > 0).any()


# ---- 6. min_inliers at equality ----------------------------------------------------------------------------------------------------

def test_min_inliers_at_the_final_count(engine):
    sizes = (300, N)
    kp, counts, pl, ml = pairs_case(sizes, seed=95)
    a = run(engine, kp, counts, pl, ml)
    check_outputs(a, kp, counts, pl, ml, 256)
    c = int(a["stats"][0, 2])
    assert a["stats"][0, 4] == 0 and c >= MIN_IN and (a["out"][0, :sizes[0], 1] >= 0).sum() == c
    at = run(engine, kp, counts, pl, ml, mi=c)              # final count == min_inliers: accepted
    check_outputs(at, kp, counts, pl, ml, 256, mi=c)
    for k in ("out", "F", "F32", "stats", "inlier"):
        assert bits(at[k][0]) == bits(a[k][0]), k
    above = run(engine, kp, counts, pl, ml, mi=c + 1)       # one more: FEWINLIERS, rejected whole, F kept
    check_outputs(above, kp, counts, pl, ml, 256, mi=c + 1)
    assert above["stats"][0].tolist() == a["stats"][0, :4].tolist() + [ref.FEWINLIERS] + a["stats"][0, 5:].tolist()
    assert (above["out"][0, :sizes[0], 1] == -1).all() and (above["out"][0, :sizes[0], 2] == ref.DIST_NONE).all()
    assert bits(above["F"][0]) == bits(a["F"][0]) and bits(above["inlier"][0]) == bits(a["inlier"][0])


# ---- 7. slots -----------------------------------------------------------------------------------------------------------------------

def test_descending_and_large_slots(engine):
    """Pairs that name their slots in descending order and one pair in slots (70001, 70000) at stride 16 (an 18 MB keypoint
    array): a sample's 8 positions are verify_ref.sample's under those slots (the (uint32)a << 32 and b * C terms of the
    stream, and kp + slot * stride), held as test_minimal_solver_on_exact_correspondences holds them: on exact data the sample's
    own 8 points lie on its F to 1e-7 |h_a| |h_b| and every candidate is an inlier."""
    stride, ns, nslots = 16, 300, 70002
    pl = [(70001, 70000), (5, 2), (3, 1), (69999, 4)]
    assert all(a > b for a, b in pl) and nslots * stride * 16 > 17e6
    rng = np.random.default_rng(97)
    kp, counts = np.zeros((nslots, stride, 4), np.int32), np.zeros(nslots, np.int32)
    ml = np.zeros((len(pl), stride, 3), np.int32)
    ml[:, :, 2] = ref.DIST_NONE
    sizes = (16, 9, 12, 16)
    for m, ((a, b), n) in enumerate(zip(pl, sizes)):
        pa, pb = vc.on_relation(rng, n)
        perm = rng.permutation(n)
        kp[a, :n, :2], kp[b, perm, :2] = pa, pb
        counts[a] = counts[b] = n
        ml[m, :n] = np.stack([np.arange(n), perm, np.full(n, 5)], 1)
    got = run(engine, kp, counts, pl, ml, ns=ns, mi=8)
    check_outputs(got, kp, counts, pl, ml, ns, mi=8)
    worst = 0.0
    for m, ((a, b), n) in enumerate(zip(pl, sizes)):
        e, pa, pb, rows = cand_points(kp, counts, pl, ml, m)
        assert len(e) == n == got["stats"][m, 0]
        nvalid = 0
        for s in range(ns):
            Fs = got["sample_F"][m, s]
            if not np.isfinite(Fs).all():
                continue
            nvalid += 1
            ids = ref.sample(SEED, a, b, s, n)
            ha, hb = np.c_[pa[ids], np.ones(8)], np.c_[pb[ids], np.ones(8)]
            r = np.abs(((ha @ Fs.reshape(3, 3)) * hb).sum(1)) / (np.linalg.norm(ha, axis=1) * np.linalg.norm(hb, axis=1))
            worst = max(worst, r.max())
            assert r.max() <= 1e-7, (m, s, r.max())
            assert got["sample_count"][m, s] == n
        assert nvalid >= 0.9 * ns, (m, nvalid)
        assert got["stats"][m, 4] == 0 and got["stats"][m, 2] == n
    print("own-8 residual / (|ha| |hb|): worst", worst)
