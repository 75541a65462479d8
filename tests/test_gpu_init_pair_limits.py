"""GPU tests of the initial pair (csrc/k_initpair.hip: pgx_init_pair_dev) past its chunk and grid limits: more than one scoring
workgroup per pair (split = ceil(stride / 2048) of 2, 3 and 4: blockIdx.x > 0, the stride of split * 256 entries, atomics from
up to 16 waves into one pair's counters), pair lists of more than 65535 pairs (the launcher's slices: nine offset pointers, and
k_init_pick reading the workspace and d_pair_stats across slices), ties of the choice's two keys across the waves and the
m += 256 passes of k_init_pick, the integer gates at equality, and mirrored x axes.  The launch rules restated are in
tests/verify_limits_cases.py (held to the source's text by tests/test_verify_limits_cases.py); every test asserts on the host,
from those rules, that its shape reaches the path it names.  Every comparison is an integer or bit-for-bit statement: the
yardstick's predicate on the candidates the device wrote (test_gpu_init_pair.check), or the device against itself.

Wall time on an MI355X: 1.5 s of pytest time for the file's 11 tests; the slowest are the three tie cases at 0.09 s each (three
calls of 600 pairs and the yardstick on one of them), a call of 65835 pairs with its host checks takes 0.04 to 0.07 s."""
import numpy as np
import pytest

import init_pair_ref as ref
import verify_limits_cases as vc
from geom_gpu import bits
from test_gpu_init_pair import K0, K1, KEYS, MAXD, NONE, PAIR_KEYS, check, pairs_case, pose_F, run, two_view

pytestmark = pytest.mark.gpu


def padded(kp, ml, stride):
    """the layout at a larger stride: zero keypoints and the (0, 0, PGX_DIST_NONE) tail behind what there is"""
    F, s0 = kp.shape[0], kp.shape[1]
    kq, mq = np.zeros((F, stride, 4), np.int32), np.zeros((len(ml), stride, 3), np.int32)
    mq[:, :, 2] = NONE
    kq[:, :s0], mq[:, :s0] = kp, ml
    return kq, mq


# ---- 1. more than one scoring workgroup per pair ----------------------------------------------------------------------------------

def test_three_scoring_workgroups_per_pair(engine):
    sizes = (1, 255, 2047, 2048, 2049, 4095, 4097)
    kp, counts, pl, ml, Fs, K = pairs_case(sizes, seed=101)
    stride = kp.shape[1]
    assert vc.init_split(stride) == 3 and 2 * vc.INIT_ROWS < stride <= 3 * vc.INIT_ROWS
    # every workgroup of the larger pairs has entries, and the workgroups come round again (e0 += split * 256)
    assert (counts[4::2] > 3 * vc.INIT_NT).all() and counts.max() > 2 * 3 * vc.INIT_NT
    got = run(engine, kp, counts, pl, ml, Fs, K)
    check(got, kp, counts, pl, ml, Fs, K)
    st = got["stats"]
    print("stride", stride, "stats", st.tolist())
    assert st[:, 0].tolist() == list(sizes)
    assert (st[1:, 7] == 0).all() and (st[1:, 1:5].max(1) >= 0.72 * st[1:, 0]).all()


# ---- 2. split invariance, bit for bit ---------------------------------------------------------------------------------------------

def test_identical_bits_at_one_to_four_workgroups_per_pair(engine):
    sizes = (1000, 513, 40, 257, 999)
    kp, counts, pl, ml, Fs, K = pairs_case(sizes, seed=102)
    rng = np.random.default_rng(103)
    Fs[1:] *= 1.0 + rng.normal(scale=2e-4, size=Fs[1:].shape)
    s0 = kp.shape[1]
    strides = (s0, 2049, 4100, 6145)
    assert [vc.init_split(s) for s in strides] == [1, 2, 3, 4]
    res = []
    for s in strides:
        kq, mq = padded(kp, ml, s)
        res.append(run(engine, kq, counts, pl, mq, Fs, K, angle=8.0))
    check(res[0], kp, counts, pl, ml, Fs, K, angle=8.0)
    assert res[0]["stats"][:, 0].tolist() == list(sizes) and res[0]["report"][1] >= 3
    for r in res[1:]:
        for k in KEYS:
            assert bits(res[0][k]) == bits(r[k]), k
    # counts[a] above the stride: clamped to the stride, so the whole padded list is walked and its tail is seen and rejected
    up = []
    for s in (s0, 6145):
        kq, mq = padded(kp, ml, s)
        cq = counts.copy()
        cq[0::2] = s + 5
        g = run(engine, kq, cq, pl, mq, Fs, K, angle=8.0)
        check(g, kq, cq, pl, mq, Fs, K, angle=8.0)
        up.append(g)
    for k in KEYS:
        assert bits(up[0][k]) == bits(up[1][k]), k
    assert (up[0]["stats"][:, 0] >= res[0]["stats"][:, 0]).all() and (up[0]["stats"][:, 0] <= counts[0::2]).all()


# ---- 3. more than 65535 pairs ------------------------------------------------------------------------------------------------------

T_COMBOS = 64
BIG_M = vc.INIT_SLICE + 300
BEST, SKIP, BAD = T_COMBOS, T_COMBOS + 1, T_COMBOS + 2     # rows of the small call behind the T tiled ones


def combos_case():
    """8 slots of 8 keypoints: slots 2i and 2i + 1 are two views of 8 points.  T (list, F, slots) combinations with at most 6
    candidates each, then one pair with all 8 (its slots' matches are all true: the best pair), a SKIPPED and a BADINPUT pair.
    -> (kp [8][8][4], counts [8], pl [T + 3], ml [T + 3][8][3], Fs [T + 3][9], K [8][4])"""
    rng = np.random.default_rng(104)
    kp, counts = np.zeros((8, 8, 4), np.int32), np.full(8, 8, np.int32)
    for i in range(4):
        pa, pb = two_view(rng, 8, K0, K1, junk=0.0 if i == 0 else 0.3)
        kp[2 * i, :, :2], kp[2 * i + 1, :, :2] = pa, pb
    K = np.array([K0, K1] * 4)
    ident = np.stack([np.arange(8), np.arange(8), np.full(8, 5)], 1)
    pl, ml, Fs = [], [], []
    for t in range(T_COMBOS):
        i = t % 4
        lst = ident.copy()
        lst[:, 2] = rng.integers(0, MAXD + 1, 8)
        for r in rng.permutation(8)[:2 + t % 3]:               # 2 to 4 rows that are no candidates
            lst[r] = [[lst[r, 0], -1, NONE], [0, 0, NONE], [8, lst[r, 1], 5], [lst[r, 0], 8, 5], [lst[r, 0], lst[r, 1], MAXD + 1]][rng.integers(0, 5)]
        pl.append((2 * i, 2 * i + 1))
        ml.append(lst[rng.permutation(8)])
        Fs.append(pose_F(K0, K1) * (1.0 + rng.normal(scale=2e-4, size=9)))
    pl += [(0, 1), (3, 3), (2, 3)]
    ml += [ident, ident, ident]
    Fs += [pose_F(K0, K1), pose_F(K0, K1), np.full(9, np.nan)]
    return kp, counts, pl, np.array(ml, np.int32), np.array(Fs), K


@pytest.fixture(scope="module")
def combos(engine):
    """the small call every large one is held to, checked against the yardstick once"""
    kp, counts, pl, ml, Fs, K = combos_case()
    small = run(engine, kp, counts, pl, ml, Fs, K, minpts=1)
    check(small, kp, counts, pl, ml, Fs, K, minpts=1)
    st = small["stats"]
    assert (st[:T_COMBOS, 0] <= 6).all() and st[BEST].tolist()[5:] == [8, st[BEST, 6], 0] and st[BEST, 0] == 8
    assert st[:T_COMBOS, 5].max() < st[BEST, 5] and (st[:T_COMBOS, 7] == 0).sum() >= T_COMBOS // 2
    assert st[SKIP, 7] == ref.SKIPPED and st[BAD, 7] == ref.BADINPUT
    return (kp, counts, pl, ml, Fs, K), small


@pytest.mark.parametrize("where", ["65534", "65535", "last", "tie"])
def test_more_pairs_than_one_slice(engine, combos, where):
    """65835 pairs: two slices of 65535 and 300.  Every row is one of T + 3 pairs of a small call, and its outputs are that
    call's rows bit for bit; the report, the choice and the per-frame arrays are the yardstick's on the device's stats.  The
    unique best pair sits in the last row of the first slice, the first of the second, the last of all; or twice, at m = 100
    and m = 65600, where the smaller m wins.  SKIPPED and BADINPUT pairs sit on both sides of the slice edge."""
    (kp, counts, pl, ml, Fs, K), small = combos
    M = BIG_M
    assert M > vc.INIT_SLICE and vc.init_split(kp.shape[1]) == 1
    idx = np.arange(M) % T_COMBOS
    flagged = {65530: SKIP, 65533: BAD, 65540: SKIP, 65545: BAD, 17: SKIP, M - 2: BAD}
    assert any(m < vc.INIT_SLICE for m in flagged) and any(m >= vc.INIT_SLICE for m in flagged)
    for m, k in flagged.items():
        idx[m] = k
    best = {"65534": [65534], "65535": [65535], "last": [M - 1], "tie": [100, 65600]}[where]
    assert (where != "65534" or best[0] == vc.INIT_SLICE - 1) and (where != "65535" or best[0] == vc.INIT_SLICE)
    assert where != "tie" or best[0] < vc.INIT_SLICE <= best[1]
    idx[best] = BEST
    plM = np.asarray(pl, np.int32)[idx]
    got = run(engine, kp, counts, plM, ml[idx], Fs[idx], K, minpts=1)
    for k in PAIR_KEYS:
        assert bits(got[k]) == bits(small[k][idx]), k
    fa = np.where(got["stats"][:, 7] == ref.SKIPPED, -1, plM[:, 0])
    fb = np.where(got["stats"][:, 7] == ref.SKIPPED, -1, plM[:, 1])
    ms = ref.choose(got["stats"], fa, fb)
    assert ms == best[0] == got["report"][6]
    want = ref.report(got["stats"], ms)
    assert (got["report"] == want).all(), (got["report"], want)
    assert want[2] == len(flagged) and want[7] == 8
    Rt, P, fixed, reg = ref.frame_outputs(ms, fa, fb, got["Rt_pair"], K, None, 8, 8)
    assert bits(got["Rt_out"]) == bits(Rt) and bits(got["P_out"]) == bits(P)
    assert (got["fixed_out"] == fixed).all() and (got["register_out"] == reg).all()


# ---- 4. ties across the waves and passes of the choice -----------------------------------------------------------------------------

@pytest.mark.parametrize("m0", [599, 70, 300])
def test_ties_across_waves_and_passes_of_the_choice(engine, m0):
    """600 pairs with one list, one F and the same keypoints, so that every count is the same and the keys alone decide.  m0's
    thread of k_init_pick and its pass of the m += 256 loop: 599 -> thread 87 (wave 1), pass 2; 70 -> thread 70 (wave 1), pass
    0; 300 -> thread 44 (wave 0), pass 1.  (a) every pair in slots of its own, the smallest frame of a at m0; (b) one slot a,
    the smallest frame of b at m0; (c) one pair of slots in every row, the rows ahead of m0 SKIPPED: the smallest m is m0."""
    M = 600
    assert ((m0 % vc.INIT_NT) // 64, m0 // vc.INIT_NT) == {599: (1, 2), 70: (1, 0), 300: (0, 1)}[m0]
    kp1, c1, _, ml1, F1, _ = pairs_case((40,), seed=105)
    nslots = 2 * M
    kp = np.tile(kp1, (M, 1, 1))                             # slot 2m is view a, slot 2m + 1 view b
    counts = np.tile(c1, M)
    ml, Fs = np.tile(ml1, (M, 1, 1)), np.tile(F1, (M, 1))
    rng = np.random.default_rng(106 + m0)
    K = np.zeros((nslots, 4))

    def frames():
        """the numbers 1 .. M in a random order with the 1 at m0"""
        order = rng.permutation(M) + 1
        order[np.argmin(order)] = order[m0]
        order[m0] = 1
        return order

    # (a) the smaller frame of a
    ids = np.zeros(nslots, np.int32)
    ids[0::2], ids[1::2] = frames() - 1, M + rng.permutation(M)
    K[ids[0::2]], K[ids[1::2]] = K0, K1
    pl = [(2 * m, 2 * m + 1) for m in range(M)]
    got = run(engine, kp, counts, pl, ml, Fs, K, ids=ids, frac=0.5)
    check(got, kp, counts, pl, ml, Fs, K, ids=ids, frac=0.5)
    st = got["stats"]
    assert (st == st[0]).all() and st[0, 7] == 0 and int(np.argmin(ids[0::2])) == m0
    assert got["report"][6] == m0 == ref.choose(st, ids[0::2], ids[1::2])
    # (b) one slot a: the smaller frame of b
    ids[0::2], ids[1::2] = -1, frames()
    ids[0] = 0
    K[:] = K1
    K[0] = K0
    pl = [(0, 2 * m + 1) for m in range(M)]
    got = run(engine, kp, counts, pl, ml, Fs, K, ids=ids, frac=0.5)
    assert bits(got["stats"]) == bits(st) and int(np.argmin(ids[1::2])) == m0
    assert got["report"][6] == m0 == ref.choose(st, np.zeros(M, int), ids[1::2])
    assert got["fixed_out"].sum() == 1 and got["fixed_out"][0] == 1 and got["register_out"][1] == 0 and got["register_out"].sum() == M - 1
    # (c) one pair of slots: the smaller m among the rows that are not SKIPPED
    pl = [(0, 0) if m < m0 else (0, 1) for m in range(M)]
    got = run(engine, kp, counts, pl, ml, Fs, K, ids=ids, frac=0.5)
    assert (got["stats"][:m0, 7] == ref.SKIPPED).all() and bits(got["stats"][m0:]) == bits(st[m0:])
    assert got["report"][6] == m0 == ref.choose(got["stats"], np.zeros(M, int), np.full(M, ids[1]))
    assert got["report"].tolist() == [M, M - m0, m0, 0, 0, 0, m0, int(st[0, 5])]


# ---- 5. the gates at equality --------------------------------------------------------------------------------------------------------

def test_gates_at_equality(engine):
    sizes = (300, 120)
    kp, counts, pl, ml, Fs, K = pairs_case(sizes, seed=107)
    a = run(engine, kp, counts, pl, ml, Fs, K)
    check(a, kp, counts, pl, ml, Fs, K)
    st = a["stats"][0]
    n, best, wide = int(st[0]), int(st[1 + st[6]]), int(st[5])
    assert st[7] == 0 and 0 < best < n and wide >= 30
    at = np.float64(best) / np.float64(n)
    flip = at                                                # the smallest float64 at which the product exceeds best: the gate's edge
    while not np.float64(best) < flip * np.float64(n):
        flip = np.nextafter(flip, np.inf)
    assert at <= flip <= at * (1 + 8 * np.finfo(np.float64).eps) and flip <= 1.0
    for frac in (at, np.nextafter(at, np.inf), np.nextafter(at, 0.0), flip, np.nextafter(flip, 0.0)):
        g = run(engine, kp, counts, pl, ml, Fs, K, frac=float(frac))
        check(g, kp, counts, pl, ml, Fs, K, frac=float(frac))
        few = bool(np.float64(best) < np.float64(frac) * np.float64(n))     # the header's test, decided in float64
        print("min_front_frac", repr(float(frac)), "frac * n", repr(float(frac * n)), "best", best, "FEWFRONT", few)
        assert bool(g["stats"][0, 7] & ref.FEWFRONT) == few and g["stats"][0, :7].tolist() == st[:7].tolist()
    for minpts, few in ((wide, False), (wide + 1, True)):
        g = run(engine, kp, counts, pl, ml, Fs, K, minpts=minpts)
        check(g, kp, counts, pl, ml, Fs, K, minpts=minpts)
        assert bool(g["stats"][0, 7] & ref.FEWPOINTS) == few and g["stats"][0, :7].tolist() == st[:7].tolist()
    z = run(engine, kp, counts, pl, ml, Fs, K, angle=0.0)     # cos2 = 1: wide is (c s_a) s_b <= 0 or c c <= a11 a22
    check(z, kp, counts, pl, ml, Fs, K, angle=0.0)
    assert ref.cos2_of(0.0) == 1.0 and (z["stats"][:, :5] == a["stats"][:, :5]).all() and (z["stats"][:, 5] >= a["stats"][:, 5]).all()
    print("wide at 2 degrees", a["stats"][:, 5].tolist(), "at 0", z["stats"][:, 5].tolist(), "front", a["stats"][:, 1:5].tolist())


# ---- 6. mirrored axes ----------------------------------------------------------------------------------------------------------------

def test_counts_with_a_mirrored_x_axis_and_both_axes_mirrored(engine):
    """fx < 0 in one frame (s_a or s_b < 0: the sign tests turn the bearings, as for test_gpu_init_pair's fy < 0) and fx < 0 with
    fy < 0 in one frame (s > 0 again, the bearings mirrored in both axes)."""
    Kx, Kxy = K0 * [-1, 1, 1, 1], K0 * [-1, -1, 1, 1]
    n = 300
    Ks = [(Kx, K1), (K0, Kx), (Kxy, K1), (K0, Kxy), (Kx, Kxy), (K0, K1)]
    kp, counts, pl, ml, Fs, K = pairs_case((n,) * len(Ks), seed=108, Ks=Ks)
    assert [np.sign(a[0] * a[1]) for a, _ in Ks] == [-1, 1, 1, 1, -1, 1] and [np.sign(b[0] * b[1]) for _, b in Ks] == [1, -1, 1, 1, 1, 1]
    got = run(engine, kp, counts, pl, ml, Fs, K)
    check(got, kp, counts, pl, ml, Fs, K)
    st = got["stats"]
    print(st.tolist())
    assert (st[:, 0] == n).all()
    for m in range(len(Ks)):                                 # the true pose wins with the 80 % of true rows, whatever the signs
        assert st[m, 7] == 0 and st[m, 1 + st[m, 6]] >= 0.72 * n, (m, st[m])
