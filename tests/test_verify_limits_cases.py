"""The helpers and cases of tests/verify_limits_cases.py are what tests/test_gpu_verify_limits.py and
tests/test_gpu_init_pair_limits.py take them for (no GPU): the restated launch rules equal the text of csrc/k_verify.hip,
csrc/k_initpair.hip and csrc/pgx_api.hip and the library's own pgx_verify_chunk; the batch predicate and the batch sampler
equal verify_ref's, bit for bit and draw for draw; and the hard-coded seeds of the late winners are where the sampler puts the
first all-good sample, so that a change to the sampler or to the builder fails here and not as a quietly shrunk GPU case."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import photogrammetry_amd._lib as L
import verify_limits_cases as vc
import verify_ref as ref
from ransac_ref import STREAM_MUL, stream_seed

CSRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "photogrammetry_amd", "csrc")


def constants(text):
    vals = {}
    for name, expr in re.findall(r"^constexpr (?:int|long long) (\w+) = ([^;]+);", text, flags=re.M):
        assert re.fullmatch(r"[\d\s<*+()-]+", expr), (name, expr)
        vals[name] = eval(expr)
    return vals


# ---- the mirrored launch facts -----------------------------------------------------------------------------------------------------

def test_constants_equal_the_kernel_sources():
    ver = open(os.path.join(CSRC, "k_verify.hip")).read()
    v = constants(ver)
    assert (v["VER_NT"], v["VER_SNT"], v["VER_CHUNK_CELLS"]) == (vc.VER_NT, vc.VER_SNT, vc.VER_CHUNK_CELLS)
    assert "return ransac_chunk(VER_CHUNK_CELLS, M, VER_NT, n_samples);" in ver
    # k_ver_pick: thread t reads the keys of scoring workgroups b0 + t, b0 + t + 256, ... of the chunk; lane 0 of each wave
    # hands its wave's key to thread 0; the running best moves on a strictly larger key and brings the chunk's hypothesis along
    assert "for (int b = b0 + threadIdx.x; b < b1; b += VER_NT)" in ver and "const int b0 = s0 / VER_NT;" in ver
    assert "for (int w = 1; w < VER_NT / 64; w++)" in ver and "if (key > a.run[m])" in ver
    assert "a.hyp + ((size_t)m * chunk + (s - s0)) * 9" in ver
    assert "dim3(chunk / VER_SNT, M), dim3(VER_SNT)" in ver and "dim3(chunk / VER_NT, M), dim3(VER_NT)" in ver
    assert "if (cur < 8) break;" in ver
    ini = open(os.path.join(CSRC, "k_initpair.hip")).read()
    i = constants(ini)
    assert (i["INIT_NT"], i["INIT_ROWS"]) == (vc.INIT_NT, vc.INIT_ROWS)
    assert "a.split = (stride + INIT_ROWS - 1) / INIT_ROWS;" in ini and "e0 += a.split * INIT_NT" in ini
    assert "for (int m0 = 0; m0 < M; m0 += %d)" % vc.INIT_SLICE in ini and "b.M = M - m0 < %d ? M - m0 : %d;" % (vc.INIT_SLICE, vc.INIT_SLICE) in ini
    assert "for (int m = threadIdx.x; m < a.M; m += INIT_NT)" in ini
    api = open(os.path.join(CSRC, "pgx_api.hip")).read()
    assert "n < 1 || n > %d ?" % vc.MAX_SAMPLES in api and 'iters_ok(c, "refit_iters", refit_iters, %d)' % vc.MAX_REFITS in api


def test_chunk_rule_equals_the_library():
    L.build()
    lib = C.CDLL(L.LIB_PATH)
    chunk_of = lib._Z16pgx_verify_chunkii
    chunk_of.restype, chunk_of.argtypes = C.c_int, [C.c_int, C.c_int]
    for M in (1, 2, 3, 4, 5, 40, 129, 255, 256, 257, 2048):
        for ns in (1, 255, 256, 257, 2000, 16384, 16385, 21760, 32768, 65281, 65535, 65536):
            assert vc.verify_chunk(M, ns) == chunk_of(M, ns), (M, ns)
    assert [vc.verify_chunk(M, 65536) for M in (1, 2, 3, 40)] == [65536, 32768, 21760, 1536]
    assert 65536 - 3 * 21760 == 256 == vc.VER_NT           # three pairs: a fourth chunk of one scoring workgroup
    assert vc.pick_place(23158, 65536) == (0, 90, 1, 0) and vc.pick_place(51091, 65536) == (0, 199, 3, 0)
    assert vc.pick_place(65535, 65536) == (0, 255, 3, 0) and vc.pick_place(65280, 21760) == (3, 0, 0, 0)
    assert vc.pick_place(37447, 32768) == (1, 18, 0, 0) and vc.pick_place(17977, 32768) == (0, 70, 1, 0)
    assert [vc.init_split(s) for s in (1, 2048, 2049, 4096, 4097, 6144, 6145)] == [1, 1, 2, 2, 3, 3, 4]


def test_probe_seed_runs_the_stream_of_sample_s():
    for seed, a, b, s, n in ((7, 0, 1, 65535, 40), (2**63 + 5, 70001, 70000, 16384, 9), (0, 3, 2, 1, 8)):
        assert vc.probe_seed(seed, s) == seed ^ (s * STREAM_MUL) % 2**64
        assert stream_seed(vc.probe_seed(seed, s), a, 0) == stream_seed(seed, a, s)
        assert ref.sample(vc.probe_seed(seed, s), a, b, 0, n) == ref.sample(seed, a, b, s, n)


# ---- the batch forms equal the yardstick's ------------------------------------------------------------------------------------------

def test_predicate_many_equals_the_predicate_row_by_row():
    rng = np.random.default_rng(1)
    n, S = 57, 400
    pa = np.stack([rng.integers(0, 1920, n), rng.integers(0, 1080, n)], 1).astype(np.float64)
    pb = np.stack([rng.integers(0, 1920, n), rng.integers(-3000, 5000, n)], 1).astype(np.float64)
    Fs = rng.normal(size=(S, 9))
    Fs[:100] = [0.0, 0.0, 2.0, 0.0, 0.0, 1.0, -2.0, -1.0, 37.0] + rng.normal(scale=1e-6, size=(100, 9))   # residuals near the threshold
    pb[:20, 1] = 2 * pa[:20, 0] + pa[:20, 1] - 2 * pb[:20, 0] + 37 + rng.integers(-6, 7, 20)
    Fs[100:110] = np.nan                                    # no model
    Fs[110, 4] = np.nan
    Fs[111:115] = 0.0                                       # d == 0 for every point
    Fs[115] = [0, 0, 0, 0, 0, 0, 0, 0, 1.0]                 # d == 0, e != 0
    Fs[116] = [0, 0, 1.0, 0, 0, 0, -1.0, 0, 0]              # l0 = -1, m0 = 1: d > 0 from constants alone
    Fs[117] = np.inf
    for ip in (1.5, 1e-9, 1e150):
        got = vc.predicate_many(Fs, pa, pb, ip)
        assert got.shape == (S, n) and got.dtype == bool
        for s in range(S):
            assert (got[s] == ref.predicate(Fs[s], pa, pb, ip)).all(), (ip, s)
        assert not got[100:116].any() and (ip != 1.5 or (got[:100].any() and not got[:100].all()))
    assert vc.predicate_many(Fs[:0], pa, pb, 1.5).shape == (0, n)


@pytest.mark.parametrize("n", (8, 9, 40))
def test_first_positions_equal_the_sampler(n):
    S = 4096
    for seed, a, b in ((7, 0, 1), (2**64 - 3, 70001, 70000)):
        ids = vc.first_positions(seed, a, b, S, n)
        assert ids.shape == (S, 8)
        for s in range(S):
            assert ids[s].tolist() == ref.sample(seed, a, b, s, n), (seed, s)
    assert (np.sort(ids, 1)[:, 1:] != np.sort(ids, 1)[:, :-1]).all() and ids.min() == 0 and ids.max() == n - 1


def test_first_positions_falls_back_past_its_vectorised_draws(monkeypatch):
    want = vc.first_positions(7, 0, 1, 512, 8)
    monkeypatch.setattr(vc, "VECTOR_DRAWS", 9)              # at n = 8 most samples need more than 9 draws
    assert (vc.first_positions(7, 0, 1, 512, 8) == want).all()


def test_first_all_good():
    ids = vc.first_positions(4, 0, 1, 30000, 40)
    good = (ids < 14).all(1)
    assert vc.first_all_good(4, 0, 1, 30000, 40, 14) == int(np.flatnonzero(good)[0])
    assert vc.first_all_good(4, 0, 1, 23158, 40, 14) == -1 and vc.first_all_good(4, 0, 1, 5, 40, 40) == 0


# ---- the late winners ---------------------------------------------------------------------------------------------------------------

def test_late_winner_seeds_are_pinned():
    """literal indices: these fail when the sampler changes"""
    assert (vc.LATE_N, vc.LATE_G) == (40, 14)
    assert {seed: vc.first_all_good(seed, 0, 1, vc.MAX_SAMPLES, 40, 14) for seed in (4, 6, 5)} == {4: 23158, 6: 40149, 5: 51091} == vc.LATE_ONE
    assert [vc.pick_place(s, 65536)[1:3] for s in (23158, 40149, 51091)] == [(90, 1), (156, 2), (199, 3)]
    two = [vc.first_all_good(29, a, b, vc.MAX_SAMPLES, 40, 14) for a, b in ((0, 1), (2, 3))]
    assert two == [37447, 17977] == list(vc.LATE_TWO["first"]) and vc.LATE_TWO["seed"] == 29
    three = [vc.first_all_good(29, a, b, vc.MAX_SAMPLES, 40, 14) for a, b in ((0, 1), (2, 3), (4, 5))]
    assert three == [37447, 17977, 45554] == list(vc.LATE_THREE["first"]) and vc.LATE_THREE["seed"] == 29
    assert [vc.pick_place(s, 32768)[0] for s in two] == [1, 0] and [vc.pick_place(s, 21760)[0] for s in three] == [1, 0, 2]


def test_late_winner_data():
    """literal rows: these fail when the builder changes"""
    for slots in (((0, 1),), vc.LATE_THREE["slots"]):
        kp, counts, pl, ml, pts = vc.late_winner_case(slots)
        assert kp.shape == (2 * len(slots), 40, 4) and (counts == 40).all() and pl == list(slots)
        assert (ml[:, :, 0] == np.arange(40)).all() and (ml[:, :, 1] == np.arange(40)).all() and (ml[:, :, 2] == 5).all()
        for (a, b), (pa, pb) in zip(slots, pts):
            assert (kp[a, :, :2] == pa).all() and (kp[b, :, :2] == pb).all()
            r = 2 * pa[:, 0] + pa[:, 1] - 2 * pb[:, 0] - pb[:, 1] + 37
            assert (r[:14] == 0).all() and (np.abs(r[14:]) >= 100).all()
            F = np.array([0.0, 0.0, 2.0, 0.0, 0.0, 1.0, -2.0, -1.0, 37.0])
            assert ref.predicate(F, pa, pb, vc.LATE_IP).tolist() == [True] * 14 + [False] * 26
    kp, counts, pl, ml, pts = vc.late_winner_case()
    assert kp[0, :3, :2].tolist() == [[1839, 98], [971, 322], [1454, 383]], kp[0, :3, :2].tolist()
    assert kp[1, 13:16, :2].tolist() == [[536, 697], [1716, 1194], [1749, 1460]], kp[1, 13:16, :2].tolist()


def test_the_first_all_good_sample_is_the_yardsticks_winner():
    """The slow case of this file (the yardstick's Python loop over 23159 samples: 5 s).  Under call seed 4 every sample ahead of
    the first all-good one is valid and counts fewer inliers than it, strictly: the yardstick's winner is sample 23158, in
    scoring workgroup 90."""
    kp, counts, pl, ml, pts = vc.late_winner_case()
    first = vc.LATE_ONE[4]
    c = vc.yardstick_counts(4, 0, 1, first + 1, *pts[0])
    assert int(np.argmax(c)) == first and c[first] == 14 and c[:first].max() < 14 and (c >= 0).all()
    print("count of the first all-good sample", c[first], "largest before it", c[:first].max(), "below 8:", (c[:first] < 8).mean())
