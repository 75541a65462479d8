"""CPU test of tests/ransac_ref.py, the one sampler of the three RANSAC yardsticks: literal draws of every stage, written down
from the samplers as they stood before they were merged (register_ref.sample, verify_ref.sample, pose_np.sample_indices), and
the key rule.  n == P forces every duplicate rejection; two seeds have bit 63 set."""
import ransac_ref as rr
import register_ref
import verify_ref
import pose_ref
from oracle import pose_np

# (seed, image pair, sample, n, P) -> positions
POSE_DRAWS = (
    ((0x7, 2, 3, 100, 8), [24, 41, 16, 3, 77, 84, 2, 22]),
    ((0x8000000000000001, 0, 0, 8, 8), [2, 3, 7, 5, 1, 0, 4, 6]),
    ((0x21, 1, 999, 30, 8), [14, 15, 5, 25, 0, 9, 7, 3]),
    ((0x5, 65536, 0, 4097, 64), [481, 1436, 1848, 2116, 154, 1034, 1945, 2982, 123, 2668, 2553, 3373, 3128, 2849, 2726, 1893, 442,
                                 2995, 322, 2641, 542, 84, 1038, 1466, 1736, 2722, 2663, 626, 3066, 171, 291, 1235, 2883, 1177, 2852,
                                 2687, 261, 387, 933, 522, 2833, 681, 3706, 447, 2896, 2966, 2808, 2309, 1908, 1877, 1846, 2901, 2311,
                                 1506, 147, 68, 106, 1910, 602, 2305, 3082, 4067, 2304, 2373]),
    ((0xFFFFFFFFFFFFFFFF, 3, 257, 64, 64), [22, 36, 45, 43, 8, 24, 44, 61, 40, 2, 10, 47, 50, 52, 16, 28, 6, 20, 49, 23, 3, 30, 33, 32,
                                            62, 26, 0, 51, 25, 35, 17, 29, 14, 4, 31, 13, 42, 55, 34, 12, 11, 37, 19, 38, 15, 7, 57, 63,
                                            48, 21, 56, 1, 60, 9, 5, 18, 46, 59, 41, 54, 39, 58, 27, 53]),
)
# (seed, frame, sample, n) -> 3 positions
REGISTER_DRAWS = (
    ((0xB, 0, 0, 3), [0, 1, 2]),
    ((0x8000000000003039, 5, 17, 50), [16, 30, 8]),
    ((0x1, 70000, 1000, 1000), [292, 679, 781]),
    ((0x63, 2, 4, 4), [2, 3, 1]),
)
# (seed, frame a, frame b, sample, n) -> 8 positions
VERIFY_DRAWS = (
    ((0x15, 0, 1, 0, 8), [3, 1, 0, 5, 2, 7, 6, 4]),
    ((0x15, 1, 0, 0, 8), [1, 4, 2, 0, 3, 5, 7, 6]),
    ((0xF000000000000003, 3, 7, 300, 40), [18, 19, 15, 9, 12, 14, 13, 27]),
    ((0x5, 10, 11, 65535, 2049), [1696, 1704, 1653, 1496, 539, 1084, 1252, 961]),
)


def test_pose_draws():
    for (seed, m, s, n, P), want in POSE_DRAWS:
        assert rr.draw(rr.stream_seed(seed, m, s), n, P) == want
        assert rr.draw(pose_ref.stream_seed(seed, m, s), n, P) == want
        assert pose_np.sample_indices(seed, m, s, P, n) == want            # the oracle's own copy
    assert any(n == P for (_, _, _, n, P), _ in POSE_DRAWS) and any(t[0] >> 63 for t, _ in POSE_DRAWS)


def test_register_draws():
    for (seed, frame, s, n), want in REGISTER_DRAWS:
        assert register_ref.sample(seed, frame, s, n) == want
        assert rr.draw(rr.stream_seed(seed, frame, s), n, 3) == want
    assert any(t[3] == 3 for t, _ in REGISTER_DRAWS) and any(t[0] >> 63 for t, _ in REGISTER_DRAWS)


def test_verify_draws():
    for (seed, a, b, s, n), want in VERIFY_DRAWS:
        assert verify_ref.sample(seed, a, b, s, n) == want
    assert any(t[4] == 8 for t, _ in VERIFY_DRAWS) and any(t[0] >> 63 for t, _ in VERIFY_DRAWS)
    assert VERIFY_DRAWS[0][1] != VERIFY_DRAWS[1][1]                          # (a, b) is not (b, a)


def test_key_rule():
    assert rr.key(True, 5, 900) > rr.key(True, 4, 0)                         # a higher count beats a lower index
    assert rr.key(True, 5, 3) > rr.key(True, 5, 4)                           # an equal count goes to the lower index
    assert rr.key(True, 0, 0xFFFFFFFE) > rr.key(False, 7, 0) == 0            # zero loses to any valid key
    keys = [rr.key(c > 0, c, s) for s, c in enumerate([0, 3, 7, 7, 2, 7])]
    assert rr.key_index(max(keys)) == 2 and rr.key_count(max(keys)) == 7     # the first best sample
    for count, index in ((0, 0), (1, 256), (4097, 2 ** 31 - 1)):
        k = rr.key(True, count, index)
        assert 0 < k < 1 << 64 and rr.key_index(k) == index and rr.key_count(k) == count
