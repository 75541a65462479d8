"""CPU test (no GPU): the epipolar-guided kernels (photogrammetry_amd/csrc/k_guided.hip) and their numpy yardstick.
  * the kernels are in libpgx.so's code object with no private segment and no spills;
  * the compiler's listing of the band walk has no v_fma_f64: the predicate of include/pgx.h is one rounding per operation;
  * the yardstick of tests/guided_ref.py (used by tests/test_gpu_guided.py) equals a literal Python double loop.
"""
import numpy as np

from codeobj import instructions, kernels, listing
from guided_ref import loop_guided, ref_guided
from knn_ref import NONE

KERNELS = ("k_guided_slots", "k_guided_bucket", "k_guided_walk", "k_knn_col_init", "k_knn_col_finish")


def test_guided_kernels_exist_without_scratch():
    for needle in KERNELS:
        mds = kernels(needle)
        # the walk: k in {1, 2} x column side on / off x (256-bit descriptors in registers, any width)
        assert len({md["name"] for md in mds}) == (8 if needle == "k_guided_walk" else 1), (needle, [md["name"] for md in mds])
        for md in mds:
            assert md["private_segment_fixed_size"] == 0, md
            assert md["vgpr_spill_count"] == 0 and md["sgpr_spill_count"] == 0, md


def test_walk_predicate_is_not_contracted():
    lines, starts = listing("k_guided.hip", "k_guided_walk")
    assert len(starts) == 8
    for start in starts:
        body = instructions(lines, start)
        assert any(i.startswith("v_mul_f64") for i in body) and any(i.startswith("v_add_f64") for i in body), lines[start]
        assert not [i for i in body if i.startswith("v_fma_f64")], lines[start]
        assert not [i for i in body if i.startswith("scratch_")], lines[start]


def _case(rng, n1, n2, words, span):
    da = rng.integers(0, 2**32, size=(n1, words), dtype=np.uint32)
    db = rng.integers(0, 2**32, size=(n2, words), dtype=np.uint32)
    kpa = rng.integers(-span, span, size=(n1, 2)).astype(np.int32)
    kpb = rng.integers(-span, span, size=(n2, 2)).astype(np.int32)
    return da, db, kpa, kpb


def _check(da, db, kpa, kpb, F, band):
    rows, cols = loop_guided(da, db, kpa, kpb, F, band)
    idx, dist, col = ref_guided(da, db, kpa, kpb, F, band, block=3)
    for i, row in enumerate(rows):
        exp = row + [(NONE, -1)] * (2 - len(row))
        assert [(int(dist[i, e]), int(idx[i, e])) for e in range(2)] == exp, (i, band)
    assert list(col) == cols, band


def test_yardstick_equals_the_literal_loop():
    rng = np.random.default_rng(0)
    for words, n1, n2, span in [(8, 9, 11, 50), (5, 7, 13, 20), (1, 12, 6, 8), (3, 5, 0, 10), (8, 0, 4, 10), (2, 16, 16, 4)]:
        da, db, kpa, kpb = _case(rng, n1, n2, words, span)
        for F in (rng.normal(size=9), np.array([0, 0, 0, 0, 0, -1, 0, 1, 0]), np.array([1, 0, 0, 0, 1, 0, -3, 2, 1])):
            for band in (0.0, 0.5, 1.0, 2.0, 7.5, 1e30):
                _check(da, db, kpa, kpb, np.asarray(F, dtype=np.float32), band)


def test_yardstick_edges():
    rng = np.random.default_rng(1)
    da, db, kpa, kpb = _case(rng, 6, 9, 8, 10)
    kpb[:, 1] = kpa[rng.integers(0, 6, 9), 1] + rng.integers(-3, 4, 9)      # rows of the axis-aligned lines at 0..3 px
    F_axis = np.array([0, 0, 0, 0, 0, -1, 0, 1, 0], dtype=np.float32)
    for band in (3.0, float(np.nextafter(np.float32(3), np.float32(0))), 0.0):
        _check(da, db, kpa, kpb, F_axis, band)
    for bad in (np.zeros(9), np.r_[np.nan, np.ones(8)], np.r_[np.ones(8), np.inf]):
        _check(da, db, kpa, kpb, np.asarray(bad, dtype=np.float32), 5.0)
        idx, _, col = ref_guided(da, db, kpa, kpb, np.asarray(bad, dtype=np.float32), 5.0)
        assert (idx == -1).all() and (col == -1).all()
    # out-of-range coordinates reject every row
    kpb[0, 0] = 1 << 20
    idx, _, col = ref_guided(da, db, kpa, kpb, F_axis, 5.0)
    assert (idx == -1).all() and (col == -1).all()
