"""CPU test (no GPU): the initial-pair kernels (photogrammetry_amd/csrc/k_initpair.hip) are in libpgx.so's code object once
each, with no private segment and no spills (k_init_setup picks the eigenvector columns by selections, so the 3x3 Jacobi solve
stays in registers), the scoring kernel gathers and scores in float64 with no division sequence, no square root and nothing
contracted into a fused multiply-add (the score is division-free by contract), and the library exports both entry points."""
import photogrammetry_amd._lib as L
from codeobj import kernel_body, kernels

KERNELS = ("k_init_setup", "k_init_score", "k_init_finish", "k_init_pick")


def test_init_pair_kernels_exist_once_without_scratch_or_spills():
    for needle in KERNELS:
        mds = kernels(needle, match="word")
        assert len(mds) == 1, (needle, [md["name"] for md in mds])
        for md in mds:
            assert md["private_segment_fixed_size"] == 0, md
            assert md["vgpr_spill_count"] == 0 and md["sgpr_spill_count"] == 0, md


def test_score_kernel_has_no_division_square_root_or_fma():
    mds = kernels("k_init_score", match="word")
    assert mds
    body = kernel_body(mds[0])
    assert "v_mul_f64" in body and "v_cvt_f64_i32" in body        # float64 on integer keypoints
    assert "global_atomic_add" in body                             # the integer counters
    assert "v_div_scale_f64" not in body and "v_rcp_f64" not in body and "v_div_fmas_f64" not in body
    assert "v_sqrt_f64" not in body and "v_rsq_f64" not in body
    assert "v_fma_f64" not in body                                 # nothing is contracted
    assert "scratch_" not in body and "buffer_store" not in body   # no private segment traffic


def test_entry_points_are_exported():
    L.build()
    lib = L.lib()
    for name in ("pgx_init_pair_dev", "pgx_relative_pose"):
        assert name in L.EXPORTS and hasattr(lib, name)
