"""CPU test (no GPU): the registration kernels (photogrammetry_amd/csrc/k_register.hip) are in libpgx.so's code object with no
private segment and no spills, the scoring kernel's listing has no float64 division and no square root (the hot loop is
division-free by contract), and the library exports both entry points."""
import photogrammetry_amd._lib as L
from codeobj import kernel_body, kernels

KERNELS = ("k_reg_frames", "k_reg_count", "k_reg_csr", "k_reg_hyp", "k_reg_score", "k_reg_pick", "k_reg_refine", "k_reg_summary")


def test_register_kernels_exist_without_scratch():
    for needle in KERNELS:
        mds = kernels(needle, match="word")
        assert len({md["name"] for md in mds}) == 1, (needle, [md["name"] for md in mds])
        for md in mds:
            assert md["private_segment_fixed_size"] == 0, md
            assert md["vgpr_spill_count"] == 0 and md["sgpr_spill_count"] == 0, md


def test_score_loop_has_no_division_or_square_root():
    mds = kernels("k_reg_score", match="word")
    assert mds
    body = kernel_body(mds[0])
    assert "v_mul_f64" in body and "ds_read" in body
    assert "v_div_scale_f64" not in body and "v_sqrt_f64" not in body and "v_rcp_f64" not in body


def test_entry_points_are_exported():
    L.build()
    lib = L.lib()
    for name in ("pgx_register_frames_dev", "pgx_register_frames"):
        assert name in L.EXPORTS and hasattr(lib, name)
