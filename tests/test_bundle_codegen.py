"""CPU test (no GPU): the bundle-adjustment kernels (photogrammetry_amd/csrc/k_bundle.hip) are in libpgx.so's code object with
no private segment and no spills -- every per-observation quantity is a scalar or an array indexed at compile time, the
reduced system lives in global memory and LDS -- and the library exports both entry points."""
import photogrammetry_amd._lib as L
from codeobj import kernels

KERNELS = ("k_ba_frames", "k_ba_setup", "k_ba_csr", "k_ba_lin", "k_ba_start", "k_ba_vinv", "k_ba_schur", "k_ba_solve",
           "k_ba_back", "k_ba_decide", "k_ba_final", "k_ba_out")


def test_bundle_kernels_exist_without_scratch():
    for needle in KERNELS:
        mds = kernels(needle, match="word")
        assert len({md["name"] for md in mds}) == 1, (needle, [md["name"] for md in mds])
        for md in mds:
            assert md["private_segment_fixed_size"] == 0, md
            assert md["vgpr_spill_count"] == 0 and md["sgpr_spill_count"] == 0, md


def test_entry_points_are_exported():
    L.build()
    lib = L.lib()
    for name in ("pgx_bundle_adjust_dev", "pgx_bundle_adjust"):
        assert name in L.EXPORTS and hasattr(lib, name)
