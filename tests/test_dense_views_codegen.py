"""CPU test (no GPU): the kernels of the dense stage's plan (photogrammetry_amd/csrc/k_denseviews.hip) are in libpgx.so's code
object once each, with no private segment and no spills; the pair kernel's two forms hold the LDS their constants say; the
launch constants that tests/test_gpu_dense_views.py sizes its cases by are the source's; the library exports both entry
points."""
import photogrammetry_amd._lib as L
from codeobj import kernels
from dense_views_ref import kernel_constants

# the pair kernel is one instance per accumulation form: LDS (b1) and global (b0)
KERNELS = ("k_dvw_frames", "k_dvw_count", "k_dvw_scanE", "k_dvw_scatter", "k_dvw_pairsILb1E", "k_dvw_pairsILb0E", "k_dvw_select")


def test_dense_views_kernels_exist_without_scratch():
    for needle in KERNELS:
        mds = kernels(needle)
        assert len({md["name"] for md in mds}) == 1, (needle, [md["name"] for md in mds])
        for md in mds:
            assert md["private_segment_fixed_size"] == 0, md
            assert md["vgpr_spill_count"] == 0 and md["sgpr_spill_count"] == 0, md
            assert md["max_flat_workgroup_size"] == kernel_constants()["DVW_NT"], md


def test_launch_constants_and_lds():
    c = kernel_constants()
    assert set(c) >= {"DVW_NT", "DVW_GRID_MAX", "DVW_PAIR_GRID_MAX", "DVW_LDS_FRAMES", "DVW_LDS_CELLS"}
    assert c["DVW_NT"] == 256 and c["DVW_LDS_CELLS"] >= 64 * 64      # the bench graph's 64 references of 64 frames stay in LDS
    lds = {needle: kernels(needle)[0]["group_segment_fixed_size"] for needle in KERNELS}
    assert 8 * c["DVW_LDS_CELLS"] <= lds["k_dvw_pairsILb1E"] < 8 * c["DVW_LDS_CELLS"] + 64
    assert lds["k_dvw_pairsILb0E"] < 64
    for needle in ("k_dvw_count", "k_dvw_scatter"):
        assert 4 * c["DVW_LDS_FRAMES"] <= lds[needle] < 4 * c["DVW_LDS_FRAMES"] + 64
    assert max(lds.values()) <= 65536


def test_entry_points_are_exported():
    L.build()
    lib = L.lib()
    for name in ("pgx_dense_views_dev", "pgx_dense_views"):
        assert name in L.EXPORTS and hasattr(lib, name)
