"""CPU test (no GPU): the kernels of the mesh's clean stage (photogrammetry_amd/csrc/k_meshclean.hip) are in libpgx.so's code
object once each, with no private segment and no spills; the launch constants that tests/test_gpu_mesh_clean.py sizes its cases
by are the source's; the library exports the two entry points."""
import photogrammetry_amd._lib as L
from codeobj import kernels
from mesh_clean_ref import kernel_constants

KERNELS = ("k_mcl_init", "k_mcl_union", "k_mcl_roots", "k_mcl_count", "k_mcl_bsum", "k_mcl_scan", "k_mcl_rank", "k_mcl_emit",
           "k_mcl_rows", "k_mcl_smooth", "k_mcl_tnormal", "k_mcl_finish")


def test_mesh_clean_kernels_exist_without_scratch():
    c = kernel_constants(L.CSRC)
    for needle in KERNELS:
        mds = kernels(needle)
        assert len(mds) == 1 and len({md["name"] for md in mds}) == 1, (needle, [md["name"] for md in mds])
        for md in mds:
            assert md["private_segment_fixed_size"] == 0, md
            assert md["vgpr_spill_count"] == 0 and md["sgpr_spill_count"] == 0, md
            assert md["max_flat_workgroup_size"] == c["MCL_NT"], md
            print(needle, "vgpr", md["vgpr_count"], "lds", md["group_segment_fixed_size"])


def test_no_other_mesh_clean_kernel():
    assert {md["name"].split("(")[0] for md in kernels("k_mcl_")} == {md["name"].split("(")[0] for k in KERNELS for md in kernels(k)}
    assert len(kernels("k_mcl_")) == len(KERNELS)


def test_launch_constants():
    c = kernel_constants(L.CSRC)
    assert set(c) == {"MCL_NT", "MCL_GRID_MAX", "MCL_UNION_GRID", "MCL_SLOTS", "MCL_LONG_ROW"}
    assert c["MCL_LONG_ROW"] >= 1 and c["MCL_NT"] == 256 and c["MCL_SLOTS"] >= 2 * c["MCL_NT"] and c["MCL_SLOTS"] & (c["MCL_SLOTS"] - 1) == 0
    assert 1 <= c["MCL_UNION_GRID"] <= c["MCL_GRID_MAX"]


def test_entry_points_are_exported():
    L.build()
    lib = L.lib()
    for name in ("pgx_mesh_clean_dev", "pgx_mesh_clean"):
        assert name in L.EXPORTS and hasattr(lib, name)
