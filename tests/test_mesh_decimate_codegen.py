"""CPU test (no GPU): the kernels of the mesh's decimation (photogrammetry_amd/csrc/k_meshdecimate.hip) are in libpgx.so's code
object once each, with no private segment and no spills; the launch constants that tests/test_gpu_mesh_decimate.py sizes its
cases by are the source's; the library exports the two entry points."""
import photogrammetry_amd._lib as L
from codeobj import kernels
from mesh_decimate_ref import kernel_constants

KERNELS = ("k_mdc_plan", "k_mdc_init", "k_mdc_tris", "k_mdc_vlevel", "k_mdc_up", "k_mdc_clusters", "k_mdc_vslot", "k_mdc_map", "k_mdc_claim",
           "k_mdc_mark", "k_mdc_bsum", "k_mdc_scan", "k_mdc_rank", "k_mdc_emit", "k_mdc_tnormal", "k_mdc_finish")


def test_mesh_decimate_kernels_exist_without_scratch():
    c = kernel_constants(L.CSRC)
    for needle in KERNELS:
        mds = kernels(needle)
        assert len(mds) == 1 and len({md["name"] for md in mds}) == 1, (needle, [md["name"] for md in mds])
        for md in mds:
            assert md["private_segment_fixed_size"] == 0, md
            assert md["vgpr_spill_count"] == 0 and md["sgpr_spill_count"] == 0, md
            assert md["max_flat_workgroup_size"] == c["MDC_NT"], md
            print(needle, "vgpr", md["vgpr_count"], "lds", md["group_segment_fixed_size"])


def test_no_other_mesh_decimate_kernel():
    assert {md["name"].split("(")[0] for md in kernels("k_mdc_")} == {md["name"].split("(")[0] for k in KERNELS for md in kernels(k)}
    assert len(kernels("k_mdc_")) == len(KERNELS)


def test_launch_constants():
    c = kernel_constants(L.CSRC)
    assert c["MDC_NT"] == 256 and c["MDC_SLOTS"] == 1 << c["MDC_LG_SLOTS"] and 0 < c["MDC_FLUSH_AT"] <= c["MDC_SLOTS"] - c["MDC_NT"]
    assert c["MDC_GRID_MAX"] >= 1 and c["MDC_LG_TMIN"] >= 1
    assert c["MDC_HASH_MUL"] % 2 == 1 and c["MDC_TRI_MUL1"] % 2 == 1 and c["MDC_TRI_MUL2"] % 2 == 1


def test_entry_points_are_exported():
    L.build()
    lib = L.lib()
    for name in ("pgx_mesh_decimate_dev", "pgx_mesh_decimate"):
        assert name in L.EXPORTS and hasattr(lib, name)
