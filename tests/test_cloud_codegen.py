"""CPU test (no GPU): the kernels of the cloud merge (photogrammetry_amd/csrc/k_cloud.hip) and the 8-bit dewarp of k_image.hip
are in libpgx.so's code object once each, with no private segment and no spills; the launch constants that
tests/test_gpu_cloud.py sizes its cases by are the source's; the library exports the four entry points."""
import photogrammetry_amd._lib as L
from cloud_ref import kernel_constants
from codeobj import kernels

# the 8-bit dewarp is one instance per (map, 8-bit source): the two flags in the mangled name
KERNELS = ("k_cld_plan", "k_cld_normals", "k_cld_points", "k_cld_count", "k_cld_scan", "k_cld_rank", "k_cld_accum", "k_cld_final",
           "k_dewarp_rgba8ILb0ELb0E", "k_dewarp_rgba8ILb0ELb1E", "k_dewarp_rgba8ILb1ELb0E", "k_dewarp_rgba8ILb1ELb1E")


def test_cloud_kernels_exist_without_scratch():
    c = kernel_constants(L.CSRC)
    for needle in KERNELS:
        mds = kernels(needle)
        assert len({md["name"] for md in mds}) == 1, (needle, [md["name"] for md in mds])
        for md in mds:
            assert md["private_segment_fixed_size"] == 0, md
            assert md["vgpr_spill_count"] == 0 and md["sgpr_spill_count"] == 0, md
            assert md["max_flat_workgroup_size"] == c["CLD_NT"], md
            print(needle, "vgpr", md["vgpr_count"], "lds", md["group_segment_fixed_size"])


def test_launch_constants():
    c = kernel_constants(L.CSRC)
    assert set(c) >= {"CLD_NT", "CLD_GRID_MAX", "CLD_LG_TMIN", "CLD_ACC", "CLD_HASH_MUL"}
    assert c["CLD_NT"] == 256 and c["CLD_HASH_MUL"] % 2 == 1 and c["CLD_ACC"] == 10


def test_entry_points_are_exported():
    L.build()
    lib = L.lib()
    for name in ("pgx_rgba8_batch_dev", "pgx_cloud_merge_dev", "pgx_rgba8_batch", "pgx_cloud_merge"):
        assert name in L.EXPORTS and hasattr(lib, name)
