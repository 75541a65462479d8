"""CPU test (no GPU): the kernels of the dense stage (photogrammetry_amd/csrc/k_depth.hip) are in libpgx.so's code object, with
no private segment and no spills -- the sweep keeps a chunk's eight raw costs and its per-pixel state in registers, with no
array indexed at run time -- and the library exports the five entry points."""
import photogrammetry_amd._lib as L
from codeobj import kernels

# the sweep is one instance per aggregation radius: the radius in the mangled name
KERNELS = ("k_dep_census", "k_dep_plan", "k_dep_sweepILi0E", "k_dep_sweepILi1E", "k_dep_sweepILi2E", "k_dep_sweepILi3E",
           "k_fuse_plan", "k_fuse_count", "k_fuse_scan", "k_fuse_write")


def test_depth_kernels_exist_without_scratch():
    for needle in KERNELS:
        mds = kernels(needle)
        assert len({md["name"] for md in mds}) == 1, (needle, [md["name"] for md in mds])
        for md in mds:
            assert md["private_segment_fixed_size"] == 0, md
            assert md["vgpr_spill_count"] == 0 and md["sgpr_spill_count"] == 0, md
            print(needle, "vgpr", md["vgpr_count"], "lds", md["group_segment_fixed_size"])


def test_entry_points_are_exported():
    L.build()
    lib = L.lib()
    for name in ("pgx_gray_batch_dev", "pgx_depth_maps_dev", "pgx_depth_fuse_dev", "pgx_depth_maps", "pgx_depth_fuse"):
        assert name in L.EXPORTS and hasattr(lib, name)
