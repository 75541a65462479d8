"""CPU test (no GPU): the kernels of the mesh (photogrammetry_amd/csrc/k_mesh.hip) are in libpgx.so's code object once each,
with no private segment and no spills; the launch constants that tests/test_gpu_mesh.py sizes its cases by are the source's; the
library exports the two entry points."""
import photogrammetry_amd._lib as L
from codeobj import kernels
from mesh_ref import kernel_constants

KERNELS = ("k_msh_plan", "k_msh_seed", "k_msh_dilate", "k_msh_tsdf", "k_msh_cubes", "k_msh_quads", "k_msh_count", "k_msh_scan",
           "k_msh_rank", "k_msh_vertices", "k_msh_tris")


def test_mesh_kernels_exist_without_scratch():
    c = kernel_constants(L.CSRC)
    for needle in KERNELS:
        mds = kernels(needle)
        assert len(mds) == 1 and len({md["name"] for md in mds}) == 1, (needle, [md["name"] for md in mds])
        for md in mds:
            assert md["private_segment_fixed_size"] == 0, md
            assert md["vgpr_spill_count"] == 0 and md["sgpr_spill_count"] == 0, md
            assert md["max_flat_workgroup_size"] == c["MSH_NT"], md
            print(needle, "vgpr", md["vgpr_count"], "lds", md["group_segment_fixed_size"])


def test_no_other_mesh_kernel():
    assert {md["name"].split("(")[0] for md in kernels("k_msh_")} == {md["name"].split("(")[0] for k in KERNELS for md in kernels(k)}
    assert len(kernels("k_msh_")) == len(KERNELS)


def test_launch_constants():
    c = kernel_constants(L.CSRC)
    assert set(c) >= {"MSH_NT", "MSH_GRID_MAX", "MSH_LG_TMIN", "MSH_MARGIN", "MSH_HASH_MUL"}
    assert c["MSH_NT"] == 256 and c["MSH_HASH_MUL"] % 2 == 1 and c["MSH_MARGIN"] == 4 and c["MSH_LG_TMIN"] == 8


def test_entry_points_are_exported():
    L.build()
    lib = L.lib()
    for name in ("pgx_mesh_dev", "pgx_mesh"):
        assert name in L.EXPORTS and hasattr(lib, name)
