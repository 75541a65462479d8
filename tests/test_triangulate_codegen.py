"""CPU test (no GPU): the triangulation kernels (photogrammetry_amd/csrc/k_triangulate.hip) are in libpgx.so's code object
with no private segment and no spills -- the 4x4 Jacobi and the 3x3 solve are indexed at compile time, nothing per
observation is held in an array -- and the library exports both entry points."""
import photogrammetry_amd._lib as L
from codeobj import kernels

KERNELS = ("k_tri_frames", "k_tri_tracks", "k_tri_summary")


def test_triangulation_kernels_exist_without_scratch():
    for needle in KERNELS:
        mds = kernels(needle)
        assert len({md["name"] for md in mds}) == 1, (needle, [md["name"] for md in mds])
        for md in mds:
            assert md["private_segment_fixed_size"] == 0, md
            assert md["vgpr_spill_count"] == 0 and md["sgpr_spill_count"] == 0, md


def test_entry_points_are_exported():
    L.build()
    lib = L.lib()
    for name in ("pgx_triangulate_tracks_dev", "pgx_triangulate_tracks"):
        assert name in L.EXPORTS and hasattr(lib, name)
