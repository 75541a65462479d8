"""CPU test (no GPU): the track-consensus kernels (photogrammetry_amd/csrc/k_consensus.hip) are in libpgx.so's code object
once each, with no private segment and no spills -- the two observations a lane holds stay in registers, the hypotheses
are walked without an array indexed at run time -- and the library exports both entry points."""
import photogrammetry_amd._lib as L
from codeobj import kernels

# the scoring kernel is one instance per length class: lanes per track and class in the mangled name
KERNELS = ("k_cns_frames", "k_cns_scoreILi64ELi2E", "k_cns_scoreILi16ELi1E", "k_cns_scoreILi4ELi0E", "k_cns_scan_reduce", "k_cns_scan_sums", "k_cns_scan_apply", "k_cns_write")


def test_consensus_kernels_exist_without_scratch():
    for needle in KERNELS:
        mds = kernels(needle)
        assert len({md["name"] for md in mds}) == 1, (needle, [md["name"] for md in mds])
        for md in mds:
            assert md["private_segment_fixed_size"] == 0, md
            assert md["vgpr_spill_count"] == 0 and md["sgpr_spill_count"] == 0, md


def test_entry_points_are_exported():
    L.build()
    lib = L.lib()
    for name in ("pgx_track_consensus_dev", "pgx_track_consensus"):
        assert name in L.EXPORTS and hasattr(lib, name)
