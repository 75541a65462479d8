"""CPU test (no GPU): the P == 256 BRIEF kernels (photogrammetry_amd/csrc/k_brief.hip, k_brief_kept<true> and
k_brief_list<true>) keep the footprint DESIGN.md section 11 asks of a kernel that runs beside two distance-kernel waves: at
most 32 vector registers, no scratch, and four LDS strips of 512 values + 16 mask words per workgroup.  The generic kernels
(<false>, brief_one) are a separate instantiation, so their larger register count does not decide the P == 256 one's."""
from codeobj import kernel_body, kernels

STRIP_BYTES = 4 * (512 + 16) * 4


def _forms(needle):
    mds = kernels(needle)
    fast = [md for md in mds if "ILb1EE" in md["name"]]
    generic = [md for md in mds if "ILb0EE" in md["name"]]
    assert len(mds) == 2 and len(fast) == 1 and len(generic) == 1, [md["name"] for md in mds]
    return fast[0], generic[0]


def test_p256_kernels_fit_beside_the_distance_kernel():
    for needle in ("k_brief_kept", "k_brief_list"):
        fast, generic = _forms(needle)
        assert fast["vgpr_count"] <= 32 and fast.get("agpr_count", 0) == 0, fast
        assert fast["private_segment_fixed_size"] == 0 and generic["private_segment_fixed_size"] == 0
        assert fast["group_segment_fixed_size"] == STRIP_BYTES, fast
        assert fast["max_flat_workgroup_size"] == 256


def test_p256_kernel_hands_values_over_in_lds_and_has_no_workgroup_barrier():
    fast, _ = _forms("k_brief_kept")
    body = kernel_body(fast)
    assert "ds_write" in body and "ds_read" in body
    assert "s_barrier" not in body           # one wave per keypoint: waves of a workgroup never wait for each other
    assert body.count("global_load_dwordx2") == 8   # the eight coalesced reads of the sorted sample table
