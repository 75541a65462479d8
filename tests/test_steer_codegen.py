"""CPU test (no GPU): the steered BRIEF kernels (photogrammetry_amd/csrc/k_steer.hip) keep the footprint of the upright ones
they stand in for (tests/test_brief_codegen.py, DESIGN.md sections 11 and 18): two instantiations each of k_steer_kept and
k_steer_list, no scratch anywhere, and the P == 256 forms with at most 32 vector registers, no AGPRs, the four LDS strips
of 512 values + 16 mask words, and no workgroup barrier -- one wave per keypoint, orientation pass included."""
import re

from codeobj import kernel_body, kernels

STRIP_BYTES = 4 * (512 + 16) * 4


def _forms(needle):
    mds = kernels(needle)
    fast = [md for md in mds if "ILb1EE" in md["name"]]
    generic = [md for md in mds if "ILb0EE" in md["name"]]
    assert len(mds) == 2 and len(fast) == 1 and len(generic) == 1, [md["name"] for md in mds]
    return fast[0], generic[0]


def test_new_kernels_exist_and_none_uses_scratch():
    orient = kernels("k_orient_list")
    assert len(orient) == 1, [md["name"] for md in orient]
    for md in orient + list(_forms("k_steer_kept")) + list(_forms("k_steer_list")):
        assert md["private_segment_fixed_size"] == 0 and md.get("vgpr_spill_count", 0) == 0, md
        assert md.get("sgpr_spill_count", 0) == 0 and md["max_flat_workgroup_size"] == 256, md
    assert orient[0]["group_segment_fixed_size"] == 0        # bins only: no descriptor, no strip


def test_steered_names_stay_out_of_the_upright_kernels_selection():
    for md in kernels("k_steer") + kernels("k_orient"):
        assert "k_brief_kept" not in md["name"] and "k_brief_list" not in md["name"], md["name"]


def test_p256_kernels_fit_beside_the_distance_kernel():
    for needle in ("k_steer_kept", "k_steer_list"):
        fast, _ = _forms(needle)
        assert fast["vgpr_count"] <= 32 and fast.get("agpr_count", 0) == 0, fast
        assert fast["group_segment_fixed_size"] == STRIP_BYTES, fast
        body = kernel_body(fast)
        assert "s_barrier" not in body
        assert "ds_write" in body and "ds_read" in body      # brief_256's hand-over through the strip


def test_orientation_rows_are_loaded_ahead():
    """The row loads of the orientation pass go out in groups: fewer waits for vector memory than loads."""
    body = kernel_body(kernels("k_orient_list")[0])
    loads = len(re.findall(r"global_load_dword\s", body))   # the row segments (dwordx2 loads are the keypoint and dirs)
    waits = len(re.findall(r"s_waitcnt[^\n]*vmcnt", body))
    assert loads >= 8 and waits < loads, (loads, waits)
