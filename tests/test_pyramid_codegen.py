"""CPU test (no GPU): the scale pyramid's kernels (photogrammetry_amd/csrc/k_pyramid.hip) on the gfx950 code
object: k_pyr_down and k_pyr_append exist once each, use no scratch and no LDS, and stay at or below 64 vector registers, so
that eight waves fit a SIMD -- both are bound by memory, and the resident waves are what hides its latency.  The resampler
has no fused multiply-add (rule 3 of pgx_set_pyramid counts on nine separate float32 operations) and does write with a
16-byte store."""
import pytest

from codeobj import disassembly, kernels


@pytest.mark.parametrize("name", ["k_pyr_down", "k_pyr_append"])
def test_footprint(name):
    mds = kernels(name)
    assert len(mds) == 1, [md["name"] for md in mds]
    md = mds[0]
    assert md["private_segment_fixed_size"] == 0 and md.get("vgpr_spill_count", 0) == 0 and md.get("sgpr_spill_count", 0) == 0, md
    assert md["group_segment_fixed_size"] == 0, md
    assert md["vgpr_count"] <= 64 and md.get("agpr_count", 0) == 0, md
    assert md["max_flat_workgroup_size"] == 256, md


def _whole_body(md):
    """From the kernel's label to the next symbol's (the resampler has more than one s_endpgm)."""
    text = disassembly(md["object"])
    start = text.index("<%s>:" % md["name"])
    end = text.find(">:\n", start + len(md["name"]) + 3)
    return text[start:end if end > 0 else len(text)]


def test_the_resampler_is_not_contracted_and_stores_16_bytes():
    body = _whole_body(kernels("k_pyr_down")[0])
    assert "s_endpgm" in body
    assert "v_fma" not in body and "v_mac" not in body and "v_mad_f32" not in body and "v_pk_fma" not in body
    assert "global_store_dwordx4" in body                    # the aligned path
    assert "global_store_dword " in body                     # the row tail and unaligned rows
