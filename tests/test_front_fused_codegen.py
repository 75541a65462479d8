"""CPU test (no GPU): the fused dewarp + grey + FAST kernel (photogrammetry_amd/csrc/k_fast.hip, k_dewarp_fast, four
instantiations: map or none, 16-bit or 8-bit source) keeps the footprint DESIGN.md asks of a kernel that runs beside two
distance-kernel waves per SIMD: at most 32 vector registers, no accumulator registers, no scratch, and the LDS of
k_fast_planes (tile 38 x 72 floats, the queue, the planes, the queue count), since both run the same passes.  k_fast_planes
itself, now a caller of the shared passes, stays within 32 registers as well."""
from codeobj import kernel_body, kernels

VGPR_BUDGET = 32
LDS_BYTES = 38 * 72 * 4 + 64 * 32 * 2 + 32 * 3 * 2 * 4 + 4     # 15 812


def test_every_form_of_the_fused_kernel_fits_beside_the_distance_kernel():
    mds = kernels("k_dewarp_fast")
    assert sorted(md["name"].split("k_dewarp_fast")[1][:10] for md in mds) == ["ILb0ELb0EE", "ILb0ELb1EE", "ILb1ELb0EE", "ILb1ELb1EE"]
    for md in mds:
        assert md["vgpr_count"] <= VGPR_BUDGET and md.get("agpr_count", 0) == 0, md
        assert md["private_segment_fixed_size"] == 0 and md.get("vgpr_spill_count", 0) == 0 and md.get("sgpr_spill_count", 0) == 0, md
        assert md["group_segment_fixed_size"] <= LDS_BYTES, md
        assert md["max_flat_workgroup_size"] == 256
        assert "scratch_" not in kernel_body(md)


def test_fast_planes_keeps_its_footprint():
    (md,) = kernels("k_fast_planes")
    assert md["vgpr_count"] <= 32 and md.get("agpr_count", 0) == 0 and md["private_segment_fixed_size"] == 0, md
    assert md["group_segment_fixed_size"] == LDS_BYTES, md


def test_the_map_forms_gather_through_the_plan_in_two_batches():
    """the map forms read eleven plan words per lane (ten rows and the halo position), the others none; every form loads
    eleven pixels; the plan's flag word is a scalar load"""
    for md in kernels("k_dewarp_fast"):
        body = kernel_body(md)
        has_map, src8 = "ILb1ELb" in md["name"], "ELb1EE" in md["name"]
        wide = body.count("global_load_dwordx2")
        narrow = body.count("global_load_dword ")
        if src8:
            assert wide == 0 and narrow == 11 + (11 if has_map else 0), (md["name"], wide, narrow)
        else:
            assert wide == 11 and narrow == (11 if has_map else 0), (md["name"], wide, narrow)
