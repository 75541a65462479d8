"""CPU test (no GPU): the FP4 nearest-neighbour kernels inside libpgx.so (k_knn_fp4, photogrammetry_amd/csrc/k_knn.hip) keep the
properties their design rests on, read from the code object the way tests/test_ham_codegen.py reads k_ham_fp4's:
  * they exist and run on the block-scaled FP4 matrix instruction (v_mfma_scale_f32_32x32x64_f8f6f4);
  * NO scratch: zero private segment, no spills -- the top-2 registers (two per accumulator element) are what set the row tiles
    per wave (two; one for the k = 2 form without the column side, which spills at two);
  * the same budget as k_ham_fp4: at most 240 vector registers, no accumulator registers, two workgroups of 256 per CU;
  * the k = 2 loop keeps the second best with one v_med3_i32 per accumulator element.
"""
from codeobj import instructions, kernels, listing

VGPR_BUDGET = 240   # two waves per SIMD with 32 registers to spare, as k_ham_fp4


def test_fp4_knn_kernels_exist_and_fit_the_budget():
    mds = kernels("k_knn_fp4")
    # k in {1, 2} x column output on / off
    assert len({md["name"] for md in mds}) == 4, [md["name"] for md in mds]
    for md in mds:
        assert md["vgpr_count"] <= VGPR_BUDGET, md
        assert md.get("agpr_count", 0) == 0, md
        assert md["vgpr_spill_count"] == 0 and md["sgpr_spill_count"] == 0, md
        assert md["private_segment_fixed_size"] == 0, md
        assert md["max_flat_workgroup_size"] == 256, md
        assert 2 * md["group_segment_fixed_size"] <= 160 * 1024, md


def test_fp4_knn_loop_is_fp4_mfma_with_med3():
    lines, starts = listing("k_knn.hip", "k_knn_fp4")
    assert len(starts) == 4
    for start in starts:
        name = lines[start]
        body = instructions(lines, start)
        assert any(i.startswith("v_mfma_scale_f32_32x32x64_f8f6f4") for i in body), name
        assert not [i for i in body if i.startswith("scratch_")], name
        if "ILi2E" in name:   # k = 2: the second best as one med3 per element of the loop
            assert sum(1 for i in body if i.startswith("v_med3_i32")) >= 64, name
