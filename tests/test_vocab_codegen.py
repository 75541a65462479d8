"""CPU test (no GPU): the vocabulary quantiser inside libpgx.so (k_vocab_fp4, photogrammetry_amd/csrc/k_vocab.hip) keeps the
properties of k_knn_fp4, whose body it shares (csrc/pgx_fp4_nn.h), read from the code object the way tests/test_knn_codegen.py
reads k_knn_fp4's:
  * it runs on the block-scaled FP4 matrix instruction (v_mfma_scale_f32_32x32x64_f8f6f4);
  * the budget of k_knn_fp4 and k_ham_fp4: at most 240 vector registers, no accumulator registers, NO scratch, two workgroups
    of 256 per CU;
  * the LDS it claims: one 32-bit key per row of the workgroup's 256-row block and nothing else;
and the FP4 kernels are the build whose times DESIGN.md records (section 14b for k_knn_fp4 and k_vocab_fp4, section 8 for
k_ham_fp4): the instructions and the resources of every form are exactly those of that build (fingerprints taken from it with
fingerprint() below).  A change to pgx_fp4.h or pgx_fp4_nn.h that moves one of them is measured again before its entry is.
"""
import hashlib
import re

from codeobj import KEYS, disassembly, instructions, kernels, listing

VGPR_BUDGET = 240


def fingerprint(md):
    """sha256 over a kernel's instructions (no addresses, no encodings) and its resource metadata."""
    m = re.search(r"<%s>:\n(.*?s_endpgm)" % re.escape(md["name"]), disassembly(md["object"], "--no-show-raw-insn"), flags=re.S)
    assert m, md["name"]
    text = "\n".join(re.sub(r"//.*$", "", ln).strip() for ln in m.group(1).splitlines())
    text += "\n" + " ".join("%s=%s" % (k, md.get(k)) for k in KEYS)
    return hashlib.sha256(text.encode()).hexdigest()[:16]


# name -> fingerprint in the measured build
MEASURED = {
    "_ZN12_GLOBAL__N_19k_knn_fp4ILi1ELb0ELi2EEEvPKjPKiS4_iiiiPiS5_Pj": "9b5c5cb0a0bf26b0",
    "_ZN12_GLOBAL__N_19k_knn_fp4ILi1ELb1ELi2EEEvPKjPKiS4_iiiiPiS5_Pj": "2665f04249986993",
    "_ZN12_GLOBAL__N_19k_knn_fp4ILi2ELb0ELi1EEEvPKjPKiS4_iiiiPiS5_Pj": "433b447041346f68",
    "_ZN12_GLOBAL__N_19k_knn_fp4ILi2ELb1ELi2EEEvPKjPKiS4_iiiiPiS5_Pj": "d29ab2d94ca88acc",
    "_ZN12_GLOBAL__N_111k_vocab_fp4EPKjPKiiiiS1_iPiS4_": "87e1565ef89f746d",
    "_ZN12_GLOBAL__N_19k_ham_fp4ILi3EEEvPjPKjPKiiiiiiiPy": "0b35e58c1b94ac03",
}


def test_quantiser_is_fp4_mfma_within_the_budget():
    mds = kernels("k_vocab_fp4")
    assert len(mds) == 1, [md["name"] for md in mds]
    md = mds[0]
    assert md["vgpr_count"] <= VGPR_BUDGET, md
    assert md.get("agpr_count", 0) == 0, md
    assert md["vgpr_spill_count"] == 0 and md["sgpr_spill_count"] == 0, md
    assert md["private_segment_fixed_size"] == 0, md
    assert md["max_flat_workgroup_size"] == 256, md
    assert md["group_segment_fixed_size"] == 256 * 4, md   # rowtop: one key per row
    lines, starts = listing("k_vocab.hip", "k_vocab_fp4")
    assert len(starts) == 1
    body = instructions(lines, starts[0])
    # five per column tile (four of the product, one that steps the key) for each of two row tiles, several steps unrolled
    assert sum(1 for i in body if i.startswith("v_mfma_scale_f32_32x32x64_f8f6f4")) >= 9
    assert not [i for i in body if i.startswith("scratch_")]


def test_the_fp4_kernels_are_the_measured_build():
    mds = kernels("k_knn_fp4") + kernels("k_vocab_fp4") + kernels("k_ham_fp4")
    got = {md["name"]: fingerprint(md) for md in mds}
    assert len(MEASURED) >= 6 and got == MEASURED
