"""CPU test (no GPU): the FP4 nearest-neighbour kernels inside libpgx.so (k_knn_fp4, photogrammetry_amd/csrc/k_knn.hip) keep the
properties their design rests on, read from the code object the way tests/test_ham_codegen.py reads k_ham_fp4's:
  * they exist and run on the block-scaled FP4 matrix instruction (v_mfma_scale_f32_32x32x64_f8f6f4);
  * NO scratch: zero private segment, no spills -- the top-2 registers (two per accumulator element) are what set the row tiles
    per wave (two; one for the k = 2 form without the column side, which spills at two);
  * the same budget as k_ham_fp4: at most 240 vector registers, no accumulator registers, two workgroups of 256 per CU;
  * the k = 2 loop keeps the second best with one v_med3_i32 per accumulator element.
"""
import os
import re
import shutil
import subprocess

import pytest

import photogrammetry_amd._lib as L

LLVM = "/opt/rocm/lib/llvm/bin"
VGPR_BUDGET = 240   # two waves per SIMD with 32 registers to spare, as k_ham_fp4


@pytest.fixture(scope="module")
def code_objects(tmp_path_factory):
    if not os.path.exists(os.path.join(LLVM, "llvm-readelf")):
        pytest.skip("llvm-readelf not found")
    L.build()
    d = str(tmp_path_factory.mktemp("knn_co"))
    so = os.path.join(d, "libpgx.so")
    shutil.copy(L.LIB_PATH, so)
    subprocess.run([os.path.join(LLVM, "llvm-objdump"), "--offloading", so], cwd=d, check=True, capture_output=True)
    return [os.path.join(d, f) for f in sorted(os.listdir(d)) if "amdgcn" in f]


def _kernels(objs, needle):
    """[{field: value}] of every kernel whose name contains `needle` (AMDGPU metadata notes)."""
    out = []
    for o in objs:
        notes = subprocess.run([os.path.join(LLVM, "llvm-readelf"), "--notes", o], check=True, capture_output=True, text=True).stdout
        for item in re.split(r"\n  - (?=\.)", notes):
            m = re.search(r"\.name:\s+(\S+)", item)
            if m and needle in m.group(1) and not m.group(1).endswith(".kd"):
                md = {"name": m.group(1), "object": o}
                for key in ("vgpr_count", "vgpr_spill_count", "sgpr_spill_count", "private_segment_fixed_size", "agpr_count",
                            "group_segment_fixed_size", "max_flat_workgroup_size"):
                    mm = re.search(r"\.%s:\s+(\d+)" % key, item)
                    if mm:
                        md[key] = int(mm.group(1))
                out.append(md)
    return out


def test_fp4_knn_kernels_exist_and_fit_the_budget(code_objects):
    mds = _kernels(code_objects, "k_knn_fp4")
    # k in {1, 2} x column output on / off
    assert len({md["name"] for md in mds}) == 4, [md["name"] for md in mds]
    for md in mds:
        assert md["vgpr_count"] <= VGPR_BUDGET, md
        assert md.get("agpr_count", 0) == 0, md
        assert md["vgpr_spill_count"] == 0 and md["sgpr_spill_count"] == 0, md
        assert md["private_segment_fixed_size"] == 0, md
        assert md["max_flat_workgroup_size"] == 256, md
        assert 2 * md["group_segment_fixed_size"] <= 160 * 1024, md


def test_fp4_knn_loop_is_fp4_mfma_with_med3(tmp_path):
    hipcc = "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not found")
    root = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
    out = os.path.join(str(tmp_path), "k_knn.s")
    subprocess.run([hipcc, "-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-ffp-contract=off", "-fno-fast-math",
                    "--cuda-device-only", "-S", os.path.join(root, "photogrammetry_amd", "csrc", "k_knn.hip"), "-o", out],
                   check=True, capture_output=True)
    lines = open(out).read().split("\n")
    starts = [i for i, l in enumerate(lines) if re.match(r"^_ZN.*k_knn_fp4.*:", l)]
    assert len(starts) == 4
    for start in starts:
        name = lines[start]
        end = next(i for i in range(start, len(lines)) if lines[i].startswith(".Lfunc_end"))
        body = [l.strip().split(";")[0].strip() for l in lines[start:end]
                if l.startswith("\t") and not l.startswith("\t.") and not l.strip().startswith(";")]
        assert any(i.startswith("v_mfma_scale_f32_32x32x64_f8f6f4") for i in body), name
        assert not [i for i in body if i.startswith("scratch_")], name
        if "ILi2E" in name:   # k = 2: the second best as one med3 per element of the loop
            assert sum(1 for i in body if i.startswith("v_med3_i32")) >= 64, name
