"""CPU test (no GPU): the registration kernels (photogrammetry_amd/csrc/k_register.hip) are in libpgx.so's code object with no
private segment and no spills, the scoring kernel's listing has no float64 division and no square root (the hot loop is
division-free by contract), and the library exports both entry points."""
import os
import re
import shutil
import subprocess

import pytest

import photogrammetry_amd._lib as L

LLVM = "/opt/rocm/lib/llvm/bin"
KERNELS = ("k_reg_frames", "k_reg_count", "k_reg_csr", "k_reg_hyp", "k_reg_score", "k_reg_pick", "k_reg_refine", "k_reg_summary")


@pytest.fixture(scope="module")
def code_objects(tmp_path_factory):
    if not os.path.exists(os.path.join(LLVM, "llvm-readelf")):
        pytest.skip("llvm-readelf not found")
    L.build()
    d = str(tmp_path_factory.mktemp("reg_co"))
    so = os.path.join(d, "libpgx.so")
    shutil.copy(L.LIB_PATH, so)
    subprocess.run([os.path.join(LLVM, "llvm-objdump"), "--offloading", so], cwd=d, check=True, capture_output=True)
    return [os.path.join(d, f) for f in sorted(os.listdir(d)) if "amdgcn" in f]


def _kernels(objs, needle):
    out = []
    for o in objs:
        notes = subprocess.run([os.path.join(LLVM, "llvm-readelf"), "--notes", o], check=True, capture_output=True, text=True).stdout
        for item in re.split(r"\n  - (?=\.)", notes):
            m = re.search(r"\.name:\s+(\S+)", item)
            if m and re.search(needle + r"\D", m.group(1) + " ") and not m.group(1).endswith(".kd"):
                md = {"name": m.group(1), "object": o}
                for key in ("vgpr_spill_count", "sgpr_spill_count", "private_segment_fixed_size", "vgpr_count"):
                    mm = re.search(r"\.%s:\s+(\d+)" % key, item)
                    if mm:
                        md[key] = int(mm.group(1))
                out.append(md)
    return out


def test_register_kernels_exist_without_scratch(code_objects):
    for needle in KERNELS:
        mds = _kernels(code_objects, needle)
        assert len({md["name"] for md in mds}) == 1, (needle, [md["name"] for md in mds])
        for md in mds:
            assert md["private_segment_fixed_size"] == 0, md
            assert md["vgpr_spill_count"] == 0 and md["sgpr_spill_count"] == 0, md


def test_score_loop_has_no_division_or_square_root(code_objects):
    mds = _kernels(code_objects, "k_reg_score")
    assert mds
    name, obj = mds[0]["name"], mds[0]["object"]
    dis = subprocess.run([os.path.join(LLVM, "llvm-objdump"), "-d", obj], check=True, capture_output=True, text=True).stdout
    m = re.search(r"<%s>:\n(.*?)s_endpgm" % re.escape(name), dis, flags=re.S)
    assert m, name
    body = m.group(1)
    assert "v_mul_f64" in body and "ds_read" in body
    assert "v_div_scale_f64" not in body and "v_sqrt_f64" not in body and "v_rcp_f64" not in body


def test_entry_points_are_exported():
    L.build()
    lib = L.lib()
    for name in ("pgx_register_frames_dev", "pgx_register_frames"):
        assert name in L.EXPORTS and hasattr(lib, name)
