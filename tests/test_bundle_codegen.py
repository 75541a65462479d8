"""CPU test (no GPU): the bundle-adjustment kernels (photogrammetry_amd/csrc/k_bundle.hip) are in libpgx.so's code object with
no private segment and no spills -- every per-observation quantity is a scalar or an array indexed at compile time, the
reduced system lives in global memory and LDS -- and the library exports both entry points."""
import os
import re
import shutil
import subprocess

import pytest

import photogrammetry_amd._lib as L

LLVM = "/opt/rocm/lib/llvm/bin"
KERNELS = ("k_ba_frames", "k_ba_setup", "k_ba_csr", "k_ba_lin", "k_ba_start", "k_ba_vinv", "k_ba_schur", "k_ba_solve",
           "k_ba_back", "k_ba_decide", "k_ba_final", "k_ba_out")


@pytest.fixture(scope="module")
def code_objects(tmp_path_factory):
    if not os.path.exists(os.path.join(LLVM, "llvm-readelf")):
        pytest.skip("llvm-readelf not found")
    L.build()
    d = str(tmp_path_factory.mktemp("ba_co"))
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
                md = {"name": m.group(1)}
                for key in ("vgpr_spill_count", "sgpr_spill_count", "private_segment_fixed_size", "vgpr_count"):
                    mm = re.search(r"\.%s:\s+(\d+)" % key, item)
                    if mm:
                        md[key] = int(mm.group(1))
                out.append(md)
    return out


def test_bundle_kernels_exist_without_scratch(code_objects):
    for needle in KERNELS:
        mds = _kernels(code_objects, needle)
        assert len({md["name"] for md in mds}) == 1, (needle, [md["name"] for md in mds])
        for md in mds:
            assert md["private_segment_fixed_size"] == 0, md
            assert md["vgpr_spill_count"] == 0 and md["sgpr_spill_count"] == 0, md


def test_entry_points_are_exported():
    L.build()
    lib = L.lib()
    for name in ("pgx_bundle_adjust_dev", "pgx_bundle_adjust"):
        assert name in L.EXPORTS and hasattr(lib, name)
