"""CPU test (no GPU): the pose kernels (photogrammetry_amd/csrc/k_pose.hip) are each in libpgx.so's gfx950 code object exactly
once and without a private segment -- k_pose.hip's comment says the 9 x 9 Jacobi solver was moved out of scratch into
registers, and nothing else holds that.  k_fund_samples does spill VGPRs, but into AGPRs (the count is not pinned; only that
there is no scratch).  The scoring kernel reads its list from the 16 KiB LDS tile, and the library exports both entry points."""
import os
import re
import shutil
import subprocess

import pytest

import photogrammetry_amd._lib as L

LLVM = "/opt/rocm/lib/llvm/bin"
KERNELS = ("k_fund_samples", "k_fund_score", "k_fund_pick", "k_pose")


@pytest.fixture(scope="module")
def code_objects(tmp_path_factory):
    if not os.path.exists(os.path.join(LLVM, "llvm-readelf")):
        pytest.skip("llvm-readelf not found")
    L.build()
    d = str(tmp_path_factory.mktemp("pose_co"))
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
            # the mangled name holds the length-prefixed identifier followed by E: "6k_poseE" is in no other kernel's name
            if m and "%d%sE" % (len(needle), needle) in m.group(1) and not m.group(1).endswith(".kd"):
                md = {"name": m.group(1), "object": o}
                for key in ("private_segment_fixed_size", "group_segment_fixed_size", "vgpr_count"):
                    mm = re.search(r"\.%s:\s+(\d+)" % key, item)
                    if mm:
                        md[key] = int(mm.group(1))
                out.append(md)
    return out


def test_pose_kernels_exist_once_without_scratch(code_objects):
    for needle in KERNELS:
        mds = _kernels(code_objects, needle)
        assert len(mds) == 1, (needle, [md["name"] for md in mds])
        assert mds[0]["private_segment_fixed_size"] == 0, mds[0]


def test_score_kernel_walks_its_list_in_lds(code_objects):
    mds = _kernels(code_objects, "k_fund_score")
    assert len(mds) == 1
    name, obj = mds[0]["name"], mds[0]["object"]
    assert mds[0]["group_segment_fixed_size"] == 1024 * 16, mds[0]      # float4 s_xy[CH]
    dis = subprocess.run([os.path.join(LLVM, "llvm-objdump"), "-d", obj], check=True, capture_output=True, text=True).stdout
    m = re.search(r"<%s>:\n(.*?)s_endpgm" % re.escape(name), dis, flags=re.S)
    assert m, name
    body = m.group(1)
    assert "ds_read" in body and "ds_write" in body and "s_barrier" in body


def test_entry_points_are_exported():
    L.build()
    lib = L.lib()
    for name in ("pgx_fundamental_ransac_dev", "pgx_pose_dev"):
        assert name in L.EXPORTS and hasattr(lib, name)
