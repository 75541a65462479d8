"""CPU test (no GPU): the pose kernels (photogrammetry_amd/csrc/k_pose.hip) are each in libpgx.so's gfx950 code object exactly
once and without a private segment -- k_pose.hip's comment says the 9 x 9 Jacobi solver was moved out of scratch into
registers, and nothing else holds that.  k_fund_samples does spill VGPRs, but into AGPRs (the count is not pinned; only that
there is no scratch).  The scoring kernel reads its list from the 16 KiB LDS tile, and the library exports both entry points."""
import photogrammetry_amd._lib as L
from codeobj import kernel_body, kernels

KERNELS = ("k_fund_samples", "k_fund_score", "k_fund_pick", "k_pose")


def test_pose_kernels_exist_once_without_scratch():
    for needle in KERNELS:
        mds = kernels(needle, match="mangled")
        assert len(mds) == 1, (needle, [md["name"] for md in mds])
        assert mds[0]["private_segment_fixed_size"] == 0, mds[0]


def test_score_kernel_walks_its_list_in_lds():
    mds = kernels("k_fund_score", match="mangled")
    assert len(mds) == 1
    assert mds[0]["group_segment_fixed_size"] == 1024 * 16, mds[0]      # float4 s_xy[CH]
    body = kernel_body(mds[0])
    assert "ds_read" in body and "ds_write" in body and "s_barrier" in body


def test_entry_points_are_exported():
    L.build()
    lib = L.lib()
    for name in ("pgx_fundamental_ransac_dev", "pgx_pose_dev"):
        assert name in L.EXPORTS and hasattr(lib, name)
