"""CPU test (no GPU): the verification kernels (photogrammetry_amd/csrc/k_verify.hip) are in libpgx.so's code object once each,
with no private segment and no spills (k_ver_samples keeps G in registers and the eigenvectors in LDS for that), the scoring
kernel's listing walks LDS in float64 with no division and no square root (the hot loop is division-free by contract), the
library exports both entry points, and the workspace a call allocates holds every launch that shares it."""
import ctypes as C

import photogrammetry_amd._lib as L
from codeobj import kernel_body, kernels

KERNELS = ("k_ver_cand", "k_ver_samples", "k_ver_score", "k_ver_pick", "k_ver_refit", "k_ver_write", "k_ver_summary")


def test_verify_kernels_exist_once_without_scratch_or_spills():
    for needle in KERNELS:
        mds = kernels(needle, match="word")
        assert len(mds) == 1, (needle, [md["name"] for md in mds])
        for md in mds:
            assert md["private_segment_fixed_size"] == 0, md
            assert md["vgpr_spill_count"] == 0 and md["sgpr_spill_count"] == 0, md


def test_score_loop_has_no_division_or_square_root():
    mds = kernels("k_ver_score", match="word")
    assert mds
    body = kernel_body(mds[0])
    assert "v_mul_f64" in body and "ds_read" in body
    assert "v_div_scale_f64" not in body and "v_sqrt_f64" not in body and "v_rcp_f64" not in body
    assert "v_fma_f64" not in body          # nothing is contracted


def test_entry_points_are_exported():
    L.build()
    lib = L.lib()
    for name in ("pgx_verify_pairs_dev", "pgx_verify_pair"):
        assert name in L.EXPORTS and hasattr(lib, name)


def test_workspace_holds_every_chunk_of_pairs():
    """pgx_api.hip sizes ws_ver once, for the first chunk of pairs, and runs every chunk of pairs with that chunk's sample
    chunking (pgx_verify_chunk, pgx_verify_ws_bytes: internal C++ functions of the library, called here by their mangled
    names; host code, no GPU).  A shorter last chunk of pairs must not need more."""
    L.build()
    lib = C.CDLL(L.LIB_PATH)
    chunk_of, ws_bytes = lib._Z16pgx_verify_chunkii, lib._Z19pgx_verify_ws_bytesiiii
    chunk_of.restype, chunk_of.argtypes = C.c_int, [C.c_int, C.c_int]
    ws_bytes.restype, ws_bytes.argtypes = C.c_size_t, [C.c_int] * 4
    for per in (16, 129, 255, 2048, 4096):
        for M in (1, 17, 257, 258, 4097, 8200):
            for ns in (1, 256, 512, 2000, 65536):
                for stride in (1, 512):
                    mc = min(M, per)
                    chunk = chunk_of(mc, ns)
                    assert chunk >= 256 and chunk % 256 == 0 and (chunk - 256 < ns or chunk == 256), (per, M, ns, chunk)
                    have = ws_bytes(mc, stride, ns, chunk)
                    assert have >= mc * (chunk * 72 + stride * 36)
                    for n in {mc, M % per or mc, 1}:
                        assert ws_bytes(n, stride, ns, chunk) <= have, (per, M, ns, stride, n)
    # the sample chunk depends on the pairs that share the workspace: 129 pairs get 256 samples a chunk, 128 get 512
    assert chunk_of(129, 512) == 256 and chunk_of(128, 512) == 512
