"""ctypes loader for libpgx.so -- the only compute backend of this package.

There is deliberately no fallback: if the HIP library is missing or cannot create a
gfx950 context, importing users get a loud error (PgxError / OSError), never a CPU path.
"""
import ctypes as C
import os
import subprocess

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("PGX_LIB", os.path.join(_HERE, "libpgx.so"))  # PGX_LIB: developer A/B builds
CSRC = os.path.join(_HERE, "csrc")

PGX_OK = 0
PGX_E_DIM_MISMATCH, PGX_E_OOB_SOURCE, PGX_E_EMPTY_SET, PGX_E_CAPACITY = 1, 2, 3, 4
PGX_E_BADARG, PGX_E_HIP, PGX_E_NOT_CONFIGURED, PGX_E_RCCL = 5, 6, 7, 8
PGX_DIST_NONE = 2**31 - 1
PGX_SRC_RGBA64, PGX_SRC_RGBA8 = 0, 1
PGX_DEP_NOCAMERA, PGX_DEP_NOVIEWS, PGX_DEP_EDGE, PGX_DEP_HIGHCOST = 1, 2, 4, 8
PGX_DVW_NOCAMERA, PGX_DVW_FEWPOINTS, PGX_DVW_FEWVIEWS, PGX_DVW_NARROW = 1, 2, 4, 8
PGX_STAGE_DETECT, PGX_STAGE_MATCH_WIDE, PGX_STAGE_MATCH_ROWS, PGX_STAGE_MATCH_DONE = 0, 1, 2, 3

# Every export of include/pgx.h with its signature, in the header's order: name -> (restype, [argtypes]).  lib() applies
# the table, so a call site passes plain Python values: ctypes converts each to the declared width (a 64-bit seed or a
# device address stays 64 bits) and refuses the wrong kind with ctypes.ArgumentError before the library is entered.  The
# kinds are coarse on purpose: every pointer, handle and out-parameter is P (numpy and device addresses, byref(...), ctypes
# arrays and None all pass), a `const char *` is S.  Adding an export means three things: the prototype in pgx.h, one line
# here, and a [DllImport] or an OMITTED entry in integration/csharp/PgxNative.cs; the CPU suite fails until all three agree
# (tests/test_abi_symbols.py holds this table to the header, tests/test_csharp_binding.py the C# side).
I, F, D, U64, SZ, P, S = C.c_int, C.c_float, C.c_double, C.c_uint64, C.c_size_t, C.c_void_p, C.c_char_p
SIGNATURES = {
    "pgx_ctx_create": (I, [I, P]),
    "pgx_ctx_destroy": (None, [P]),
    "pgx_last_error": (S, [P]),
    "pgx_version": (S, []),
    "pgx_set_stream": (I, [P, P]),
    "pgx_check_status": (I, [P]),
    "pgx_set_source_format": (I, [P, I]),
    "pgx_set_dewarp_map": (I, [P, P, I, I]),
    "pgx_set_dewarp_coeffs": (I, [P, I, I, P, I]),
    "pgx_get_dewarp_map": (I, [P, P, I, I]),
    "pgx_set_brief_pairs": (I, [P, P, I]),
    "pgx_set_brief_steering": (I, [P, P, P, I, I]),
    "pgx_set_pyramid": (I, [P, I, I]),
    "pgx_pyramid_dims": (I, [I, I, I, I, P, P]),
    "pgx_set_detect_params": (I, [P, F, I]),
    "pgx_set_capacity": (I, [P, I, I]),
    "pgx_set_match_chunk": (I, [P, I]),
    "pgx_dewarp": (I, [P, P, I, I, P]),
    "pgx_gray": (I, [P, P, I, I, P]),
    "pgx_fast": (I, [P, P, I, I, P, I, P]),
    "pgx_brief": (I, [P, P, I, I, P, I, P]),
    "pgx_orient": (I, [P, P, I, I, P, I, P]),
    "pgx_pyramid_level": (I, [P, P, I, I, I, P]),
    "pgx_nms": (I, [P, P, I, I, I, P, P]),
    "pgx_match": (I, [P, P, I, P, I, I, P]),
    "pgx_match_batch": (I, [P, P, P, I, I, P, I, P, P]),
    "pgx_detect": (I, [P, P, I, I, P, P, I, P, P]),
    "pgx_detect_batch_dev": (I, [P, P, I, I, I, P, P, P, P, I]),
    "pgx_detect_batch_steered_dev": (I, [P, P, I, I, I, P, P, P, P, I, P]),
    "pgx_detect_batch_pyramid_dev": (I, [P, P, I, I, I, P, P, P, P, I, P, P, P]),
    "pgx_match_batch_dev": (I, [P, P, P, I, I, P, I, I, P]),
    "pgx_wait_stage": (I, [P, P, I]),
    "pgx_gate_match": (I, [P, P, I]),
    "pgx_knn_batch_dev": (I, [P, P, P, I, I, P, I, I, I, P, P, P]),
    "pgx_match_nn_batch_dev": (I, [P, P, P, I, I, P, I, I, I, F, I, P]),
    "pgx_knn": (I, [P, P, I, P, I, I, I, P, P, P]),
    "pgx_knn_guided_batch_dev": (I, [P, P, P, P, I, I, P, I, I, P, F, I, P, P, P]),
    "pgx_match_guided_batch_dev": (I, [P, P, P, P, I, I, P, I, I, P, F, I, F, I, P]),
    "pgx_knn_guided": (I, [P, P, P, I, P, P, I, I, P, F, I, P, P, P]),
    "pgx_fundamental_ransac_dev": (I, [P, P, P, P, P, I, I, I, I, F, I, U64, P, P, P]),
    "pgx_pose_dev": (I, [P, P, P, P, P, I, I, P, P, P, P, P]),
    "pgx_comm_unique_id": (I, [P]),
    "pgx_comm_init": (I, [P, I, I, P]),
    "pgx_comm_destroy": (I, [P]),
    "pgx_comm_info": (I, [P, P, P]),
    "pgx_allgather_dev": (I, [P, P, SZ]),
    "pgx_sequence_step_dev": (I, [P, P, I, I, I, I, P, P, P, P, I, P, I, I, P]),
    "pgx_tracks_dev": (I, [P, P, P, P, I, I, I, P, I, I, I, P, P, P, P]),
    "pgx_tracks_split_dev": (I, [P, P, P, P, I, I, I, P, I, I, P, I, I, P, P, P, P]),
    "pgx_tracks_create": (I, [P, I, P]),
    "pgx_tracks_destroy": (None, [P]),
    "pgx_tracks_add_pair": (I, [P, I, I, P, I, I]),
    "pgx_tracks_finish": (I, [P, I, P, P]),
    "pgx_tracks_get": (I, [P, P, P]),
    "pgx_tracks_finish_split": (I, [P, P, I, I, P, P, P]),
    "pgx_tracks_dropped": (I, [P, P, P]),
    "pgx_triangulate_tracks_dev": (I, [P, P, I, I, P, I, P, P, P, P, I, D, D, I, P, P, P, P, P]),
    "pgx_triangulate_tracks": (I, [P, P, P, I, P, P, P, I, D, D, I, P, P, P, P, P]),
    "pgx_bundle_adjust_dev": (I, [P, P, I, I, P, I, P, P, P, P, P, P, I, P, P, I, D, D, P, P, P, P, P, P]),
    "pgx_bundle_adjust": (I, [P, P, P, I, P, P, P, P, P, I, P, P, I, D, D, P, P, P, P, P, P]),
    "pgx_register_frames_dev": (I, [P, P, I, I, P, I, P, P, P, P, P, P, I, P, P, I, D, I, I, U64, P, P, P, P, P, P]),
    "pgx_register_frames": (I, [P, P, P, I, P, P, P, P, P, I, P, P, I, D, I, I, U64, P, P, P, P, P, P]),
    "pgx_track_consensus_dev": (I, [P, P, I, I, P, I, P, P, P, P, I, D, D, I, I, I, U64, P, P, P, P, P, P, P, P, P]),
    "pgx_track_consensus": (I, [P, P, P, I, P, P, P, I, D, D, I, I, I, U64, P, P, P, P, P, P, P, P]),
    "pgx_verify_pairs_dev":(I, [P, P, P, P, P, I, I, I, I, D, I, I, U64, P, P, P, P, P, P, P, P]),
    "pgx_verify_pair": (I, [P, P, I, P, I, P, I, I, D, I, I, U64, P, P, P, P]),
    "pgx_init_pair_dev": (I, [P, P, P, P, P, I, I, I, P, I, I, P, P, D, D, I, P, P, P, P, P, P, P, P, P]),
    "pgx_relative_pose": (I, [P, P, I, P, I, P, I, P, P, P, D, D, I, P, P, P, P]),
    "pgx_vocab_quantize_dev": (I, [P, P, P, I, I, P, I, P, P]),
    "pgx_vocab_train_dev": (I, [P, P, P, I, I, I, I, U64, P, P]),
    "pgx_select_pairs_dev": (I, [P, P, P, I, I, P, I, I, I, I, I, I, P, P, P, P]),
    "pgx_vocab_train": (I, [P, P, P, I, I, I, I, U64, P, P]),
    "pgx_select_pairs": (I, [P, P, P, I, I, P, I, I, I, I, I, I, P, P, P, P]),
    "pgx_gray_batch_dev": (I, [P, P, I, I, I, P]),
    "pgx_depth_maps_dev": (I, [P, P, I, I, I, P, I, P, P, I, I, P, I, I, I, I, P, P, P, P, P, P, P]),
    "pgx_depth_fuse_dev": (I, [P, P, P, I, I, I, I, I, P, D, I, I, P, P, P, P]),
    "pgx_depth_maps": (I, [P, P, I, I, I, P, P, I, I, P, I, I, I, I, P, P, P, P, P, P, P]),
    "pgx_depth_fuse": (I, [P, P, P, I, I, I, I, I, P, D, I, I, P, P, P, P]),
    "pgx_dense_views_dev": (I, [P, P, P, P, I, I, P, P, I, P, P, I, I, D, D, I, I, I, I, D, P, P, P, P, P]),
    "pgx_dense_views": (I, [P, P, P, I, P, P, I, P, P, I, I, D, D, I, I, I, I, D, P, P, P, P, P]),
    "pgx_rgba8_batch_dev": (I, [P, P, I, I, I, P]),
    "pgx_cloud_merge_dev": (I, [P, P, P, P, I, P, P, I, I, I, I, I, P, P, I, P, D, D, D, D, I, D, I, I, P, P, P, P, P, P, P]),
    "pgx_rgba8_batch": (I, [P, P, I, I, I, P]),
    "pgx_cloud_merge": (I, [P, P, P, I, P, P, I, I, I, I, I, P, P, D, D, D, D, I, D, I, I, P, P, P, P, P, P, P]),
    "pgx_mesh_dev": (I, [P, P, P, P, I, P, P, I, I, I, I, I, P, P, I, P, I, P, D, D, D, D, I, I, I, I, I, I, P, P, P, P, P, P]),
    "pgx_mesh": (I, [P, P, P, I, P, P, I, I, I, I, I, P, P, I, P, D, D, D, D, I, I, I, I, I, I, P, P, P, P, P, P]),
    "pgx_mesh_clean_dev": (I, [P, P, P, P, P, P, P, I, I, D, D, D, D, I, I, I, D, D, I, I, P, P, P, P, P, P, P, P]),
    "pgx_mesh_clean": (I, [P, P, P, P, P, P, I, I, D, D, D, D, I, I, I, D, D, I, I, P, P, P, P, P, P, P, P]),
    "pgx_mesh_decimate_dev": (I, [P, P, P, P, P, P, P, I, I, D, D, D, D, I, I, I, I, I, P, P, P, P, P, P, P, P]),
    "pgx_mesh_decimate": (I, [P, P, P, P, P, P, I, I, D, D, D, D, I, I, I, I, I, P, P, P, P, P, P, P, P]),
    "pgx_profile_enable": (I, [P, I]),
    "pgx_profile_filter": (I, [P, S]),
    "pgx_profile_get": (I, [P, S, P, P]),
    "pgx_profile_reset": (I, [P]),
    "pgx_profile_serialize": (I, [P, I]),
    "pgx_match_stats": (I, [P, P, P, P]),
    "pgx_debug_counters": (I, [P, P]),
    "pgx_make_brief_pairs": (I, [U64, I, I, P]),
    "pgx_make_steering": (I, [P, I, I, P, P]),
    "pgx_build_dewarp_map": (I, [I, I, P, I, P]),
}
EXPORTS = list(SIGNATURES)


def build(force=False):
    """Compile libpgx.so for gfx950 with hipcc (cross-compiles without a GPU)."""
    cmd = ["make", "-C", CSRC, "-j8"]
    if force:
        subprocess.check_call(["make", "-C", CSRC, "clean"], stdout=subprocess.DEVNULL)
    subprocess.check_call(cmd, stdout=subprocess.DEVNULL)
    if not os.path.exists(LIB_PATH):
        raise OSError("libpgx.so was not produced by " + " ".join(cmd))
    return LIB_PATH


_lib = None


def lib():
    """Load libpgx.so (in-tree).  Raises OSError if it has not been built."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise OSError("%s is missing: run `python -c 'import __graft_entry__ as g; g.build()'` "
                          "(there is no CPU fallback)" % LIB_PATH)
        L = C.CDLL(LIB_PATH)
        for name, (restype, argtypes) in SIGNATURES.items():
            f = getattr(L, name)  # AttributeError if the ABI lost a symbol
            f.restype, f.argtypes = restype, argtypes
        _lib = L
    return _lib
