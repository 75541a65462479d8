"""Host-side mirror of the reference's ImageProcessing classes over the C ABI (include/pgx.h).

The reference's seam is "concrete class method called from a Dataflow block" (SURVEY D1):
DeWarp.ApplyDistortionMat, Grayscale.FromRgba64 (via Matrix.Convert), KeypointDetection.Detect,
RedundantKeypointEliminator.EliminateRedundantKeypoints, KeypointMatching.MatchKeypoints.
The classes below keep those names, argument meanings and error behaviour (the .NET exception
types are mirrored by the exception classes here) so that tests read like the reference's own.
All arithmetic happens in libpgx.so on the GPU; numpy arrays are only the marshalling format.
The C++ twin of this file (for a compiled host) is photogrammetry_amd/host/pgx_host.hpp.
"""
import ctypes as C

import numpy as np

from . import _lib
from ._lib import (PGX_DIST_NONE, PGX_SRC_RGBA64, PGX_SRC_RGBA8, PGX_E_BADARG, PGX_E_CAPACITY, PGX_E_DIM_MISMATCH, PGX_E_EMPTY_SET,
                   PGX_E_HIP, PGX_E_NOT_CONFIGURED, PGX_E_OOB_SOURCE, PGX_OK)

KEYPOINT_DTYPE = np.dtype([("x", "<i4"), ("y", "<i4"), ("fast_score", "<i4"), ("value", "<f4")])
PAIR_DTYPE = np.dtype([("k1", "<i4"), ("k2", "<i4"), ("dist", "<i4")])


class PgxError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__("pgx error %d: %s" % (code, msg))
        self.code = code


class ArgumentException(PgxError, ValueError):
    """System.ArgumentException (DeWarp.cs:23, :48)."""


class IndexOutOfRangeException(PgxError, IndexError):
    """System.IndexOutOfRangeException (Matrix.cs:65, :207)."""


class ArgumentOutOfRangeException(PgxError, IndexError):
    """System.ArgumentOutOfRangeException (KeypointMatching.cs:61 with an empty keypoints2)."""


class CapacityError(PgxError):
    pass


_EXC = {PGX_E_DIM_MISMATCH: ArgumentException, PGX_E_BADARG: ArgumentException,
        PGX_E_OOB_SOURCE: IndexOutOfRangeException, PGX_E_EMPTY_SET: ArgumentOutOfRangeException,
        PGX_E_CAPACITY: CapacityError}


class RcclError(PgxError):
    pass


_EXC[_lib.PGX_E_RCCL] = RcclError


def _ptr(a):
    """A pointer argument: the address of a numpy array, the device pointer of a torch tensor, a raw int as it is; None is
    NULL.  _lib.SIGNATURES declares every such parameter as c_void_p, so the plain int keeps its 64 bits."""
    if a is None or isinstance(a, int):
        return a
    return a.ctypes.data if isinstance(a, np.ndarray) else a.data_ptr()


_dptr = _ptr   # the name the device-resident call sites use


def _host_tracks(kps_per_frame, track_offsets, nodes):
    """The host forms' inputs: tracks as (track_offsets, nodes) or, with nodes=None, as a list of tracks; keypoints per frame.
    -> (off [n_tracks + 1], nd [n_nodes][2], kp per frame, counts [n_frames], flat keypoints)"""
    if nodes is None:
        tracks = track_offsets
        track_offsets = np.cumsum([0] + [len(t) for t in tracks])
        nodes = [fk for t in tracks for fk in t]
    off = np.ascontiguousarray(track_offsets, dtype=np.int32).reshape(-1)
    nd = np.ascontiguousarray(nodes, dtype=np.int32).reshape(-1, 2)
    kp = [np.ascontiguousarray(k, dtype=KEYPOINT_DTYPE) for k in kps_per_frame]
    counts = np.array([len(k) for k in kp], dtype=np.int32)
    flat = np.ascontiguousarray(np.concatenate(kp) if len(kp) else np.zeros(0, KEYPOINT_DTYPE))
    return off, nd, kp, counts, flat


def _host_problem(kps_per_frame, K, Rt, sel, track_offsets, nodes, xyz, track_flags):
    """What the host forms of bundle adjustment and registration share: their arguments kps .. track_flags in the C order (arrays
    for pointers, None for NULL; sel = the per-frame int32 array, `fixed` or `reg`) -> (those arguments, n_frames, n_tracks,
    n_nodes)."""
    off, nd, kp, counts, flat = _host_tracks(kps_per_frame, track_offsets, nodes)
    nf, n = len(kp), len(off) - 1
    Kc = np.ascontiguousarray(K, dtype=np.float64).reshape(nf, 4)
    Rc = np.ascontiguousarray(Rt, dtype=np.float64).reshape(nf, 12)
    sl = np.ascontiguousarray(sel, dtype=np.int32).reshape(nf)
    X = np.ascontiguousarray(xyz, dtype=np.float64).reshape(n, 3)
    fl = None if track_flags is None else np.ascontiguousarray(track_flags, dtype=np.int32).reshape(n)
    head = (flat if len(flat) else None, counts, nf, Kc, Rc, sl, off, nd if len(nd) else None, n, X if n else None, fl if n else None)
    return head, nf, n, len(nd)


def _desc_pair(desc1, desc2):
    """The two descriptor sets of a one-pair host call -> (d1, d2, words): words from the first set that has rows, 8 when
    neither has."""
    d1 = np.ascontiguousarray(desc1, dtype=np.uint32)
    d2 = np.ascontiguousarray(desc2, dtype=np.uint32)
    words = d1.shape[1] if d1.ndim == 2 and d1.shape[0] else (d2.shape[1] if d2.ndim == 2 and d2.shape[0] else 8)
    return d1, d2, words


def _dense_inputs(xyz, src, depth, views, cameras, rgba8):
    """what cloud_merge and mesh take alike, converted: the list (xyz [n][3], src [n][2]), depth [R][H][W], views [R][1 + S], cameras
    [n_frames][12] and rgba8 [n_frames][H][W] or None"""
    X = np.ascontiguousarray(xyz, dtype=np.float64).reshape(-1, 3)
    sr = np.ascontiguousarray(src, dtype=np.int32).reshape(-1, 2)
    d = np.ascontiguousarray(depth, dtype=np.float64)
    R, H, W = d.shape
    vw = np.ascontiguousarray(views, dtype=np.int32)
    vw = vw.reshape(R, vw.shape[-1])
    P = np.ascontiguousarray(cameras, dtype=np.float64).reshape(-1, 12)
    col = None if rgba8 is None else np.ascontiguousarray(rgba8, dtype=np.uint32).reshape(len(P), H, W)
    return X, sr, d, vw, P, col


def _mesh_inputs(xyz, normal, rgba8, info, tri):
    """the five arrays of a mesh in pgx_mesh's layout, converted"""
    X = np.ascontiguousarray(xyz, dtype=np.float64).reshape(-1, 3)
    n = len(X)
    return (X, np.ascontiguousarray(normal, dtype=np.float32).reshape(n, 3), np.ascontiguousarray(rgba8, dtype=np.uint32).reshape(n),
            np.ascontiguousarray(info, dtype=np.int32).reshape(n, 4), np.ascontiguousarray(tri, dtype=np.int32).reshape(-1, 3))


def _mesh_outputs(nv, nt):
    """... for a stage to write at most nv vertices and nt triangles into, and its report"""
    mv, mt = max(nv, 1), max(nt, 1)
    return (np.zeros((mv, 3)), np.zeros((mv, 3), dtype=np.float32), np.zeros(mv, dtype=np.uint32), np.zeros((mv, 4), dtype=np.int32),
            np.zeros((mt, 3), dtype=np.int32), np.zeros(8, dtype=np.int32))


def _mesh_result(out, nv, nt, **per_vertex):
    """... trimmed to the counts of the report, with the stage's per-vertex maps"""
    oxyz, onrm, orgb, oinf, otri, report = out
    kv, kt = min(int(report[5]), nv), min(int(report[6]), nt)
    return dict(xyz=oxyz[:kv], normal=onrm[:kv], rgba8=orgb[:kv], info=oinf[:kv], tri=otri[:kt], **per_vertex, report=report)


class Engine:
    """One pgx context = one GPU (pgx_ctx_create).  Thin, 1:1 with the C ABI."""

    def __init__(self, device=0):
        self._L = _lib.lib()
        h = C.c_void_p()
        rc = self._L.pgx_ctx_create(int(device), C.byref(h))
        if rc != PGX_OK:
            raise PgxError(rc, "pgx_ctx_create(device=%d) failed: no usable gfx950 device "
                               "(this package has no CPU fallback)" % device)
        self._h = h
        self.device = device
        self.words = 0
        self.P = 0

    def close(self):
        if getattr(self, "_h", None):
            self._L.pgx_ctx_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _chk(self, rc):
        if rc != PGX_OK:
            msg = self._L.pgx_last_error(self._h).decode()
            raise _EXC.get(rc, PgxError)(rc, msg)

    # -- configuration ------------------------------------------------------------------
    def set_stream(self, stream_handle):
        self._chk(self._L.pgx_set_stream(self._h, stream_handle))

    def check_status(self):
        self._chk(self._L.pgx_check_status(self._h))

    def set_dewarp_map(self, map_uv):
        if map_uv is None:
            self._chk(self._L.pgx_set_dewarp_map(self._h, None, 0, 0))
            return
        m = np.ascontiguousarray(map_uv, dtype=np.int32)
        assert m.ndim == 3 and m.shape[2] == 2
        self._chk(self._L.pgx_set_dewarp_map(self._h, _ptr(m), m.shape[1], m.shape[0]))

    def set_dewarp_coeffs(self, W, H, coeffs):
        """Build the table on the device from the five distortion coefficients (DeWarp.GetDistortionMatrix)."""
        k = np.ascontiguousarray(coeffs, dtype=np.float64).reshape(-1)
        self._chk(self._L.pgx_set_dewarp_coeffs(self._h, int(W), int(H), _ptr(k), int(k.size)))

    def get_dewarp_map(self, W, H):
        out = np.zeros((H, W, 2), dtype=np.int32)
        self._chk(self._L.pgx_get_dewarp_map(self._h, _ptr(out), int(W), int(H)))
        return out

    def set_brief_pairs(self, pairs):
        p = np.ascontiguousarray(pairs, dtype=np.int32).reshape(-1, 4)
        self._chk(self._L.pgx_set_brief_pairs(self._h, _ptr(p), p.shape[0]))
        self.P = p.shape[0]
        self.words = (self.P + 31) // 32

    def set_brief_steering(self, pairs_rot, dirs=None, radius=15):
        """Steered BRIEF (pgx.h): pairs_rot [B][P][4] and dirs [B][2] from make_steering, disc radius of the orientation
        pass.  pairs_rot=None turns the mode off."""
        if pairs_rot is None:
            self._chk(self._L.pgx_set_brief_steering(self._h, None, None, 0, 0))
            return
        t = np.ascontiguousarray(pairs_rot, dtype=np.int32)
        d = np.ascontiguousarray(dirs, dtype=np.int32).reshape(-1, 2)
        B = d.shape[0]
        if 4 <= B <= 64 and B % 4 == 0 and t.size != B * self.P * 4:   # the library reads B x P x 4 values; it rejects any other B itself
            raise ValueError("pairs_rot has %d values; %d directions of the current table need %d" % (t.size, B, B * self.P * 4))
        self._chk(self._L.pgx_set_brief_steering(self._h, _ptr(t), _ptr(d), int(B), int(radius)))

    def set_pyramid(self, n_levels, step_q16=92682):
        """Scale pyramid (pgx.h): n_levels in [1, 8] (1 = off), step_q16 = the scale step between levels in 16.16 fixed
        point, 69632 ... 131072 (92682 ~ sqrt 2).  With it on the detect entry points write merged multi-level lists."""
        self._chk(self._L.pgx_set_pyramid(self._h, int(n_levels), int(step_q16)))
        self._pyramid = (int(n_levels), int(step_q16))

    def set_detect_params(self, threshold, suppression_radius):
        self._chk(self._L.pgx_set_detect_params(self._h, threshold, int(suppression_radius)))

    def set_capacity(self, max_raw_per_frame, max_keypoints_per_frame):
        self._chk(self._L.pgx_set_capacity(self._h, int(max_raw_per_frame), int(max_keypoints_per_frame)))

    def set_source_format(self, fmt):
        """PGX_SRC_RGBA64 (0, default) or PGX_SRC_RGBA8 (1): 8-bit frames, widened x257 on the device (pgx.h)."""
        self._chk(self._L.pgx_set_source_format(self._h, int(fmt)))
        self._src_dtype = np.uint8 if int(fmt) == PGX_SRC_RGBA8 else np.uint16

    def set_match_chunk(self, image_pairs_per_chunk):
        self._chk(self._L.pgx_set_match_chunk(self._h, int(image_pairs_per_chunk)))

    def wait_stage(self, other, stage):
        """This context's stream waits for a stage (PGX_STAGE_*) of `other`'s most recent call of that kind (pgx.h)."""
        self._chk(self._L.pgx_wait_stage(self._h, other._h, int(stage)))

    def gate_match(self, other, stage):
        """The next matcher call of this context waits for a stage of `other` between its init kernel and its first distance
        round (pgx_gate_match; one shot)."""
        self._chk(self._L.pgx_gate_match(self._h, other._h, int(stage)))

    # -- stage-granular host API ----------------------------------------------------------
    def dewarp(self, rgba64):
        a = np.ascontiguousarray(rgba64, dtype=getattr(self, "_src_dtype", np.uint16))
        out = np.empty(a.shape, dtype=np.uint16)
        self._chk(self._L.pgx_dewarp(self._h, _ptr(a), a.shape[1], a.shape[0], _ptr(out)))
        return out

    def gray(self, rgba64):
        a = np.ascontiguousarray(rgba64, dtype=getattr(self, "_src_dtype", np.uint16))
        out = np.empty(a.shape[:2], dtype=np.float32)
        self._chk(self._L.pgx_gray(self._h, _ptr(a), a.shape[1], a.shape[0], _ptr(out)))
        return out

    def fast(self, gray, capacity=None):
        g = np.ascontiguousarray(gray, dtype=np.float32)
        cap = int(capacity) if capacity is not None else max(1, g.size)
        out = np.zeros(cap, dtype=KEYPOINT_DTYPE)
        n = C.c_int(0)
        self._chk(self._L.pgx_fast(self._h, _ptr(g), g.shape[1], g.shape[0], _ptr(out), cap, C.byref(n)))
        return out[:n.value].copy()

    def brief(self, gray, kps):
        g = np.ascontiguousarray(gray, dtype=np.float32)
        k = np.ascontiguousarray(kps, dtype=KEYPOINT_DTYPE)
        out = np.zeros((len(k), self.words), dtype=np.uint32)
        self._chk(self._L.pgx_brief(self._h, _ptr(g), g.shape[1], g.shape[0], _ptr(k), len(k), _ptr(out)))
        return out

    def orient(self, gray, kps):
        """The direction bin of every keypoint (steered mode on), int32 [n]."""
        g = np.ascontiguousarray(gray, dtype=np.float32)
        k = np.ascontiguousarray(kps, dtype=KEYPOINT_DTYPE)
        out = np.zeros(len(k), dtype=np.int32)
        self._chk(self._L.pgx_orient(self._h, _ptr(g), g.shape[1], g.shape[0], _ptr(k), len(k), _ptr(out)))
        return out

    def pyramid_level(self, gray, level):
        """Level `level` of a float32 grey image under the context's pyramid step, float32 [H_l][W_l]."""
        g = np.ascontiguousarray(gray, dtype=np.float32)
        n_levels, step = getattr(self, "_pyramid", (1, 0))
        dims = pyramid_dims(g.shape[1], g.shape[0], n_levels, step)[0] if n_levels > 1 else np.zeros((1, 2), np.int32)
        w, h = (int(v) for v in dims[level]) if 0 <= level < len(dims) else (0, 0)
        out = np.empty((max(h, 1), max(w, 1)), dtype=np.float32)
        self._chk(self._L.pgx_pyramid_level(self._h, _ptr(g), g.shape[1], g.shape[0], int(level), _ptr(out)))
        return out

    def nms(self, kps, W, H):
        k = np.ascontiguousarray(kps, dtype=KEYPOINT_DTYPE)
        order = np.zeros(max(1, len(k)), dtype=np.int32)
        n = C.c_int(0)
        self._chk(self._L.pgx_nms(self._h, _ptr(k), len(k), int(W), int(H), _ptr(order), C.byref(n)))
        return order[:n.value].copy()

    def match(self, desc1, desc2):
        d1, d2, words = _desc_pair(desc1, desc2)
        out = np.zeros(max(1, len(d1)), dtype=PAIR_DTYPE)
        self._chk(self._L.pgx_match(self._h, _ptr(d1), len(d1), _ptr(d2), len(d2), words, _ptr(out)))
        return out[:len(d1)].copy()

    def match_batch(self, descs, pair_list):
        """pgx_match_batch: descs = list of [n_f][words] arrays (one per frame), pair_list = [(a, b), ...] -> list of
        PAIR_DTYPE arrays, one per image pair, in the reference's emission order.  Raises ArgumentOutOfRangeException
        (after all lists are computed) when some pair has an empty second set."""
        F = len(descs)
        arrs = [np.ascontiguousarray(d, dtype=np.uint32) for d in descs]
        words = next((a.shape[1] for a in arrs if a.ndim == 2 and a.shape[0]), 8)
        for f, a in enumerate(arrs):   # the library copies counts[f] * words words from every descs[f]
            if len(a) and (a.ndim != 2 or a.shape[1] != words):
                raise ValueError("descs[%d] has shape %s; every non-empty set must be [n][%d]" % (f, a.shape, words))
        counts = np.array([len(a) for a in arrs], dtype=np.int32)
        ptrs = (C.c_void_p * max(1, F))(*[a.ctypes.data if len(a) else None for a in arrs])
        pl = np.ascontiguousarray(pair_list, dtype=np.int32).reshape(-1, 2)
        M = len(pl)
        total = int(sum(int(counts[a]) for a, _ in pl))
        out = np.zeros(max(1, total), dtype=PAIR_DTYPE)
        offs = np.zeros(M + 1, dtype=np.int64)
        rc = self._L.pgx_match_batch(self._h, ptrs, _ptr(counts), F, int(words), _ptr(pl), M, _ptr(out), _ptr(offs))
        lists = [out[offs[m]:offs[m + 1]].copy() for m in range(M)]
        if rc == _lib.PGX_E_EMPTY_SET:
            self.last_batch_lists = lists   # all lists are valid; the reference would have thrown at the empty pair
        self._chk(rc)
        return lists

    def detect(self, rgba64, capacity=8192):
        a = np.ascontiguousarray(rgba64, dtype=getattr(self, "_src_dtype", np.uint16))
        kp = np.zeros(capacity, dtype=KEYPOINT_DTYPE)
        desc = np.zeros((capacity, max(1, self.words)), dtype=np.uint32)
        n, nraw = C.c_int(0), C.c_int(0)
        self._chk(self._L.pgx_detect(self._h, _ptr(a), a.shape[1], a.shape[0], _ptr(kp), _ptr(desc), int(capacity),
                                     C.byref(n), C.byref(nraw)))
        return kp[:n.value].copy(), desc[:n.value].copy(), nraw.value

    def detect_pyramid(self, rgba64, capacity=8192, bins=False):
        """The chain in pyramid mode for one host image -> (keypoints, descriptors, origin [n][3] = (level, x_l, y_l),
        level stats [n_levels][2] = (entries, raw hits), nraw[, bins with bins=True; steering on]).  The frame and the
        outputs go through torch device tensors (pgx_detect_batch_pyramid_dev has no host form); the call waits."""
        import torch
        a = np.ascontiguousarray(rgba64, dtype=getattr(self, "_src_dtype", np.uint16))
        H, W = a.shape[:2]
        n_levels = getattr(self, "_pyramid", (1, 0))[0]
        dev = torch.device("cuda", self.device)
        words = max(1, self.words)
        d_frame = torch.from_numpy(a.view(np.int16 if a.dtype == np.uint16 else np.uint8)).to(dev)
        i32 = dict(dtype=torch.int32, device=dev)
        d_kp, d_desc = torch.zeros((capacity, 4), **i32), torch.zeros((capacity, words), **i32)
        d_cnt, d_origin = torch.zeros(2, **i32), torch.zeros((capacity, 3), **i32)
        d_stats = torch.zeros((max(1, n_levels), 2), **i32)
        d_bins = torch.zeros(capacity, **i32) if bins else None
        torch.cuda.synchronize(dev)   # torch's fills run on its own stream; the context's stream does not order against it
        self._chk(self._L.pgx_detect_batch_pyramid_dev(self._h, _dptr(d_frame), 1, W, H, _dptr(d_kp), _dptr(d_desc), _dptr(d_cnt),
                                                       d_cnt.data_ptr() + 4, int(capacity), _dptr(d_origin), _dptr(d_stats),
                                                       _dptr(d_bins)))
        err = None
        try:
            self.check_status()
        except CapacityError as e:   # the first `capacity` entries are intact: hand them over with the error
            err = e
        n, nraw = (int(v) for v in d_cnt.cpu().numpy())
        kp = np.ascontiguousarray(d_kp[:n].cpu().numpy()).view(KEYPOINT_DTYPE).reshape(-1)
        out = (kp, d_desc[:n].cpu().numpy().view(np.uint32), d_origin[:n].cpu().numpy(), d_stats.cpu().numpy(), nraw)
        if bins:
            out += (d_bins[:n].cpu().numpy(),)
        if err is not None:
            err.partial = out
            raise err
        return out

    # -- device-resident batched API (torch tensors or raw device pointers) -------------------
    def detect_batch_dev(self, d_rgba64, F, W, H, d_kp, d_desc, d_counts, d_nraw, capacity):
        self._chk(self._L.pgx_detect_batch_dev(self._h, _dptr(d_rgba64), int(F), int(W), int(H), _dptr(d_kp),
                                               _dptr(d_desc), _dptr(d_counts), _dptr(d_nraw), int(capacity)))

    def detect_batch_steered_dev(self, d_rgba64, F, W, H, d_kp, d_desc, d_counts, d_nraw, capacity, d_bins):
        self._chk(self._L.pgx_detect_batch_steered_dev(self._h, _dptr(d_rgba64), int(F), int(W), int(H), _dptr(d_kp),
                                                       _dptr(d_desc), _dptr(d_counts), _dptr(d_nraw), int(capacity), _dptr(d_bins)))

    def detect_batch_pyramid_dev(self, d_rgba64, F, W, H, d_kp, d_desc, d_counts, d_nraw, capacity, d_origin, d_level_stats,
                                 d_bins=None):
        """pgx_detect_batch_pyramid_dev: the merged lists plus d_origin [F][capacity][3] and d_level_stats [F][n_levels][2];
        d_bins [F][capacity] only with steering on."""
        self._chk(self._L.pgx_detect_batch_pyramid_dev(self._h, _dptr(d_rgba64), int(F), int(W), int(H), _dptr(d_kp), _dptr(d_desc),
                                                       _dptr(d_counts), _dptr(d_nraw), int(capacity), _dptr(d_origin),
                                                       _dptr(d_level_stats), _dptr(d_bins)))

    def match_batch_dev(self, d_desc, d_counts, stride, words, d_pairlist, M, d_out, max_count=None):
        self._chk(self._L.pgx_match_batch_dev(self._h, _dptr(d_desc), _dptr(d_counts), int(stride), int(words),
                                              _dptr(d_pairlist), int(M), int(stride if max_count is None else max_count), _dptr(d_out)))

    # -- exact nearest-neighbour matching (include/pgx.h, "exact nearest-neighbour matching") --------------
    def knn(self, desc1, desc2, k=2, col=False):
        """pgx_knn: the k (1 or 2) nearest columns of every row of desc1 in desc2, ascending in (distance, column).
        Returns (idx [n1][k], dist [n1][k]) int32 arrays, and col_nn [n2] (the nearest row of every column, -1 when desc1 is
        empty) as a third array when col=True.  Missing neighbours are (-1, PGX_DIST_NONE)."""
        d1, d2, words = _desc_pair(desc1, desc2)
        return self._knn_out(len(d1), len(d2), k, col, lambda *out: self._L.pgx_knn(
            self._h, _ptr(d1), len(d1), _ptr(d2), len(d2), words, int(k), *out))

    def _knn_out(self, n1, n2, k, col, call):
        """The output side of knn / knn_guided: buffers of at least one row (no NULL for an empty set), call(idx, dist, col_nn)
        on their addresses, the results cut to n1 rows and n2 columns."""
        kk = max(1, int(k))
        idx = np.zeros((max(1, n1), kk), dtype=np.int32)
        dist = np.zeros((max(1, n1), kk), dtype=np.int32)
        cnn = np.zeros(max(1, n2), dtype=np.int32) if col else None
        self._chk(call(_ptr(idx), _ptr(dist), _ptr(cnn)))
        if col:
            return idx[:n1].copy(), dist[:n1].copy(), cnn[:n2].copy()
        return idx[:n1].copy(), dist[:n1].copy()

    def knn_batch_dev(self, d_desc, d_counts, stride, words, d_pairlist, M, k, d_idx, d_dist, d_col_nn=None, max_count=None):
        """pgx_knn_batch_dev: d_idx, d_dist [M][stride][k] int32, d_col_nn [M][stride] int32 or None (device tensors)."""
        self._chk(self._L.pgx_knn_batch_dev(self._h, _dptr(d_desc), _dptr(d_counts), int(stride), int(words), _dptr(d_pairlist),
                                            int(M), int(stride if max_count is None else max_count), int(k), _dptr(d_idx),
                                            _dptr(d_dist), _dptr(d_col_nn)))

    def match_nn_batch_dev(self, d_desc, d_counts, stride, words, d_pairlist, M, d_out, max_dist, ratio=0.0, cross_check=False,
                           max_count=None):
        """pgx_match_nn_batch_dev: d_out [M][stride] PAIR_DTYPE (int32 [..][3]) -- per row (i, j1, d1) when accepted, else
        (i, -1, PGX_DIST_NONE); feeds tracks_dev as it is."""
        self._chk(self._L.pgx_match_nn_batch_dev(self._h, _dptr(d_desc), _dptr(d_counts), int(stride), int(words), _dptr(d_pairlist),
                                                 int(M), int(stride if max_count is None else max_count), int(max_dist),
                                                 ratio, 1 if cross_check else 0, _dptr(d_out)))

    # -- epipolar-guided exact matching (include/pgx.h, "epipolar-guided exact matching") ----------------
    def knn_guided(self, desc1, kp1, desc2, kp2, F, band, k=2, col=False):
        """pgx_knn_guided: knn() restricted to the columns within `band` pixels of each row's epipolar line.  kp1, kp2:
        KEYPOINT_DTYPE arrays (or int32 [n][4]) of the same lengths as desc1, desc2; F: 9 float32 values, row-major,
        h1^T F h2 = 0.  Returns (idx [n1][k], dist [n1][k]) and col_nn [n2] as a third array when col=True."""
        d1, d2, words = _desc_pair(desc1, desc2)
        k1 = np.ascontiguousarray(np.asarray(kp1).view(np.int32).reshape(-1, 4) if len(kp1) else np.zeros((0, 4), np.int32))
        k2 = np.ascontiguousarray(np.asarray(kp2).view(np.int32).reshape(-1, 4) if len(kp2) else np.zeros((0, 4), np.int32))
        f = np.ascontiguousarray(np.asarray(F, dtype=np.float32).reshape(9))
        n1, n2 = len(d1), len(d2)
        if len(k1) != n1 or len(k2) != n2:
            raise ValueError("keypoint and descriptor counts differ")
        return self._knn_out(n1, n2, k, col, lambda *out: self._L.pgx_knn_guided(
            self._h, _ptr(d1), _ptr(k1), n1, _ptr(d2), _ptr(k2), n2, words, _ptr(f), band, int(k), *out))

    def knn_guided_batch_dev(self, d_desc, d_kp, d_counts, stride, words, d_pairlist, M, d_F, band, k, d_idx, d_dist,
                             d_col_nn=None, max_count=None):
        """pgx_knn_guided_batch_dev: d_kp [F][stride] keypoints, d_F [M][9] float32; d_idx, d_dist [M][stride][k] int32,
        d_col_nn [M][stride] int32 or None (device tensors)."""
        self._chk(self._L.pgx_knn_guided_batch_dev(self._h, _dptr(d_desc), _dptr(d_kp), _dptr(d_counts), int(stride), int(words),
                                                   _dptr(d_pairlist), int(M), int(stride if max_count is None else max_count),
                                                   _dptr(d_F), band, int(k), _dptr(d_idx), _dptr(d_dist), _dptr(d_col_nn)))

    def match_guided_batch_dev(self, d_desc, d_kp, d_counts, stride, words, d_pairlist, M, d_F, band, d_out, max_dist, ratio=0.0,
                               cross_check=False, max_count=None):
        """pgx_match_guided_batch_dev: the guided NN lists, d_out [M][stride] PAIR_DTYPE as match_nn_batch_dev's."""
        self._chk(self._L.pgx_match_guided_batch_dev(self._h, _dptr(d_desc), _dptr(d_kp), _dptr(d_counts), int(stride), int(words),
                                                     _dptr(d_pairlist), int(M), int(stride if max_count is None else max_count),
                                                     _dptr(d_F), band, int(max_dist), ratio, 1 if cross_check else 0, _dptr(d_out)))

    # -- RANSAC fundamental matrix / pose (device tensors) ------------------------------------------
    def fundamental_ransac_dev(self, d_kp, d_matches, d_counts, d_pairlist, M, stride, n_samples, pairs_per_sample, threshold,
                               d_F, d_inliers, d_best_sample, rank_check=False, seed=0):
        self._chk(self._L.pgx_fundamental_ransac_dev(self._h, _dptr(d_kp), _dptr(d_matches), _dptr(d_counts), _dptr(d_pairlist),
                                                     int(M), int(stride), int(n_samples), int(pairs_per_sample), threshold,
                                                     1 if rank_check else 0, seed, _dptr(d_F), _dptr(d_inliers), _dptr(d_best_sample)))

    def pose_dev(self, d_kp, d_matches, d_counts, d_pairlist, M, stride, d_F, d_Rt, d_votes, d_best, d_points=None):
        self._chk(self._L.pgx_pose_dev(self._h, _dptr(d_kp), _dptr(d_matches), _dptr(d_counts), _dptr(d_pairlist), int(M),
                                       int(stride), _dptr(d_F), _dptr(d_Rt), _dptr(d_votes), _dptr(d_best), _dptr(d_points)))

    # -- the track graph on the device (pgx_tracks_dev) ----------------------------------------------
    def tracks_dev(self, d_matches, d_counts, d_pairlist, M, F, stride, n_frames, max_dist, min_len, d_track_of, d_offsets,
                   d_nodes, d_summary, d_frame_ids=None):
        """Connected components over the gated match lists where they sit in HBM (pgx.h: order-independent semantics).
        d_track_of [n_frames][stride], d_offsets [n_frames * stride + 1], d_nodes [n_frames * stride][2], d_summary [8]."""
        self._chk(self._L.pgx_tracks_dev(self._h, _dptr(d_matches), _dptr(d_counts), _dptr(d_pairlist), int(M), int(F), int(stride),
                                         _dptr(d_frame_ids), int(n_frames), int(max_dist), int(min_len), _dptr(d_track_of),
                                         _dptr(d_offsets), _dptr(d_nodes), _dptr(d_summary)))

    def tracks_split_dev(self, d_matches, d_counts, d_pairlist, M, F, stride, n_frames, max_dist, gates, min_len, d_track_of,
                         d_offsets, d_nodes, d_summary, d_frame_ids=None):
        """The split mode (pgx_tracks_split_dev): a component inconsistent at max_dist is split at the first of the tighter
        `gates` (strictly decreasing, below max_dist, >= 0, at most 7) where its parts are consistent, instead of dropped.
        Layouts as tracks_dev, but d_summary [16]: [8 + l] = nodes in tracks resolved at level l (level 0 = max_dist)."""
        g = np.ascontiguousarray(list(gates), dtype=np.int32)
        self._chk(self._L.pgx_tracks_split_dev(self._h, _dptr(d_matches), _dptr(d_counts), _dptr(d_pairlist), int(M), int(F),
                                               int(stride), _dptr(d_frame_ids), int(n_frames), int(max_dist),
                                               _ptr(g) if len(g) else None, len(g), int(min_len),
                                               _dptr(d_track_of), _dptr(d_offsets), _dptr(d_nodes), _dptr(d_summary)))

    # -- multi-view triangulation of tracks (pgx_triangulate_tracks*) -----------------------------------
    def triangulate_tracks_dev(self, d_kp, F, stride, n_frames, d_P, d_offsets, d_nodes, d_track_summary, max_tracks, d_xyz,
                               d_quality, d_flags, d_summary, min_parallax_deg=1.0, max_reproj_px=float("inf"), refine_iters=10,
                               d_node_err=None, d_frame_ids=None):
        """One point per track of the graph's output, where it sits in HBM (pgx.h: multi-view triangulation).  d_P [n_frames][12]
        float64 by frame number; d_xyz / d_quality [max_tracks][3] float64, d_flags [max_tracks] int32, d_summary [8] int32,
        d_node_err [n_frames * stride] float64 or None.  n_tracks is read on the device: no sync."""
        self._chk(self._L.pgx_triangulate_tracks_dev(
            self._h, _dptr(d_kp), int(F), int(stride), _dptr(d_frame_ids), int(n_frames), _dptr(d_P), _dptr(d_offsets),
            _dptr(d_nodes), _dptr(d_track_summary), int(max_tracks), min_parallax_deg, max_reproj_px, int(refine_iters),
            _dptr(d_xyz), _dptr(d_quality), _dptr(d_flags), _dptr(d_node_err), _dptr(d_summary)))

    def triangulate_tracks(self, kps_per_frame, cameras, track_offsets, nodes=None, min_parallax_deg=1.0,
                           max_reproj_px=float("inf"), refine_iters=10):
        """The host form (pgx_triangulate_tracks).  kps_per_frame: one KEYPOINT_DTYPE array per frame; cameras [n_frames][3][4]
        (or [n_frames][12]) float64, NaN rows for frames without a pose.  Tracks as pgx_tracks_get gives them (track_offsets
        [n_tracks + 1], nodes [n_nodes][2]) or, with nodes=None, the `tracks` list of tracks_host.
        -> dict(xyz [n][3], quality [n][3] = (rms, max, parallax), flags [n], node_err [n_nodes], summary [8])."""
        off, nd, kp, counts, flat = _host_tracks(kps_per_frame, track_offsets, nodes)
        P = np.ascontiguousarray(cameras, dtype=np.float64).reshape(len(kp), 12)
        n = len(off) - 1
        xyz, q = np.zeros((max(n, 1), 3)), np.zeros((max(n, 1), 3))
        flags, err = np.zeros(max(n, 1), dtype=np.int32), np.zeros(max(len(nd), 1))
        summary = np.zeros(8, dtype=np.int32)
        self._chk(self._L.pgx_triangulate_tracks(
            self._h, _ptr(flat) if len(flat) else None, _ptr(counts), len(kp), _ptr(P), _ptr(off), _ptr(nd) if len(nd) else None, n,
            min_parallax_deg, max_reproj_px, int(refine_iters), _ptr(xyz), _ptr(q), _ptr(flags), _ptr(err), _ptr(summary)))
        return dict(xyz=xyz[:n], quality=q[:n], flags=flags[:n], node_err=err[:len(nd)], summary=summary)

    # -- bundle adjustment of cameras and track points (pgx_bundle_adjust*) ------------------------------
    def bundle_adjust_dev(self, d_kp, F, stride, n_frames, d_K, d_Rt_in, d_fixed, d_offsets, d_nodes, d_track_summary, max_tracks,
                          d_xyz_in, d_Rt_out, d_P_out, d_xyz_out, d_trace, d_report, max_iters=20, huber_px=float("inf"),
                          lambda0=1e-3, d_track_flags=None, d_node_err=None, d_frame_ids=None):
        """Levenberg-Marquardt on the free cameras and the points of the graph's tracks, where they sit in HBM (pgx.h: bundle
        adjustment).  d_K [n_frames][4], d_Rt_in / d_Rt_out / d_P_out [n_frames][12] float64, d_fixed [n_frames] int32,
        d_xyz_in / d_xyz_out [max_tracks][3] float64, d_track_flags [max_tracks] int32 or None, d_trace [max_iters + 1][2]
        float64, d_report [8] int32, d_node_err [n_frames * stride] float64 or None.  n_tracks is read on the device: no sync."""
        self._chk(self._L.pgx_bundle_adjust_dev(
            self._h, _dptr(d_kp), int(F), int(stride), _dptr(d_frame_ids), int(n_frames), _dptr(d_K), _dptr(d_Rt_in), _dptr(d_fixed),
            _dptr(d_offsets), _dptr(d_nodes), _dptr(d_track_summary), int(max_tracks), _dptr(d_xyz_in), _dptr(d_track_flags),
            int(max_iters), huber_px, lambda0, _dptr(d_Rt_out), _dptr(d_P_out), _dptr(d_xyz_out), _dptr(d_node_err), _dptr(d_trace),
            _dptr(d_report)))

    def bundle_adjust(self, kps_per_frame, K, Rt, fixed, track_offsets, nodes, xyz, track_flags=None, max_iters=20,
                      huber_px=float("inf"), lambda0=1e-3):
        """The host form (pgx_bundle_adjust).  kps_per_frame: one KEYPOINT_DTYPE array per frame; K [n_frames][4], Rt
        [n_frames][12] float64; fixed [n_frames]; tracks as pgx_tracks_get gives them (track_offsets [n_tracks + 1], nodes
        [n_nodes][2]) or, with nodes=None, the `tracks` list of tracks_host; xyz [n_tracks][3]; track_flags [n_tracks] or None.
        -> dict(Rt [F][12], P [F][12], xyz [n][3], node_err [n_nodes], trace [max_iters + 1][2], report [8])"""
        head, nf, n, n_nodes = _host_problem(kps_per_frame, K, Rt, fixed, track_offsets, nodes, xyz, track_flags)
        Rt_out, P_out = np.zeros((nf, 12)), np.zeros((nf, 12))
        xyz_out, err = np.zeros((max(n, 1), 3)), np.zeros(max(n_nodes, 1))
        trace, report = np.zeros((int(max_iters) + 1, 2)), np.zeros(8, dtype=np.int32)
        self._chk(self._L.pgx_bundle_adjust(
            self._h, *map(_ptr, head), int(max_iters), huber_px, lambda0, _ptr(Rt_out), _ptr(P_out), _ptr(xyz_out), _ptr(err),
            _ptr(trace), _ptr(report)))
        return dict(Rt=Rt_out, P=P_out, xyz=xyz_out[:n], node_err=err[:n_nodes], trace=trace, report=report)

    # -- frame registration by P3P RANSAC against track points (pgx_register_frames*) ------------------
    def register_frames_dev(self, d_kp, F, stride, n_frames, d_K, d_Rt_in, d_register, d_offsets, d_nodes, d_track_summary,
                            max_tracks, d_xyz, d_Rt_out, d_P_out, d_frame_stats, d_frame_err, d_report, n_samples=1024,
                            inlier_px=2.0, min_inliers=12, refine_iters=10, seed=0, d_track_flags=None, d_node_inlier=None,
                            d_frame_ids=None):
        """Pose of every frame with d_register != 0 from its 2D-3D correspondences, where they sit in HBM (pgx.h: frame
        registration).  d_K [n_frames][4], d_Rt_in / d_Rt_out / d_P_out [n_frames][12] float64, d_register [n_frames] int32,
        d_xyz [max_tracks][3] float64, d_track_flags [max_tracks] int32 or None, d_frame_stats [n_frames][4] int32,
        d_frame_err [n_frames][2] float64, d_node_inlier [n_frames * stride] int32 or None, d_report [8] int32.  n_tracks is
        read on the device: no sync."""
        self._chk(self._L.pgx_register_frames_dev(
            self._h, _dptr(d_kp), int(F), int(stride), _dptr(d_frame_ids), int(n_frames), _dptr(d_K), _dptr(d_Rt_in),
            _dptr(d_register), _dptr(d_offsets), _dptr(d_nodes), _dptr(d_track_summary), int(max_tracks), _dptr(d_xyz),
            _dptr(d_track_flags), int(n_samples), inlier_px, int(min_inliers), int(refine_iters), seed,
            _dptr(d_Rt_out), _dptr(d_P_out), _dptr(d_frame_stats), _dptr(d_frame_err), _dptr(d_node_inlier), _dptr(d_report)))

    def register_frames(self, kps_per_frame, K, Rt, reg, track_offsets, nodes, xyz, track_flags=None, n_samples=1024,
                        inlier_px=2.0, min_inliers=12, refine_iters=10, seed=0):
        """The host form (pgx_register_frames).  kps_per_frame: one KEYPOINT_DTYPE array per frame; K [n_frames][4], Rt
        [n_frames][12] float64; reg [n_frames]; tracks as pgx_tracks_get gives them (track_offsets [n_tracks + 1], nodes
        [n_nodes][2]) or, with nodes=None, the `tracks` list of tracks_host; xyz [n_tracks][3]; track_flags [n_tracks] or None.
        -> dict(Rt [F][12], P [F][12], frame_stats [F][4], frame_err [F][2], node_inlier [n_nodes], report [8])"""
        head, nf, n, n_nodes = _host_problem(kps_per_frame, K, Rt, reg, track_offsets, nodes, xyz, track_flags)
        Rt_out, P_out = np.zeros((nf, 12)), np.zeros((nf, 12))
        stats, ferr = np.zeros((nf, 4), dtype=np.int32), np.zeros((nf, 2))
        ni, report = np.zeros(max(n_nodes, 1), dtype=np.int32), np.zeros(8, dtype=np.int32)
        self._chk(self._L.pgx_register_frames(
            self._h, *map(_ptr, head), int(n_samples), inlier_px, int(min_inliers), int(refine_iters), seed, _ptr(Rt_out),
            _ptr(P_out), _ptr(stats), _ptr(ferr), _ptr(ni), _ptr(report)))
        return dict(Rt=Rt_out, P=P_out, frame_stats=stats, frame_err=ferr, node_inlier=ni[:n_nodes], report=report)

    # -- track consensus: outlier observations dropped from tracks (pgx_track_consensus*) ------------------
    def track_consensus_dev(self, d_kp, F, stride, n_frames, d_P, d_offsets, d_nodes, d_track_summary, max_tracks, d_offsets_out,
                            d_nodes_out, d_summary_out, d_track_map, d_xyz_out, d_flags_out, d_track_stats, d_report, inlier_px=4.0,
                            min_parallax_deg=1.0, min_inliers=2, min_len=2, max_hyp=256, seed=0, d_track_of=None, d_frame_ids=None):
        """A deterministic two-view RANSAC per track of the graph, where it sits in HBM, and the compacted graph without the
        observations its winner rejects (pgx.h: track consensus).  It sits between tracks_dev and triangulate_tracks_dev.
        d_P [n_frames][12] float64; d_offsets_out [max_tracks + 1], d_nodes_out [n_frames * stride][2], d_summary_out [8] int32 in
        tracks_dev's layout (they must not be the inputs); d_track_map [max_tracks] int32; d_xyz_out [max_tracks][3] float64
        and d_flags_out [max_tracks] int32 by the new index; d_track_stats [max_tracks][4] int32 by the old index; d_report [8]
        int32; d_track_of [n_frames][stride] int32 or None, rewritten in place.  n_tracks is read on the device: no sync."""
        self._chk(self._L.pgx_track_consensus_dev(
            self._h, _dptr(d_kp), int(F), int(stride), _dptr(d_frame_ids), int(n_frames), _dptr(d_P), _dptr(d_offsets),
            _dptr(d_nodes), _dptr(d_track_summary), int(max_tracks), inlier_px, min_parallax_deg, int(min_inliers), int(min_len),
            int(max_hyp), seed, _dptr(d_offsets_out), _dptr(d_nodes_out), _dptr(d_summary_out), _dptr(d_track_map), _dptr(d_xyz_out),
            _dptr(d_flags_out), _dptr(d_track_stats), _dptr(d_track_of), _dptr(d_report)))

    def track_consensus(self, kps_per_frame, cameras, track_offsets, nodes=None, inlier_px=4.0, min_parallax_deg=1.0,
                        min_inliers=2, min_len=2, max_hyp=256, seed=0):
        """The host form (pgx_track_consensus).  kps_per_frame: one KEYPOINT_DTYPE array per frame; cameras [n_frames][3][4]
        (or [n_frames][12]) float64, NaN rows for frames without a pose.  Tracks as pgx_tracks_get gives them (track_offsets
        [n_tracks + 1], nodes [n_nodes][2]) or, with nodes=None, the `tracks` list of tracks_host.
        -> dict(offsets [n_out + 1], nodes [nodes_out][2], summary [8], map [n], xyz [n_out][3], flags [n_out], stats [n][4],
                report [8])"""
        off, nd, kp, counts, flat = _host_tracks(kps_per_frame, track_offsets, nodes)
        P = np.ascontiguousarray(cameras, dtype=np.float64).reshape(len(kp), 12)
        n = len(off) - 1
        off_out, nd_out = np.zeros(n + 1, dtype=np.int32), np.zeros((max(len(nd), 1), 2), dtype=np.int32)
        summary, report = np.zeros(8, dtype=np.int32), np.zeros(8, dtype=np.int32)
        tmap, stats = np.zeros(max(n, 1), dtype=np.int32), np.zeros((max(n, 1), 4), dtype=np.int32)
        xyz, flags = np.zeros((max(n, 1), 3)), np.zeros(max(n, 1), dtype=np.int32)
        self._chk(self._L.pgx_track_consensus(
            self._h, _ptr(flat) if len(flat) else None, _ptr(counts), len(kp), _ptr(P), _ptr(off), _ptr(nd) if len(nd) else None, n,
            inlier_px, min_parallax_deg, int(min_inliers), int(min_len), int(max_hyp), seed, _ptr(off_out), _ptr(nd_out),
            _ptr(summary), _ptr(tmap), _ptr(xyz), _ptr(flags), _ptr(stats), _ptr(report)))
        n_out = int(summary[0])
        return dict(offsets=off_out[:n_out + 1], nodes=nd_out[:int(summary[1])], summary=summary, map=tmap[:n], xyz=xyz[:n_out],
                    flags=flags[:n_out], stats=stats[:n], report=report)

    # -- two-view verification of match lists by epipolar RANSAC (pgx_verify_pair*) ------------------------
    def verify_pairs_dev(self, d_kp, d_matches, d_counts, d_pairlist, M, stride, max_dist, d_out, d_F, d_stats, d_report,
                         n_samples=256, inlier_px=1.5, min_inliers=24, refit_iters=2, seed=0, d_F32=None, d_inlier=None,
                         d_sample_F=None, d_sample_count=None):
        """A robust fundamental matrix per image pair and the match lists with everything but its inliers rejected, where they
        sit in HBM (pgx.h: two-view geometric verification).  d_matches / d_out [M][stride] PAIR_DTYPE (d_out may be
        d_matches), d_F [M][9] float64, d_F32 [M][9] float32 or None (what match_guided_batch_dev takes), d_stats [M][8] int32,
        d_inlier [M][stride] int32 or None, d_sample_F [M][n_samples][9] float64 and d_sample_count [M][n_samples] int32 or
        None, d_report [8] int32.  No sync."""
        self._chk(self._L.pgx_verify_pairs_dev(
            self._h, _dptr(d_kp), _dptr(d_matches), _dptr(d_counts), _dptr(d_pairlist), int(M), int(stride), int(max_dist),
            int(n_samples), inlier_px, int(min_inliers), int(refit_iters), seed, _dptr(d_out), _dptr(d_F), _dptr(d_F32),
            _dptr(d_stats), _dptr(d_inlier), _dptr(d_sample_F), _dptr(d_sample_count), _dptr(d_report)))

    def verify_pair(self, kp1, kp2, matches, max_dist, n_samples=256, inlier_px=1.5, min_inliers=24, refit_iters=2, seed=0):
        """The host form (pgx_verify_pair): one pair, frame a in slot 1 and frame b in slot 2.  kp1, kp2: KEYPOINT_DTYPE
        arrays; matches: PAIR_DTYPE array (or int32 [n1][3]) of len(kp1) entries.
        -> dict(out [n1] PAIR_DTYPE, F [9], stats [8], inlier [n1])"""
        k1 = np.ascontiguousarray(kp1, dtype=KEYPOINT_DTYPE)
        k2 = np.ascontiguousarray(kp2, dtype=KEYPOINT_DTYPE)
        n1, n2 = len(k1), len(k2)
        ml = np.ascontiguousarray(matches)
        ml = ml if ml.dtype == PAIR_DTYPE else np.ascontiguousarray(ml, dtype=np.int32).reshape(-1, 3).view(PAIR_DTYPE).reshape(-1)
        if len(ml) != n1:
            raise ValueError("the match list must hold one entry per keypoint of the first frame")
        out, inl = np.zeros(max(n1, 1), dtype=PAIR_DTYPE), np.zeros(max(n1, 1), dtype=np.int32)
        F, stats = np.zeros(9), np.zeros(8, dtype=np.int32)
        self._chk(self._L.pgx_verify_pair(
            self._h, _ptr(k1) if n1 else None, n1, _ptr(k2) if n2 else None, n2, _ptr(ml) if n1 else None, int(max_dist),
            int(n_samples), inlier_px, int(min_inliers), int(refit_iters), seed, _ptr(out), _ptr(F), _ptr(stats), _ptr(inl)))
        return dict(out=out[:n1], F=F, stats=stats, inlier=inl[:n1])

    # -- relative pose per image pair and the choice of the initial pair (pgx_init_pair_dev, pgx_relative_pose) ------
    def init_pair_dev(self, d_kp, d_matches, d_counts, d_pairlist, M, F, stride, n_frames, max_dist, d_F, d_K, d_Rt_pair,
                      d_pair_stats, d_Rt_out, d_P_out, d_fixed_out, d_register_out, d_report, min_angle_deg=2.0,
                      min_front_frac=0.7, min_points=30, d_sigma=None, d_cand_Rt=None, d_frame_ids=None):
        """The first two cameras of a reconstruction from verification's F and the intrinsics, where they sit in HBM (pgx.h:
        relative pose per image pair).  d_matches [M][stride] PAIR_DTYPE (verify_pairs_dev's d_out), d_F [M][9] and d_K
        [n_frames][4] float64; d_Rt_pair [M][12] float64, d_pair_stats [M][8] int32, d_sigma [M] float64 or None, d_cand_Rt
        [M][4][12] float64 or None; d_Rt_out / d_P_out [n_frames][12] float64 and d_fixed_out / d_register_out [n_frames]
        int32, as triangulate_tracks_dev, bundle_adjust_dev and register_frames_dev take them; d_report [8] int32.  No sync."""
        self._chk(self._L.pgx_init_pair_dev(
            self._h, _dptr(d_kp), _dptr(d_matches), _dptr(d_counts), _dptr(d_pairlist), int(M), int(F), int(stride),
            _dptr(d_frame_ids), int(n_frames), int(max_dist), _dptr(d_F), _dptr(d_K), min_angle_deg, min_front_frac,
            int(min_points), _dptr(d_Rt_pair), _dptr(d_pair_stats), _dptr(d_sigma), _dptr(d_cand_Rt), _dptr(d_Rt_out),
            _dptr(d_P_out), _dptr(d_fixed_out), _dptr(d_register_out), _dptr(d_report)))

    def relative_pose(self, kp1, kp2, matches, max_dist, F, K_a, K_b, min_angle_deg=2.0, min_front_frac=0.7, min_points=30,
                      candidates=True):
        """The host form (pgx_relative_pose): one pair, frame a in slot 1 and frame b in slot 2.  kp1, kp2: KEYPOINT_DTYPE
        arrays; matches: PAIR_DTYPE array (or int32 [n1][3]) of len(kp1) entries; F [9] with h_a^T F h_b = 0; K_a, K_b
        (fx, fy, cx, cy).  -> dict(Rt [12], stats [8], sigma, cand_Rt [4][12] or None)"""
        k1 = np.ascontiguousarray(kp1, dtype=KEYPOINT_DTYPE)
        k2 = np.ascontiguousarray(kp2, dtype=KEYPOINT_DTYPE)
        n1, n2 = len(k1), len(k2)
        ml = np.ascontiguousarray(matches)
        ml = ml if ml.dtype == PAIR_DTYPE else np.ascontiguousarray(ml, dtype=np.int32).reshape(-1, 3).view(PAIR_DTYPE).reshape(-1)
        if len(ml) != n1:
            raise ValueError("the match list must hold one entry per keypoint of the first frame")
        Fm = np.ascontiguousarray(F, dtype=np.float64).reshape(9)
        Ka, Kb = np.ascontiguousarray(K_a, dtype=np.float64).reshape(4), np.ascontiguousarray(K_b, dtype=np.float64).reshape(4)
        Rt, stats, sigma = np.zeros(12), np.zeros(8, dtype=np.int32), np.zeros(1)
        cand = np.zeros((4, 12)) if candidates else None
        self._chk(self._L.pgx_relative_pose(
            self._h, _ptr(k1) if n1 else None, n1, _ptr(k2) if n2 else None, n2, _ptr(ml) if n1 else None, int(max_dist),
            _ptr(Fm), _ptr(Ka), _ptr(Kb), min_angle_deg, min_front_frac, int(min_points), _ptr(Rt), _ptr(stats), _ptr(sigma),
            _ptr(cand) if candidates else None))
        return dict(Rt=Rt, stats=stats, sigma=float(sigma[0]), cand_Rt=cand)

    # -- image-pair selection on a binary visual vocabulary (pgx_vocab_*, pgx_select_pairs*) -----------------------
    def vocab_quantize_dev(self, d_desc, d_counts, F, stride, d_vocab, V, d_word, d_wdist=None):
        """pgx_vocab_quantize_dev: d_desc [F][stride][8] uint32, d_vocab [V][8] uint32; d_word and d_wdist [F][stride] int32
        (d_wdist or None): the nearest word of every valid descriptor, ties to the smaller word.  No sync."""
        self._chk(self._L.pgx_vocab_quantize_dev(self._h, _dptr(d_desc), _dptr(d_counts), int(F), int(stride), _dptr(d_vocab),
                                                 int(V), _dptr(d_word), _dptr(d_wdist)))

    def vocab_train_dev(self, d_desc, d_counts, F, stride, V, d_vocab, d_report, iters=2, seed=0):
        """pgx_vocab_train_dev: k-majority on the device; d_vocab [V][8] uint32 out, d_report [4] int32.  No sync."""
        self._chk(self._L.pgx_vocab_train_dev(self._h, _dptr(d_desc), _dptr(d_counts), int(F), int(stride), int(V), int(iters),
                                              seed, _dptr(d_vocab), _dptr(d_report)))

    def select_pairs_dev(self, d_desc, d_counts, F, stride, d_vocab, V, max_pairs, d_pairlist, d_pair_score, d_summary,
                         weighting=1, top_k=10, window=0, min_score=1, d_scores=None):
        """pgx_select_pairs_dev: d_pairlist [max_pairs][2] int32 (rows past the count hold -1), d_pair_score [max_pairs] int32,
        d_scores [F][F] int32 or None, d_summary [8] int32 ([0] = the pairs selected).  No sync."""
        self._chk(self._L.pgx_select_pairs_dev(self._h, _dptr(d_desc), _dptr(d_counts), int(F), int(stride), _dptr(d_vocab),
                                               int(V), int(weighting), int(top_k), int(window), int(min_score), int(max_pairs),
                                               _dptr(d_pairlist), _dptr(d_pair_score), _dptr(d_scores), _dptr(d_summary)))

    @staticmethod
    def _host_slots(desc, counts):
        d = np.ascontiguousarray(desc, dtype=np.uint32)
        if d.ndim != 3 or d.shape[2] != 8:
            raise ValueError("descriptors must be [F][stride][8] uint32 (256-bit)")
        cn = np.ascontiguousarray(counts, dtype=np.int32).reshape(-1)
        if len(cn) != d.shape[0]:
            raise ValueError("one count per slot")
        return d, cn

    def vocab_train(self, desc, counts, V, iters=2, seed=0):
        """The host form (pgx_vocab_train): desc [F][stride][8] uint32, counts [F] -> (vocab [V][8] uint32, report [4])."""
        d, cn = self._host_slots(desc, counts)
        vocab, report = np.zeros((max(int(V), 1), 8), dtype=np.uint32), np.zeros(4, dtype=np.int32)
        self._chk(self._L.pgx_vocab_train(self._h, _ptr(d), _ptr(cn), d.shape[0], d.shape[1], int(V), int(iters), seed,
                                          _ptr(vocab), _ptr(report)))
        return vocab, report

    def select_pairs(self, desc, counts, vocab, weighting=1, top_k=10, window=0, min_score=1, max_pairs=None, scores=False):
        """The host form (pgx_select_pairs) -> dict(pairs [n][2] trimmed to summary[0], pair_score [n], scores [F][F] or None,
        summary [8]).  max_pairs defaults to all F (F - 1) / 2; a smaller one that cuts the list raises CapacityError."""
        d, cn = self._host_slots(desc, counts)
        vc = np.ascontiguousarray(vocab, dtype=np.uint32).reshape(-1, 8)
        F = d.shape[0]
        cap = F * (F - 1) // 2 if max_pairs is None else int(max_pairs)
        pl, ps = np.zeros((max(cap, 1), 2), dtype=np.int32), np.zeros(max(cap, 1), dtype=np.int32)
        sc = np.zeros((F, F), dtype=np.int32) if scores else None
        summary = np.zeros(8, dtype=np.int32)
        self._chk(self._L.pgx_select_pairs(self._h, _ptr(d), _ptr(cn), F, d.shape[1], _ptr(vc), len(vc), int(weighting), int(top_k),
                                           int(window), int(min_score), cap, _ptr(pl), _ptr(ps), _ptr(sc), _ptr(summary)))
        n = min(int(summary[0]), cap)
        return dict(pairs=pl[:n], pair_score=ps[:n], scores=sc, summary=summary)

    # -- dense depth maps by census plane sweep and the cross-view filter (pgx_gray_batch_dev, pgx_depth_*) --------
    def gray_batch_dev(self, d_rgba, F, W, H, d_gray):
        """pgx_gray_batch_dev: d_gray [F][H][W] float32 from d_rgba [F][H][W] in the context's source format, through the
        context's dewarp map when one is set.  No sync."""
        self._chk(self._L.pgx_gray_batch_dev(self._h, _dptr(d_rgba), int(F), int(W), int(H), _dptr(d_gray)))

    def depth_maps_dev(self, d_gray, F, W, H, n_frames, d_P, d_views, R, S, d_range, D, d_kq8, d_depth, d_flags, d_summary,
                       agg_radius=2, min_views=2, max_cost=2**30, d_cost=None, d_warp=None, d_planes=None, d_frame_ids=None):
        """pgx_depth_maps_dev: one depth map per row of d_views [R][1 + S] int32 (reference frame, then sources; -1 = none).
        d_gray [F][H][W] float32 by slot, d_P [n_frames][12] float64 by frame number, d_range [R][2] float64 = (z_near,
        z_far); d_kq8 / d_flags [R][H][W] int32, d_depth [R][H][W] float64, d_summary [8] int32; d_cost [R][H][W] int32,
        d_warp [R][S][12] and d_planes [R][D] float64 or None.  No sync."""
        self._chk(self._L.pgx_depth_maps_dev(
            self._h, _dptr(d_gray), int(F), int(W), int(H), _dptr(d_frame_ids), int(n_frames), _dptr(d_P), _dptr(d_views), int(R),
            int(S), _dptr(d_range), int(D), int(agg_radius), int(min_views), int(max_cost), _dptr(d_kq8), _dptr(d_depth),
            _dptr(d_cost), _dptr(d_flags), _dptr(d_warp), _dptr(d_planes), _dptr(d_summary)))

    def depth_fuse_dev(self, d_depth, d_views, R, S, W, H, n_frames, d_P, max_points, d_xyz, d_src, d_summary, rel_tol=0.05,
                       min_agree=2, d_agree=None):
        """pgx_depth_fuse_dev: the pixels of d_depth [R][H][W] that min_agree other maps of the call confirm within rel_tol, in
        (r, v, u) order: d_xyz [max_points][3] float64, d_src [max_points][2] int32 = (r, v W + u), d_agree [R][H][W] int32 or
        None, d_summary [4] int32 ([0] = the pixels kept).  More than max_points: CapacityError from check_status.  No sync."""
        self._chk(self._L.pgx_depth_fuse_dev(
            self._h, _dptr(d_depth), _dptr(d_views), int(R), int(S), int(W), int(H), int(n_frames), _dptr(d_P), float(rel_tol),
            int(min_agree), int(max_points), _dptr(d_xyz), _dptr(d_src), _dptr(d_agree), _dptr(d_summary)))

    def depth_maps(self, gray, cameras, views, depth_range, D=64, agg_radius=2, min_views=2, max_cost=2**30, cost=True,
                   warp=True, planes=True):
        """The host form (pgx_depth_maps).  gray [n_frames][H][W] float32, cameras [n_frames][3][4] (or [n_frames][12]) float64,
        views [R][1 + S] int32, depth_range [R][2] float64 -> dict(kq8, depth, cost, flags [R][H][W], warp [R][S][12],
        planes [R][D], summary [8]); cost, warp and planes are None when not asked for."""
        g = np.ascontiguousarray(gray, dtype=np.float32)
        nf, H, W = g.shape
        P = np.ascontiguousarray(cameras, dtype=np.float64).reshape(nf, 12)
        vw = np.ascontiguousarray(views, dtype=np.int32)
        vw = vw.reshape(-1, vw.shape[-1])
        R, S = vw.shape[0], vw.shape[1] - 1
        rg = np.ascontiguousarray(depth_range, dtype=np.float64).reshape(R, 2)
        shape = (max(R, 1), H, W)
        kq8, dep, fl = np.zeros(shape, np.int32), np.zeros(shape), np.zeros(shape, np.int32)
        cs = np.zeros(shape, np.int32) if cost else None
        wp = np.zeros((max(R, 1), S, 12)) if warp else None
        pl = np.zeros((max(R, 1), int(D))) if planes else None
        summary = np.zeros(8, dtype=np.int32)
        self._chk(self._L.pgx_depth_maps(self._h, _ptr(g), nf, W, H, _ptr(P), _ptr(vw), R, S, _ptr(rg), int(D), int(agg_radius),
                                         int(min_views), int(max_cost), _ptr(kq8), _ptr(dep), _ptr(cs), _ptr(fl), _ptr(wp), _ptr(pl),
                                         _ptr(summary)))
        return dict(kq8=kq8[:R], depth=dep[:R], cost=None if cs is None else cs[:R], flags=fl[:R],
                    warp=None if wp is None else wp[:R], planes=None if pl is None else pl[:R], summary=summary)

    def depth_fuse(self, depth, views, cameras, rel_tol=0.05, min_agree=2, max_points=None, agree=True):
        """The host form (pgx_depth_fuse).  depth [R][H][W] float64, views [R][1 + S] int32, cameras [n_frames][3][4] float64 ->
        dict(xyz [n][3], src [n][2] trimmed to min(summary[0], max_points), agree [R][H][W] or None, summary [4]).  max_points
        defaults to every pixel; a smaller one that cuts the list raises CapacityError."""
        d = np.ascontiguousarray(depth, dtype=np.float64)
        R, H, W = d.shape
        vw = np.ascontiguousarray(views, dtype=np.int32)
        vw = vw.reshape(R, vw.shape[-1])
        P = np.ascontiguousarray(cameras, dtype=np.float64).reshape(-1, 12)
        cap = R * H * W if max_points is None else int(max_points)
        xyz, src = np.zeros((max(cap, 1), 3)), np.zeros((max(cap, 1), 2), dtype=np.int32)
        ag = np.zeros((max(R, 1), H, W), dtype=np.int32) if agree else None
        summary = np.zeros(4, dtype=np.int32)
        self._chk(self._L.pgx_depth_fuse(self._h, _ptr(d), _ptr(vw), R, vw.shape[1] - 1, W, H, len(P), _ptr(P), float(rel_tol),
                                         int(min_agree), cap, _ptr(xyz), _ptr(src), _ptr(ag), _ptr(summary)))
        n = min(int(summary[0]), cap)
        return dict(xyz=xyz[:n], src=src[:n], agree=None if ag is None else ag[:R], summary=summary)

    # -- the plan of the dense stage from the sparse model (pgx_dense_views*) ---------------------------------------
    def dense_views_dev(self, d_offsets, d_nodes, d_track_summary, max_tracks, max_nodes, d_xyz, n_frames, d_P, R, S, d_views,
                        d_range, d_ref_stats, d_report, d_track_flags=None, d_refs=None, min_angle_deg=2.0, max_angle_deg=45.0,
                        min_shared=8, min_points=8, q_near_pm=10, q_far_pm=990, grow=1.25, d_pair_counts=None):
        """pgx_dense_views_dev: per reference frame (d_refs [R] int32, or None: every frame, R = n_frames) its S source frames
        and the depth interval to sweep, from the track graph (d_offsets, d_nodes [max_nodes][2], d_track_summary), the track
        points d_xyz [max_tracks][3] (d_track_flags or None) and d_P [n_frames][12]: d_views [R][1 + S] int32 and d_range
        [R][2] float64 as pgx_depth_maps_dev takes them, d_ref_stats [R][4], d_report [8] int32, d_pair_counts
        [R][n_frames][2] int32 or None.  No sync."""
        self._chk(self._L.pgx_dense_views_dev(
            self._h, _dptr(d_offsets), _dptr(d_nodes), _dptr(d_track_summary), int(max_tracks), int(max_nodes), _dptr(d_xyz),
            _dptr(d_track_flags), int(n_frames), _dptr(d_P), _dptr(d_refs), int(R), int(S), float(min_angle_deg),
            float(max_angle_deg), int(min_shared), int(min_points), int(q_near_pm), int(q_far_pm), float(grow), _dptr(d_views),
            _dptr(d_range), _dptr(d_pair_counts), _dptr(d_ref_stats), _dptr(d_report)))

    def dense_views(self, track_offsets, nodes, xyz, cameras, S, refs=None, track_flags=None, min_angle_deg=2.0,
                    max_angle_deg=45.0, min_shared=8, min_points=8, q_near_pm=10, q_far_pm=990, grow=1.25, pair_counts=True,
                    ref_stats=True):
        """The host form (pgx_dense_views).  Tracks as (track_offsets, nodes [n_nodes][2]), xyz [n_tracks][3], cameras
        [n_frames][3][4] (or [n_frames][12]) float64, refs [R] or None (every frame) -> dict(views [R][1 + S], range [R][2],
        pair_counts [R][n_frames][2], ref_stats [R][4], report [8]); pair_counts and ref_stats are None when not asked for."""
        off = np.ascontiguousarray(track_offsets, dtype=np.int32).reshape(-1)
        nd = np.ascontiguousarray(nodes, dtype=np.int32).reshape(-1, 2)
        n = len(off) - 1
        X = np.ascontiguousarray(xyz, dtype=np.float64).reshape(n, 3)
        fl = None if track_flags is None else np.ascontiguousarray(track_flags, dtype=np.int32).reshape(n)
        P = np.ascontiguousarray(cameras, dtype=np.float64).reshape(-1, 12)
        nf = len(P)
        rf = None if refs is None else np.ascontiguousarray(refs, dtype=np.int32).reshape(-1)
        R = nf if rf is None else len(rf)
        vw, rg = np.zeros((max(R, 1), 1 + int(S)), np.int32), np.zeros((max(R, 1), 2))
        pc = np.zeros((max(R, 1), nf, 2), np.int32) if pair_counts else None
        st = np.zeros((max(R, 1), 4), np.int32) if ref_stats else None
        report = np.zeros(8, dtype=np.int32)
        self._chk(self._L.pgx_dense_views(
            self._h, _ptr(off), _ptr(nd) if len(nd) else None, n, _ptr(X) if n else None, _ptr(fl) if n else None, nf, _ptr(P),
            _ptr(rf) if R else None, R, int(S), float(min_angle_deg), float(max_angle_deg), int(min_shared), int(min_points),
            int(q_near_pm), int(q_far_pm), float(grow), _ptr(vw), _ptr(rg), _ptr(pc), _ptr(st), _ptr(report)))
        return dict(views=vw[:R], range=rg[:R], pair_counts=None if pc is None else pc[:R],
                    ref_stats=None if st is None else st[:R], report=report)

    # -- the fused points merged into one cloud with normals and colour (pgx_rgba8_batch*, pgx_cloud_merge*) ---------
    def rgba8_batch_dev(self, d_rgba, F, W, H, d_rgba8):
        """pgx_rgba8_batch_dev: d_rgba8 [F][H][W] uint32 = pgx_dewarp's pixel of every frame of d_rgba at 8 bits a channel
        (channel c in bits 8 c .. 8 c + 7).  No sync."""
        self._chk(self._L.pgx_rgba8_batch_dev(self._h, _dptr(d_rgba), int(F), int(W), int(H), _dptr(d_rgba8)))

    def cloud_merge_dev(self, d_xyz, d_src, d_count, max_in, d_depth, d_views, R, S, W, H, n_frames, d_P, cell, origin, max_points,
                        d_out_xyz, d_out_normal, d_out_rgba8, d_out_info, d_report, d_rgba8=None, F=0, d_frame_ids=None,
                        normal_step=1, disc_tol=0.02, min_support=1, d_pt_normal=None, d_cell_of=None):
        """pgx_cloud_merge_dev: the list d_xyz [max_in][3] float64 / d_src [max_in][2] int32 of pgx_depth_fuse_dev (d_count int32
        on the device, e.g. the filter's d_summary, or None: max_in entries) merged into one point per occupied cell of the grid
        of `cell` at `origin`: d_out_xyz [max_points][3] float64, d_out_normal [max_points][3] float32, d_out_rgba8 [max_points]
        uint32, d_out_info [max_points][4] int32 = (cnt, nn, nc, first), d_report [8] int32 ([6] = the cells kept); d_pt_normal
        [max_in][3] and d_cell_of [max_in] int32 or None.  More than max_points: CapacityError from check_status.  No sync."""
        ox, oy, oz = (float(x) for x in origin)
        self._chk(self._L.pgx_cloud_merge_dev(
            self._h, _dptr(d_xyz), _dptr(d_src), _dptr(d_count), int(max_in), _dptr(d_depth), _dptr(d_views), int(R), int(S), int(W),
            int(H), int(n_frames), _dptr(d_P), _dptr(d_rgba8), int(F), _dptr(d_frame_ids), float(cell), ox, oy, oz, int(normal_step),
            float(disc_tol), int(min_support), int(max_points), _dptr(d_out_xyz), _dptr(d_out_normal), _dptr(d_out_rgba8),
            _dptr(d_out_info), _dptr(d_pt_normal), _dptr(d_cell_of), _dptr(d_report)))

    def rgba8_batch(self, rgba):
        """The host form (pgx_rgba8_batch).  rgba [F][H][W][4] in the context's source format (uint16, or uint8 after
        set_source_format(PGX_SRC_RGBA8)) -> [F][H][W] uint32."""
        a = np.ascontiguousarray(rgba, dtype=getattr(self, "_src_dtype", np.uint16))
        F, H, W = a.shape[:3]
        out = np.zeros((F, H, W), dtype=np.uint32)
        self._chk(self._L.pgx_rgba8_batch(self._h, _ptr(a), F, W, H, _ptr(out)))
        return out

    def cloud_merge(self, xyz, src, depth, views, cameras, cell, origin, rgba8=None, normal_step=1, disc_tol=0.02, min_support=1,
                    max_points=None, pt_normal=True, cell_of=True):
        """The host form (pgx_cloud_merge).  xyz [n][3] float64 and src [n][2] int32 as depth_fuse returns them, depth [R][H][W],
        views [R][1 + S], cameras [n_frames][3][4], rgba8 [n_frames][H][W] uint32 or None -> dict(xyz [m][3], normal [m][3]
        float32, rgba8 [m], info [m][4] trimmed to min(report[6], max_points), pt_normal [n][3], cell_of [n] or None, report [8]).
        max_points defaults to n; a smaller one that cuts the cloud raises CapacityError."""
        X, sr, d, vw, P, col = _dense_inputs(xyz, src, depth, views, cameras, rgba8)
        n, (R, H, W) = len(X), d.shape
        cap = n if max_points is None else int(max_points)
        m = max(cap, 1)
        oxyz, onrm = np.zeros((m, 3)), np.zeros((m, 3), dtype=np.float32)
        orgb, oinf = np.zeros(m, dtype=np.uint32), np.zeros((m, 4), dtype=np.int32)
        pn = np.zeros((max(n, 1), 3), dtype=np.int32) if pt_normal else None
        co = np.zeros(max(n, 1), dtype=np.int32) if cell_of else None
        report = np.zeros(8, dtype=np.int32)
        ox, oy, oz = (float(x) for x in origin)
        self._chk(self._L.pgx_cloud_merge(
            self._h, _ptr(X) if n else None, _ptr(sr) if n else None, n, _ptr(d), _ptr(vw), R, vw.shape[1] - 1, W, H, len(P), _ptr(P),
            _ptr(col), float(cell), ox, oy, oz, int(normal_step), float(disc_tol), int(min_support), cap, _ptr(oxyz), _ptr(onrm),
            _ptr(orgb), _ptr(oinf), _ptr(pn), _ptr(co), _ptr(report)))
        k = min(int(report[6]), cap)
        return dict(xyz=oxyz[:k], normal=onrm[:k], rgba8=orgb[:k], info=oinf[:k], pt_normal=None if pn is None else pn[:n],
                    cell_of=None if co is None else co[:n], report=report)

    # -- a triangle mesh from the depth maps: TSDF grid and surface nets (pgx_mesh*) -------------------------------
    def mesh_dev(self, d_xyz, d_src, d_count, max_in, d_depth, d_views, R, S, W, H, n_frames, d_P, cell, origin, max_voxels,
                 max_vertices, max_tris, d_out_xyz, d_out_normal, d_out_rgba8, d_out_info, d_out_tri, d_report, d_agree=None,
                 min_agree=0, d_rgba8=None, F=0, d_frame_ids=None, band=1, trunc_cells=3, min_weight=1):
        """pgx_mesh_dev: the list, maps, cameras and colours as for cloud_merge_dev (d_agree [R][H][W] int32, the filter's optional
        output, or None) -> the surface-nets mesh of the TSDF on the nodes within `band` cells of the list's points: d_out_xyz
        [max_vertices][3] float64, d_out_normal [max_vertices][3] float32, d_out_rgba8 [max_vertices] uint32, d_out_info
        [max_vertices][4] int32 = (c_0, c_1, c_2, mask | k << 8), d_out_tri [max_tris][3] int32, d_report [8] int32 ([3] voxels,
        [5] vertices, [6] triangles).  A capacity exceeded: CapacityError from check_status.  No sync."""
        ox, oy, oz = (float(x) for x in origin)
        self._chk(self._L.pgx_mesh_dev(
            self._h, _dptr(d_xyz), _dptr(d_src), _dptr(d_count), int(max_in), _dptr(d_depth), _dptr(d_views), int(R), int(S), int(W),
            int(H), int(n_frames), _dptr(d_P), _dptr(d_agree), int(min_agree), _dptr(d_rgba8), int(F), _dptr(d_frame_ids), float(cell),
            ox, oy, oz, int(band), int(trunc_cells), int(min_weight), int(max_voxels), int(max_vertices), int(max_tris),
            _dptr(d_out_xyz), _dptr(d_out_normal), _dptr(d_out_rgba8), _dptr(d_out_info), _dptr(d_out_tri), _dptr(d_report)))

    def mesh(self, xyz, src, depth, views, cameras, cell, origin, agree=None, min_agree=0, rgba8=None, band=1, trunc_cells=3,
             min_weight=1, max_voxels=None, max_vertices=None, max_tris=None):
        """The host form (pgx_mesh).  xyz [n][3] float64 and src [n][2] int32 as depth_fuse returns them, depth [R][H][W], views
        [R][1 + S], cameras [n_frames][3][4], agree [R][H][W] int32 or None, rgba8 [n_frames][H][W] uint32 or None ->
        dict(xyz [m][3], normal [m][3] float32, rgba8 [m], info [m][4], tri [t][3] int32, report [8]), trimmed to the counts of
        the report.  max_voxels defaults to (2 band)^3 n, max_vertices to max_voxels, max_tris to 6 max_voxels (none of them can
        then be exceeded); a smaller one that cuts the mesh raises CapacityError."""
        X, sr, d, vw, P, col = _dense_inputs(xyz, src, depth, views, cameras, rgba8)
        n, (R, H, W) = len(X), d.shape
        ag = None if agree is None else np.ascontiguousarray(agree, dtype=np.int32).reshape(R, H, W)
        lim = 1 << 28
        nvox = min((2 * int(band)) ** 3 * n, lim) if max_voxels is None else int(max_voxels)
        nv = nvox if max_vertices is None else int(max_vertices)
        nt = min(6 * nvox, lim) if max_tris is None else int(max_tris)
        out = _mesh_outputs(nv, nt)
        ox, oy, oz = (float(x) for x in origin)
        self._chk(self._L.pgx_mesh(
            self._h, _ptr(X) if n else None, _ptr(sr) if n else None, n, _ptr(d), _ptr(vw), R, vw.shape[1] - 1, W, H, len(P), _ptr(P),
            _ptr(ag), int(min_agree), _ptr(col), float(cell), ox, oy, oz, int(band), int(trunc_cells), int(min_weight), nvox, nv, nt,
            *(_ptr(o) for o in out)))
        return _mesh_result(out, nv, nt)

    # -- the mesh cleaned: small components dropped, smoothed, normals again (pgx_mesh_clean*) ---------------------
    def mesh_clean_dev(self, d_xyz, d_normal, d_rgba8, d_info, d_tri, d_counts, max_vertices, max_tris, cell, origin,
                       max_out_vertices, max_out_tris, d_out_xyz, d_out_normal, d_out_rgba8, d_out_info, d_out_tri, d_report,
                       min_tris=1, min_frac_pm=0, iters=0, lam=0.5, mu=-0.53, d_vertex_map=None, d_comp=None):
        """pgx_mesh_clean_dev: the mesh d_xyz .. d_tri as mesh_dev writes it (d_counts int32 [8] on the device, mesh_dev's
        d_report, or None: the capacities) without the components of fewer than min_tris triangles or fewer than
        min_frac_pm / 1000 of the largest one's, after `iters` Taubin steps (lam, mu) on the grid of `cell` at `origin`, with the
        normals of the smoothed triangles: d_out_xyz [max_out_vertices][3] float64, d_out_normal [max_out_vertices][3] float32,
        d_out_rgba8 [max_out_vertices] uint32, d_out_info [max_out_vertices][4] int32, d_out_tri [max_out_tris][3] int32,
        d_report [8] int32 ([5] vertices, [6] triangles out); d_vertex_map and d_comp [max_vertices] int32 or None.  A capacity
        exceeded: CapacityError from check_status.  No sync."""
        ox, oy, oz = (float(x) for x in origin)
        self._chk(self._L.pgx_mesh_clean_dev(
            self._h, _dptr(d_xyz), _dptr(d_normal), _dptr(d_rgba8), _dptr(d_info), _dptr(d_tri), _dptr(d_counts), int(max_vertices),
            int(max_tris), float(cell), ox, oy, oz, int(min_tris), int(min_frac_pm), int(iters), float(lam), float(mu),
            int(max_out_vertices), int(max_out_tris), _dptr(d_out_xyz), _dptr(d_out_normal), _dptr(d_out_rgba8), _dptr(d_out_info),
            _dptr(d_out_tri), _dptr(d_vertex_map), _dptr(d_comp), _dptr(d_report)))

    def mesh_clean(self, xyz, normal, rgba8, info, tri, cell, origin, min_tris=1, min_frac_pm=0, iters=0, lam=0.5, mu=-0.53,
                   max_out_vertices=None, max_out_tris=None, vertex_map=True, comp=True):
        """The host form (pgx_mesh_clean).  xyz [n][3] float64, normal [n][3] float32, rgba8 [n] uint32, info [n][4] int32 and tri
        [t][3] int32 as mesh returns them -> dict(xyz [m][3], normal [m][3] float32, rgba8 [m], info [m][4], tri [k][3] int32
        trimmed to the counts of the report, vertex_map [n], comp [n] or None, report [8]).  The capacities default to n and t
        (they can then not be exceeded); a smaller one that cuts the mesh raises CapacityError."""
        arrays = _mesh_inputs(xyz, normal, rgba8, info, tri)
        n, t = len(arrays[0]), len(arrays[4])
        nv = n if max_out_vertices is None else int(max_out_vertices)
        nt = t if max_out_tris is None else int(max_out_tris)
        out = _mesh_outputs(nv, nt)
        vm = np.zeros(max(n, 1), dtype=np.int32) if vertex_map else None
        cp = np.zeros(max(n, 1), dtype=np.int32) if comp else None
        ox, oy, oz = (float(x) for x in origin)
        self._chk(self._L.pgx_mesh_clean(
            self._h, *(_ptr(a) if len(a) else None for a in arrays), n, t, float(cell), ox, oy, oz, int(min_tris), int(min_frac_pm),
            int(iters), float(lam), float(mu), nv, nt, *(_ptr(o) for o in out[:5]), _ptr(vm), _ptr(cp), _ptr(out[5])))
        return _mesh_result(out, nv, nt, vertex_map=None if vm is None else vm[:n], comp=None if cp is None else cp[:n])

    # -- the mesh decimated: adaptive vertex clustering over grid blocks (pgx_mesh_decimate*) ----------------------
    def mesh_decimate_dev(self, d_xyz, d_normal, d_rgba8, d_info, d_tri, d_counts, max_vertices, max_tris, cell, origin,
                          max_out_vertices, max_out_tris, d_out_xyz, d_out_normal, d_out_rgba8, d_out_info, d_out_tri, d_report,
                          lmin=0, lmax=3, flat_q=1015, d_vertex_map=None, d_level=None):
        """pgx_mesh_decimate_dev: the mesh d_xyz .. d_tri in mesh_dev's layout (d_counts int32 [8] on the device: the report of
        mesh_dev, mesh_clean_dev or of this call, or None: the capacities) with the vertices of a grid block of 2^l cells, l in
        lmin .. lmax, merged where the block's triangle normals agree (|sum m| >= flat_q / 1024 of their number) on the grid of
        `cell` at `origin`: d_out_xyz [max_out_vertices][3] float64, d_out_normal [max_out_vertices][3] float32, d_out_rgba8
        [max_out_vertices] uint32, d_out_info [max_out_vertices][4] int32 = (name, L, members, 0), d_out_tri [max_out_tris][3] int32,
        d_report [8] int32 ([5] vertices, [6] triangles out); d_vertex_map and d_level [max_vertices] int32 or None.  A capacity
        exceeded: CapacityError from check_status.  No sync."""
        ox, oy, oz = (float(x) for x in origin)
        self._chk(self._L.pgx_mesh_decimate_dev(
            self._h, _dptr(d_xyz), _dptr(d_normal), _dptr(d_rgba8), _dptr(d_info), _dptr(d_tri), _dptr(d_counts), int(max_vertices),
            int(max_tris), float(cell), ox, oy, oz, int(lmin), int(lmax), int(flat_q), int(max_out_vertices), int(max_out_tris),
            _dptr(d_out_xyz), _dptr(d_out_normal), _dptr(d_out_rgba8), _dptr(d_out_info), _dptr(d_out_tri), _dptr(d_vertex_map),
            _dptr(d_level), _dptr(d_report)))

    def mesh_decimate(self, xyz, normal, rgba8, info, tri, cell, origin, lmin=0, lmax=3, flat_q=1015, max_out_vertices=None,
                      max_out_tris=None, vertex_map=True, level=True):
        """The host form (pgx_mesh_decimate).  xyz [n][3] float64, normal [n][3] float32, rgba8 [n] uint32, info [n][4] int32 and tri
        [t][3] int32 as mesh or mesh_clean return them -> dict(xyz [m][3], normal [m][3] float32, rgba8 [m], info [m][4], tri [k][3]
        int32 trimmed to the counts of the report, vertex_map [n], level [n] or None, report [8]).  The capacities default to n and
        t (they can then not be exceeded); a smaller one that cuts the mesh raises CapacityError."""
        arrays = _mesh_inputs(xyz, normal, rgba8, info, tri)
        n, t = len(arrays[0]), len(arrays[4])
        nv = n if max_out_vertices is None else int(max_out_vertices)
        nt = t if max_out_tris is None else int(max_out_tris)
        out = _mesh_outputs(nv, nt)
        vm = np.zeros(max(n, 1), dtype=np.int32) if vertex_map else None
        lv = np.zeros(max(n, 1), dtype=np.int32) if level else None
        ox, oy, oz = (float(x) for x in origin)
        self._chk(self._L.pgx_mesh_decimate(
            self._h, *(_ptr(a) if len(a) else None for a in arrays), n, t, float(cell), ox, oy, oz, int(lmin), int(lmax), int(flat_q),
            nv, nt, *(_ptr(o) for o in out[:5]), _ptr(vm), _ptr(lv), _ptr(out[5])))
        return _mesh_result(out, nv, nt, vertex_map=None if vm is None else vm[:n], level=None if lv is None else lv[:n])

    # -- multi-GPU: the context's own RCCL communicator (pgx_comm_*) ------------------------------
    def comm_init(self, rank, world, unique_id):
        """Collective: every rank calls this with the 128 bytes rank 0 got from comm_unique_id()."""
        buf = (C.c_char * 128).from_buffer_copy(bytes(unique_id))
        self._chk(self._L.pgx_comm_init(self._h, int(rank), int(world), buf))

    def comm_destroy(self):
        self._chk(self._L.pgx_comm_destroy(self._h))

    def comm_info(self):
        r, w = C.c_int(0), C.c_int(0)
        self._chk(self._L.pgx_comm_info(self._h, C.byref(r), C.byref(w)))
        return r.value, w.value

    def allgather_dev(self, d_buf, bytes_per_rank):
        """In-place all-gather of fixed-size records on the context's stream (rank-major buffer)."""
        self._chk(self._L.pgx_allgather_dev(self._h, _dptr(d_buf), int(bytes_per_rank)))

    def sequence_step_dev(self, d_frames_local, n_local_frames, frame_slots, W, H, d_kp_local, d_desc_all, d_counts_all,
                          d_nraw_local, capacity, d_pairlist_local, n_local_pairs, pair_slots, d_out_all):
        """The four phases of one sharded job (detect -> all-gather -> match -> all-gather) in one C call."""
        self._chk(self._L.pgx_sequence_step_dev(self._h, _dptr(d_frames_local), int(n_local_frames), int(frame_slots), int(W), int(H),
                                                _dptr(d_kp_local), _dptr(d_desc_all), _dptr(d_counts_all), _dptr(d_nraw_local),
                                                int(capacity), _dptr(d_pairlist_local), int(n_local_pairs), int(pair_slots),
                                                _dptr(d_out_all)))

    def debug_counters(self):
        """The eight diagnostic counters of the match tail, summed over the calls since the last read: reading clears them."""
        out = np.zeros(8, dtype=np.int64)
        self._chk(self._L.pgx_debug_counters(self._h, _ptr(out)))
        return out.tolist()

    def match_stats(self):
        r, ev, ev0 = C.c_int(0), C.c_int64(0), C.c_int64(0)
        self._chk(self._L.pgx_match_stats(self._h, C.byref(r), C.byref(ev), C.byref(ev0)))
        return r.value, ev.value, ev0.value

    # -- measurement ------------------------------------------------------------------------
    def profile_enable(self, on=True):
        self._chk(self._L.pgx_profile_enable(self._h, 1 if on else 0))

    def profile_filter(self, name=None):
        self._chk(self._L.pgx_profile_filter(self._h, name.encode() if name else None))

    def profile_serialize(self, on=True):
        self._chk(self._L.pgx_profile_serialize(self._h, 1 if on else 0))

    def profile_reset(self):
        self._chk(self._L.pgx_profile_reset(self._h))

    def profile_get(self, name):
        n, ms = C.c_int(0), C.c_double(0.0)
        self._chk(self._L.pgx_profile_get(self._h, name.encode(), C.byref(n), C.byref(ms)))
        return n.value, ms.value


def comm_unique_id():
    """128 bytes from ncclGetUniqueId (rank 0 makes them, the host hands them to every rank)."""
    buf = (C.c_char * 128)()
    rc = _lib.lib().pgx_comm_unique_id(buf)
    if rc != PGX_OK:
        raise PgxError(rc, "pgx_comm_unique_id: librccl could not be loaded or ncclGetUniqueId failed")
    return bytes(buf)


def tracks_host(counts, pair_list, lists, max_dist, min_len=2, gates=None):
    """The host form of the track graph (pgx_tracks_*: sequential, no GPU work; same semantics as Engine.tracks_dev).
    counts [F]; pair_list [(a, b)]; lists[m] = that pair's match list ([n][3] ints or PAIR_DTYPE).
    -> (tracks, dropped_components, dropped_nodes); tracks = list of [(frame, keypoint)] lists in pgx_tracks_get's order.
    gates (a list, possibly empty): the split mode (pgx_tracks_finish_split, the rule of Engine.tracks_split_dev)
    -> (tracks, dropped_components, dropped_nodes, per_level); per_level[l] = nodes in tracks of level l, l = 0 .. len(gates)."""
    L = _lib.lib()
    c = np.ascontiguousarray(counts, dtype=np.int32)
    h = C.c_void_p()
    if L.pgx_tracks_create(_ptr(c), len(c), C.byref(h)) != PGX_OK:
        raise PgxError(PGX_E_BADARG, "pgx_tracks_create")
    try:
        for (a, b), rows in zip(pair_list, lists):
            rows = np.asarray(rows)
            if rows.dtype == PAIR_DTYPE:
                rows = np.stack([rows["k1"], rows["k2"], rows["dist"]], axis=1)
            rows = np.ascontiguousarray(rows.reshape(-1, 3)[:int(c[a])], dtype=np.int32)
            if L.pgx_tracks_add_pair(h, int(a), int(b), _ptr(rows), len(rows), int(max_dist)) != PGX_OK:
                raise PgxError(PGX_E_BADARG, "pgx_tracks_add_pair(%d, %d)" % (a, b))
        nt, nn, nd, ndn = C.c_int(0), C.c_int(0), C.c_int(0), C.c_int(0)
        if gates is None:
            if L.pgx_tracks_finish(h, int(min_len), C.byref(nt), C.byref(nn)) != PGX_OK:
                raise PgxError(PGX_E_BADARG, "pgx_tracks_finish")
        else:
            g = np.ascontiguousarray(list(gates), dtype=np.int32)
            summary = np.zeros(16, dtype=np.int32)
            if len(g) and g[0] >= max_dist:
                raise ArgumentException(PGX_E_BADARG, "gates must be below max_dist")
            if L.pgx_tracks_finish_split(h, _ptr(g) if len(g) else None, len(g), int(min_len), C.byref(nt), C.byref(nn),
                                         _ptr(summary)) != PGX_OK:
                raise ArgumentException(PGX_E_BADARG, "pgx_tracks_finish_split: gates %s" % g.tolist())
        off = np.zeros(nt.value + 1, dtype=np.int32)
        nodes = np.zeros((max(nn.value, 1), 2), dtype=np.int32)
        if L.pgx_tracks_get(h, _ptr(off), _ptr(nodes)) != PGX_OK or L.pgx_tracks_dropped(h, C.byref(nd), C.byref(ndn)) != PGX_OK:
            raise PgxError(PGX_E_BADARG, "pgx_tracks_get")
        tracks = [[(int(f), int(k)) for f, k in nodes[off[t]:off[t + 1]]] for t in range(nt.value)]
        if gates is None:
            return tracks, nd.value, ndn.value
        return tracks, nd.value, ndn.value, summary[8:9 + len(g)].tolist()
    finally:
        L.pgx_tracks_destroy(h)


def make_brief_pairs(seed, sigma, P):
    """Seeded table with the reference's generator formula (Utils.cs:14-38)."""
    out = np.zeros((P, 4), dtype=np.int32)
    rc = _lib.lib().pgx_make_brief_pairs(seed, int(sigma), int(P), _ptr(out))
    if rc != PGX_OK:
        raise PgxError(rc, "pgx_make_brief_pairs")
    return out


def make_steering(pairs, B):
    """The steering table of a pair table (pgx_make_steering) -> (pairs_rot int32 [B][P][4], dirs int32 [B][2])."""
    p = np.ascontiguousarray(pairs, dtype=np.int32).reshape(-1, 4)
    B = int(B)
    rot = np.zeros((max(B, 0), p.shape[0], 4), dtype=np.int32)
    dirs = np.zeros((max(B, 0), 2), dtype=np.int32)
    rc = _lib.lib().pgx_make_steering(_ptr(p), p.shape[0], B, _ptr(rot), _ptr(dirs))
    if rc != PGX_OK:
        raise ArgumentException(rc, "B must be a multiple of 4 in [4, 64] and every offset within +-2^20")
    return rot, dirs


def pyramid_dims(W, H, n_levels, step_q16):
    """Rules 1 and 2 of the scale pyramid (pgx.h; host only) -> (dims int32 [n_levels][2] = (W_l, H_l), (0, 0) for an empty
    level; scale int32 [n_levels] = S_l)."""
    n = int(n_levels)
    dims, scale = np.zeros((max(n, 1), 2), dtype=np.int32), np.zeros(max(n, 1), dtype=np.int32)
    rc = _lib.lib().pgx_pyramid_dims(int(W), int(H), n, int(step_q16), _ptr(dims), _ptr(scale))
    if rc != PGX_OK:
        raise _EXC.get(rc, PgxError)(rc, "pgx_pyramid_dims(%d, %d, %d, %d)" % (W, H, n, step_q16))
    return dims, scale


def build_dewarp_map(W, H, coeffs):
    """DeWarp.GetDistortionMatrix (DeWarp.cs:39-107) -> int32 [H][W][2]."""
    k = np.ascontiguousarray(coeffs, dtype=np.float64)
    out = np.zeros((H, W, 2), dtype=np.int32)
    rc = _lib.lib().pgx_build_dewarp_map(int(W), int(H), _ptr(k), len(k), _ptr(out))
    if rc != PGX_OK:
        raise ArgumentException(rc, "You must pass exactly 5 distortion coefficients")
    return out


# ---- the reference's classes --------------------------------------------------------------------

class DeWarp:
    """ImageProcessing/DeWarp.cs.  Options: MatrixDimensions (W, H), DistortionCoefficients[5]."""

    def __init__(self, engine, width, height, distortion_coefficients):
        self._e = engine
        self.width, self.height = int(width), int(height)
        self.coeffs = list(distortion_coefficients)

    def GetDistortionMatrix(self):
        return build_dewarp_map(self.width, self.height, self.coeffs)

    def ApplyDistortionMat(self, image_rgba64, distortion_matrix):
        """DeWarp.cs:19-37.  ArgumentException on size mismatch, IndexOutOfRangeException on an
        out-of-image source coordinate."""
        self._e.set_dewarp_map(distortion_matrix)
        return self._e.dewarp(image_rgba64)


class Grayscale:
    """Images.Abstractions/Pixels/Grayscale.cs:19-23 applied through Matrix.Convert."""

    def __init__(self, engine):
        self._e = engine

    def FromRgba64(self, image_rgba64):
        return self._e.gray(image_rgba64)


class KeypointDetection:
    """ImageProcessing/KeypointDetection.cs.  Options: Threshold, (GaussianStandardDeviation,
    NumGaussianPairs -> here the explicit pair table)."""

    def __init__(self, engine, threshold, gaussian_pairs, suppression_radius=0):
        self._e = engine
        engine.set_detect_params(threshold, suppression_radius)
        engine.set_brief_pairs(gaussian_pairs)

    def Detect(self, gray):
        """KeypointDetection.cs:42-63 -> (keypoints, descriptors) in raster order."""
        kps = self._e.fast(gray)
        return kps, self._e.brief(gray, kps)


class RedundantKeypointEliminator:
    """ImageProcessing/RedundantKeypointEliminator.cs.  Option: SuppressionRadius."""

    def __init__(self, engine, suppression_radius, threshold=0.0):
        self._e = engine
        self._r = int(suppression_radius)
        self._t = threshold

    def EliminateRedundantKeypoints(self, keypoints, width, height):
        """Returns the indices of the accepted keypoints in acceptance order (:16-35)."""
        self._e.set_detect_params(self._t, self._r)
        return self._e.nms(keypoints, width, height)


class KeypointMatching:
    """ImageProcessing/KeypointMatching.cs."""

    def __init__(self, engine):
        self._e = engine

    def MatchKeypoints(self, descriptors1, descriptors2):
        """KeypointMatching.cs:14-69 -> PAIR_DTYPE[n1] (indices + Hamming distance)."""
        return self._e.match(descriptors1, descriptors2)
