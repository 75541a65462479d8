"""numpy yardstick of epipolar-guided matching (include/pgx.h, "epipolar-guided exact matching"), shared by
tests/test_gpu_guided.py and tests/test_guided_codegen.py.

The admissibility predicate is evaluated exactly as the header writes it: float64 values, one IEEE operation per step in the
written order (numpy never fuses a multiply and an add).  Top-2 and column nearest are a brute force over the masked distance
matrix, so the results can be compared with ==.
"""
import numpy as np

NONE = 2**31 - 1
LIM = 1 << 20
POP8 = np.array([bin(x).count("1") for x in range(256)], dtype=np.uint16)


def dist_matrix(a, b):
    a8 = np.ascontiguousarray(a).view(np.uint8)
    b8 = np.ascontiguousarray(b).view(np.uint8)
    return POP8[a8[:, None, :] ^ b8[None, :, :]].sum(-1, dtype=np.int32)


def admissible(kpa, kpb, F, band):
    """[n1][n2] bool: the header's predicate.  kpa, kpb: int [n][2] (x, y); F: 9 float32 values, row-major."""
    f = np.asarray(F, dtype=np.float32).reshape(9).astype(np.float64)
    n1, n2 = len(kpa), len(kpb)
    if not np.isfinite(f).all() or n1 == 0 or n2 == 0:
        return np.zeros((n1, n2), dtype=bool)
    x, y = kpa[:, 0].astype(np.float64), kpa[:, 1].astype(np.float64)
    u, v = kpb[:, 0].astype(np.float64)[None, :], kpb[:, 1].astype(np.float64)[None, :]
    l0 = (f[0] * x + f[3] * y) + f[6]
    l1 = (f[1] * x + f[4] * y) + f[7]
    l2 = (f[2] * x + f[5] * y) + f[8]
    n2v = l0 * l0 + l1 * l1
    e = (l0[:, None] * u + l1[:, None] * v) + l2[:, None]
    T = np.float64(np.float32(band)) * np.float64(np.float32(band))
    return (n2v > 0)[:, None] & (e * e <= T * n2v[:, None])


def in_range(kp):
    return bool(((kp >= -LIM) & (kp < LIM)).all())


def ref_guided(da, db, kpa, kpb, F, band, block=256):
    """-> idx [n1][2], dist [n1][2] (ascending (d, j) over admissible columns; missing = (-1, NONE)), col [n2]."""
    n1, n2 = len(da), len(db)
    idx = np.full((n1, 2), -1, dtype=np.int32)
    dist = np.full((n1, 2), NONE, dtype=np.int32)
    col = np.full(n2, -1, dtype=np.int32)
    if n1 == 0 or n2 == 0 or not (in_range(kpa) and in_range(kpb)):
        return idx, dist, col
    cbest = np.full(n2, NONE, dtype=np.int64)
    for i0 in range(0, n1, block):
        i1 = min(n1, i0 + block)
        adm = admissible(kpa[i0:i1], kpb, F, band)
        d = np.where(adm, dist_matrix(da[i0:i1], db).astype(np.int64), np.int64(NONE))
        j = np.broadcast_to(np.arange(n2), d.shape)
        order = np.lexsort((j, d), axis=-1)[:, :2]
        kk = order.shape[1]
        dd = np.take_along_axis(d, order, axis=1)
        ok = dd < NONE
        idx[i0:i1, :kk] = np.where(ok, order, -1)
        dist[i0:i1, :kk] = np.where(ok, dd, NONE)
        mn, am = d.min(0), d.argmin(0)   # argmin: the first (smallest) row of a tie
        better = mn < cbest              # strict: an earlier block keeps a tie
        cbest[better] = mn[better]
        col[better] = am[better] + i0
    return idx, dist, col


def ref_select(idx, dist, col, max_dist, ratio, cross):
    """pgx_match_nn_batch_dev's selection on top-2 and column-nearest results."""
    n1 = len(idx)
    i = np.arange(n1)
    j1, d1, j2, d2 = idx[:, 0], dist[:, 0].astype(np.int64), idx[:, 1], dist[:, 1].astype(np.int64)
    ok = (j1 >= 0) & (d1 <= max_dist)
    if ratio > 0:
        ok &= (j2 < 0) | (d1.astype(np.float64) < np.float64(np.float32(ratio)) * d2.astype(np.float64))
    if cross and len(col):
        ok &= col[np.where(j1 >= 0, j1, 0)] == i
    out = np.zeros((n1, 3), dtype=np.int32)
    out[:, 0] = i
    out[:, 1] = np.where(ok, j1, -1)
    out[:, 2] = np.where(ok, dist[:, 0], NONE)
    return out


def loop_guided(da, db, kpa, kpb, F, band):
    """Literal Python loops over floats (IEEE doubles), tiny inputs only: (rows [(d, j), ...] <= 2, cols [i or -1])."""
    f = [float(np.float32(v)) for v in np.asarray(F, dtype=np.float32).reshape(9)]
    finite = all(np.isfinite(f))
    T = float(np.float32(band)) * float(np.float32(band))
    ints = lambda d: [int("".join("%08x" % w for w in row[::-1]), 16) for row in d]   # noqa: E731
    A, B = ints(da), ints(db)

    def adm(i, j):
        x, y = float(kpa[i][0]), float(kpa[i][1])
        u, v = float(kpb[j][0]), float(kpb[j][1])
        l0 = (f[0] * x + f[3] * y) + f[6]
        l1 = (f[1] * x + f[4] * y) + f[7]
        l2 = (f[2] * x + f[5] * y) + f[8]
        n2 = l0 * l0 + l1 * l1
        e = (l0 * u + l1 * v) + l2
        return finite and n2 > 0 and e * e <= T * n2

    rows = []
    for i, a in enumerate(A):
        rows.append(sorted((bin(a ^ b).count("1"), j) for j, b in enumerate(B) if adm(i, j))[:2])
    cols = [min(((bin(a ^ b).count("1"), i) for i, a in enumerate(A) if adm(i, j)), default=(NONE, -1))[1]
            for j, b in enumerate(B)]
    return rows, cols
