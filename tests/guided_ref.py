"""numpy yardstick of epipolar-guided matching (include/pgx.h, "epipolar-guided exact matching"), shared by
tests/test_gpu_guided.py and tests/test_guided_codegen.py.

The admissibility predicate is evaluated exactly as the header writes it: float64 values, one IEEE operation per step in the
written order (numpy never fuses a multiply and an add).  Top-2 and column nearest are a brute force over the masked distance
matrix, so the results can be compared with ==.
"""
import numpy as np

from knn_ref import loop_knn, top2_and_col

LIM = 1 << 20


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
    ok = in_range(kpa) and in_range(kpb)     # one coordinate out of range rejects every pair
    return top2_and_col(da, db, block, lambda i0, i1: ok & admissible(kpa[i0:i1], kpb, F, band))


def loop_guided(da, db, kpa, kpb, F, band):
    """Literal Python loops over floats (IEEE doubles), tiny inputs only: (rows [(d, j), ...] <= 2, cols [i or -1])."""
    f = [float(np.float32(v)) for v in np.asarray(F, dtype=np.float32).reshape(9)]
    finite = all(np.isfinite(f))
    T = float(np.float32(band)) * float(np.float32(band))

    def adm(i, j):
        x, y = float(kpa[i][0]), float(kpa[i][1])
        u, v = float(kpb[j][0]), float(kpb[j][1])
        l0 = (f[0] * x + f[3] * y) + f[6]
        l1 = (f[1] * x + f[4] * y) + f[7]
        l2 = (f[2] * x + f[5] * y) + f[8]
        n2 = l0 * l0 + l1 * l1
        e = (l0 * u + l1 * v) + l2
        return finite and n2 > 0 and e * e <= T * n2

    return loop_knn(da, db, adm)
