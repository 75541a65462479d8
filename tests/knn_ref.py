"""numpy yardstick of the exact nearest-neighbour modes (include/pgx.h), shared by tests/test_gpu_knn.py and, through
tests/guided_ref.py, by the guided tests: a popcount table over uint8 views, a blocked brute force for the two nearest columns
of every row and the nearest row of every column, pgx_match_nn_batch_dev's selection on top of them, and a literal Python
loop over bin(x ^ y).count("1") -- the hamming_distance of the reference's Python prototype
(python_src/photogrammetry/image_processing/keypoint_matching.py) -- for tiny inputs.

Every value is an exact integer, so results compare with ==.  The order is (d, index) everywhere: rows by lexsort((j, d)),
columns by the first occurrence of the minimum within a block and a strict < across blocks.
"""
import numpy as np

NONE = 2**31 - 1
POP8 = np.array([bin(x).count("1") for x in range(256)], dtype=np.uint16)


def rand_desc(rng, n, words):
    return rng.integers(0, 2**32, size=(n, words), dtype=np.uint32)


def dist_matrix(a, b, i0=0, i1=None):
    """[i1 - i0][n2] hamming distances of rows i0..i1 of a against b (uint32 [n][words])."""
    a8 = np.ascontiguousarray(a[i0:i1]).view(np.uint8)
    b8 = np.ascontiguousarray(b).view(np.uint8)
    return POP8[a8[:, None, :] ^ b8[None, :, :]].sum(-1, dtype=np.int32)


def top2_and_col(a, b, block, admissible=None):
    """The brute force.  admissible(i0, i1) -> bool [i1 - i0][n2] masks the pairs of a row block (None: every pair counts).
    -> idx [n1][2], dist [n1][2] (ascending (d, j), missing = (-1, NONE)), col [n2] (smallest (d, i), -1 without rows)."""
    n1, n2 = len(a), len(b)
    idx = np.full((n1, 2), -1, dtype=np.int32)
    dist = np.full((n1, 2), NONE, dtype=np.int32)
    cbest = np.full(n2, NONE, dtype=np.int64)
    col = np.full(n2, -1, dtype=np.int32)
    if n2 == 0:
        return idx, dist, col
    for i0 in range(0, n1, block):
        i1 = min(n1, i0 + block)
        d = dist_matrix(a, b, i0, i1).astype(np.int64)
        if admissible is not None:
            d = np.where(admissible(i0, i1), d, np.int64(NONE))
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


def ref_knn(a, b, block=128):
    return top2_and_col(a, b, block)


def ref_select(idx, dist, col, max_dist, ratio, cross):
    """pgx_match_nn_batch_dev's selection on top-2 and column-nearest results."""
    n1 = len(idx)
    i = np.arange(n1)
    j1, d1, j2, d2 = idx[:, 0], dist[:, 0].astype(np.int64), idx[:, 1], dist[:, 1].astype(np.int64)
    ok = (j1 >= 0) & (d1 <= max_dist)
    if ratio > 0:
        ok &= (j2 < 0) | (d1.astype(np.float64) < np.float64(np.float32(ratio)) * d2.astype(np.float64))
    if cross and len(col):   # no column: no row was accepted anyway
        ok &= col[np.where(j1 >= 0, j1, 0)] == i
    out = np.zeros((n1, 3), dtype=np.int32)
    out[:, 0] = i
    out[:, 1] = np.where(ok, j1, -1)
    out[:, 2] = np.where(ok, dist[:, 0], NONE)
    return out


def ints(d):
    """Descriptors as Python integers, word 0 lowest."""
    return [int("".join("%08x" % w for w in row[::-1]), 16) for row in d]


def loop_knn(a, b, adm=lambda i, j: True):
    """Literal loops over the pairs adm(i, j) admits, tiny inputs only: (rows [(d, j), ...] <= 2, cols [i or -1])."""
    A, B = ints(a), ints(b)
    rows = [sorted((bin(x ^ y).count("1"), j) for j, y in enumerate(B) if adm(i, j))[:2] for i, x in enumerate(A)]
    cols = [min(((bin(x ^ y).count("1"), i) for i, x in enumerate(A) if adm(i, j)), default=(NONE, -1))[1]
            for j, y in enumerate(B)]
    return rows, cols
