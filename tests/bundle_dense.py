"""The dense side of the bundle-adjustment yardstick (tests/bundle_ref.py): the full Jacobian of every used observation over
all free-camera and point parameters, and the full damped normal equations solved without a Schur complement.  A plain helper
module of tests/test_bundle_ref.py and tests/bundle_paths_cases.py: no test module imports another."""
import numpy as np

import bundle_ref as ref


def dense_jacobian(pb, lin):
    """Full J [2m][6 n_free + 3 n_points] from the yardstick's per-observation blocks"""
    m, nfr, npt = len(pb.ob_t), pb.n_free, len(pb.tracks)
    J = np.zeros((2 * m, 6 * nfr + 3 * npt))
    for i in range(m):
        c = pb.ob_cf[i]
        if c >= 0:
            J[2 * i:2 * i + 2, 6 * c:6 * c + 6] = lin["Jc"][i]
        J[2 * i:2 * i + 2, 6 * nfr + 3 * pb.ob_t[i]:6 * nfr + 3 * pb.ob_t[i] + 3] = lin["Jp"][i]
    return J


def dense_solver(pb, lin, lam):
    """(A + lam D) delta = -g on the full system, A = J^T W J, g = J^T W r"""
    J = dense_jacobian(pb, lin)
    w = np.repeat(lin["w"], 2)
    A = J.T @ (w[:, None] * J)
    g = J.T @ (w * lin["r"].reshape(-1))
    Ad = A + lam * np.diag(np.clip(np.diag(A), 1e-6, 1e32))
    if not np.isfinite(Ad).all():           # as the yardstick: a NaN block is not positive definite
        raise ref.NotPD()
    try:
        L = np.linalg.cholesky(Ad)
    except np.linalg.LinAlgError:
        raise ref.NotPD()
    d = np.linalg.solve(L.T, np.linalg.solve(L, -g))
    nfr = 6 * pb.n_free
    return d[:nfr], d[nfr:].reshape(-1, 3)
