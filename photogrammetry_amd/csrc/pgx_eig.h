// pgx_eig.h -- the float64 symmetric eigen-solver that k_pose.hip and k_verify.hip share: cyclic Jacobi with every index a
// compile-time constant, and the eigenvector of the smallest eigenvalue under the sign rule "largest component positive".
// Internal to libpgx.so.
#pragma once

#ifdef __HIPCC__

// cyclic Jacobi on a symmetric N x N matrix (float64); on return A holds the eigenvalues on its diagonal and the
// columns of V the eigenvectors
template <int N>
__device__ void jacobi_eig(double (&A)[N][N], double (&V)[N][N])
{
#pragma unroll
    for (int i = 0; i < N; i++)
#pragma unroll
        for (int j = 0; j < N; j++) V[i][j] = i == j ? 1.0 : 0.0;
    for (int sweep = 0; sweep < 40; sweep++) {
        double off = 0.0, diag = 0.0;
#pragma unroll
        for (int i = 0; i < N; i++) {
            diag += A[i][i] * A[i][i];
#pragma unroll
            for (int j = i + 1; j < N; j++) off += A[i][j] * A[i][j];
        }
        if (off <= 1e-30 * (diag + 1e-300)) break;
        // p, q and k unrolled: every index is a compile-time constant, so local arrays A and V live in registers (2 x 81
        // doubles for N = 9; with run-time indices they sat in scratch and the solver was bound by scratch latency), and
        // a V the caller keeps in LDS is read and written at fixed offsets
#pragma unroll
        for (int p = 0; p < N - 1; p++)
#pragma unroll
            for (int q = p + 1; q < N; q++) {
                const double apq = A[p][q];
                if (fabs(apq) < 1e-300) continue;
                const double theta = (A[q][q] - A[p][p]) / (2.0 * apq);
                const double t = (theta >= 0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
                const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
#pragma unroll
                for (int k = 0; k < N; k++) {
                    const double akp = A[k][p], akq = A[k][q];
                    A[k][p] = c * akp - s * akq;
                    A[k][q] = s * akp + c * akq;
                }
#pragma unroll
                for (int k = 0; k < N; k++) {
                    const double apk = A[p][k], aqk = A[q][k];
                    A[p][k] = c * apk - s * aqk;
                    A[q][k] = s * apk + c * aqk;
                }
#pragma unroll
                for (int k = 0; k < N; k++) {
                    const double vkp = V[k][p], vkq = V[k][q];
                    V[k][p] = c * vkp - s * vkq;
                    V[k][q] = s * vkp + c * vkq;
                }
            }
    }
}

// eigenvector of the smallest eigenvalue of the symmetric matrix A (destroyed), sign: largest component positive; V is the
// caller's room for the eigenvectors (k_verify.hip keeps it in LDS)
template <int N>
__device__ void smallest_eigvec_in(double (&A)[N][N], double (&V)[N][N], double (&v)[N])
{
    jacobi_eig<N>(A, V);
    // selections instead of run-time indices (no array is forced into scratch): first smallest diagonal entry, its column
    double lmin = A[0][0];
#pragma unroll
    for (int i = 0; i < N; i++) v[i] = V[i][0];
#pragma unroll
    for (int j = 1; j < N; j++) {
        const bool take = A[j][j] < lmin;
        lmin = take ? A[j][j] : lmin;
#pragma unroll
        for (int i = 0; i < N; i++) v[i] = take ? V[i][j] : v[i];
    }
    double vbig = v[0];
#pragma unroll
    for (int i = 1; i < N; i++) vbig = fabs(v[i]) > fabs(vbig) ? v[i] : vbig;
    if (vbig < 0) {
#pragma unroll
        for (int i = 0; i < N; i++) v[i] = -v[i];
    }
}

// the same with V a local array: registers (k_pose.hip's form, the same operations as before the split)
template <int N>
__device__ void smallest_eigvec(double (&A)[N][N], double (&v)[N])
{
    double V[N][N];
    smallest_eigvec_in<N>(A, V, v);
}

#endif // __HIPCC__
