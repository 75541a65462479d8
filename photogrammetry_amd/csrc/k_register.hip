// k_register.hip -- frame registration by P3P RANSAC against triangulated track points (pgx_register_frames_dev;
// include/pgx.h).
//
// A target frame's correspondences are the nodes it has in tracks whose 3D point is known; the frame's pose is the P3P
// hypothesis with the most inliers, refined by Gauss-Newton.  float64 throughout, in the world shifted to the mean of the
// frame's correspondence points (a rotation about a far-away origin couples omega and tau).
//
// Kernels (all on the caller's stream; n_tracks is read on the device):
//   k_reg_frames   one workgroup: K validation, the slot -> frame inverse, targets numbered in frame order, the rows of
//                  every frame that is not registered here (copied Rt, its P, stats and errors)
//   k_reg_count    per track (G lanes): which nodes are correspondences of a target (a per-node mark), per-target counts
//                  by integer atomics (the counts do not depend on the order)
//   k_reg_csr      one workgroup per target: its correspondences in track order (a block scan over the tracks), the shift
//                  S from a fixed-shape sum, and the SoA arrays X' = X - S, cu = cx - u, cv = cy - v
//   k_reg_hyp      one thread per (target, sample) of a chunk of samples: the sample, P3P, the solutions ranked by |t_S|,
//                  four hypothesis slots (R, t_S; NaN = no hypothesis)
//   k_reg_score    the hot path: one thread per hypothesis, a workgroup covers 256 hypotheses of one target and walks the
//                  target's correspondences through LDS (every lane reads the same address: a broadcast).  The predicate
//                  has no division and no square root; the counts are integers in registers; the workgroup's best key
//                  (pgx_ransac.h: inliers, then the smallest h) goes to its own slot, no atomics
//   k_reg_pick     one workgroup per target: the winner (a max over the per-workgroup keys) and its hypothesis again (the
//                  same device code as k_reg_hyp, so the same bits)
//   k_reg_refine   one workgroup per target: Gauss-Newton on the winner's inliers (6x6 normal equations summed per lane,
//                  xor butterflies per wave, four waves in a fixed order), the final classification, the outputs
//   k_reg_summary  one workgroup: the report, integer sums over the frames
// Samples run in chunks so that the hypothesis buffer stays bounded; the chunk size changes no result.
// DESIGN.md section 17 has the measurements.
#include "pgx_stage_args.h"

namespace {

constexpr int REG_NT = 256;         // threads per workgroup of every kernel here
static_assert(REG_NT == 256, "block_sums (pgx_trackgraph.h) adds up four waves");
constexpr int REG_G = 16;           // lanes per track in k_reg_count
constexpr int REG_GRID_MAX = 1024;  // workgroups of k_reg_count, at most
constexpr int REG_HD = 12;          // doubles per hypothesis: R row-major, t_S
constexpr long long REG_CHUNK_CELLS = 1 << 17;  // (target slots x samples) per chunk, at most (25 MB of hypotheses)

__device__ __forceinline__ bool good_k(const double *K)
{
    return isfinite(K[0]) && isfinite(K[1]) && isfinite(K[2]) && isfinite(K[3]) && K[0] != 0.0 && K[1] != 0.0;
}

// ---- P3P (Lambda Twist, Persson and Nordberg, ECCV 2018) -----------------------------------------------------------

__device__ __forceinline__ double det3c(double a0, double a1, double a2, double b0, double b1, double b2, double c0, double c1,
                                        double c2)
{
    // det of the matrix with columns a, b, c
    return (a0 * (b1 * c2 - b2 * c1) - b0 * (a1 * c2 - a2 * c1)) + c0 * (a1 * b2 - a2 * b1);
}

// a real root of x^3 + b x^2 + c x + d by Newton from the side where the iteration is monotone
__device__ __forceinline__ double cubic_root(double b, double c, double d)
{
    const double disc = b * b - 3.0 * c;
    double m = -b / 3.0;
    if (disc >= 0.0) m = (-b + sqrt(disc)) / 3.0;   // the local minimum
    const double fm = ((m + b) * m + c) * m + d;
    const double bound = 1.0 + fmax(fabs(b), fmax(fabs(c), fabs(d)));
    const bool right = fm <= 0.0;
    double x = right ? bound : -bound;
    for (int it = 0; it < 200; it++) {
        const double f = ((x + b) * x + c) * x + d;
        const double fp = (3.0 * x + 2.0 * b) * x + c;
        const double xn = x - f / fp;
        if (!(right ? xn < x : xn > x)) break;
        x = xn;
    }
    return x;
}

// the eigenvector of the symmetric M for eigenvalue sig: the longest cross product of two rows of M - sig I, normalised
__device__ __forceinline__ void null_vec(const double (&M)[3][3], double sig, double (&e)[3])
{
    const double r0[3] = {M[0][0] - sig, M[0][1], M[0][2]};
    const double r1[3] = {M[1][0], M[1][1] - sig, M[1][2]};
    const double r2[3] = {M[2][0], M[2][1], M[2][2] - sig};
    const double c01[3] = {r0[1] * r1[2] - r0[2] * r1[1], r0[2] * r1[0] - r0[0] * r1[2], r0[0] * r1[1] - r0[1] * r1[0]};
    const double c02[3] = {r0[1] * r2[2] - r0[2] * r2[1], r0[2] * r2[0] - r0[0] * r2[2], r0[0] * r2[1] - r0[1] * r2[0]};
    const double c12[3] = {r1[1] * r2[2] - r1[2] * r2[1], r1[2] * r2[0] - r1[0] * r2[2], r1[0] * r2[1] - r1[1] * r2[0]};
    const double n01 = (c01[0] * c01[0] + c01[1] * c01[1]) + c01[2] * c01[2];
    const double n02 = (c02[0] * c02[0] + c02[1] * c02[1]) + c02[2] * c02[2];
    const double n12 = (c12[0] * c12[0] + c12[1] * c12[1]) + c12[2] * c12[2];
    double n = n01;
#pragma unroll
    for (int k = 0; k < 3; k++) e[k] = c01[k];
    if (n02 > n) {
        n = n02;
#pragma unroll
        for (int k = 0; k < 3; k++) e[k] = c02[k];
    }
    if (n12 > n) {
        n = n12;
#pragma unroll
        for (int k = 0; k < 3; k++) e[k] = c12[k];
    }
    const double s = sqrt(n);
#pragma unroll
    for (int k = 0; k < 3; k++) e[k] = e[k] / s;
}

// squared norm of the residual of the three distance equations
__device__ __forceinline__ double lam_res(const double (&l)[3], double a12, double a13, double a23, double b12, double b13, double b23,
                                          double (&F)[3])
{
    F[0] = ((l[0] * l[0] + l[1] * l[1]) + b12 * (l[0] * l[1])) - a12;
    F[1] = ((l[0] * l[0] + l[2] * l[2]) + b13 * (l[0] * l[2])) - a13;
    F[2] = ((l[1] * l[1] + l[2] * l[2]) + b23 * (l[1] * l[2])) - a23;
    return (F[0] * F[0] + F[1] * F[1]) + F[2] * F[2];
}

// P3P on unit bearings y[i] and points X[i]: up to four (R, t) in the fixed slots 2 * sign + root, ok[] marks them
__device__ void p3p(const double (&y)[3][3], const double (&X)[3][3], double (&R)[4][9], double (&t)[4][3], bool (&ok)[4])
{
    const double b12 = -2.0 * ((y[0][0] * y[1][0] + y[0][1] * y[1][1]) + y[0][2] * y[1][2]);
    const double b13 = -2.0 * ((y[0][0] * y[2][0] + y[0][1] * y[2][1]) + y[0][2] * y[2][2]);
    const double b23 = -2.0 * ((y[1][0] * y[2][0] + y[1][1] * y[2][1]) + y[1][2] * y[2][2]);
    double d12[3], d13[3], d23[3];
#pragma unroll
    for (int k = 0; k < 3; k++) {
        d12[k] = X[0][k] - X[1][k];
        d13[k] = X[0][k] - X[2][k];
        d23[k] = X[1][k] - X[2][k];
    }
    const double a12 = (d12[0] * d12[0] + d12[1] * d12[1]) + d12[2] * d12[2];
    const double a13 = (d13[0] * d13[0] + d13[1] * d13[1]) + d13[2] * d13[2];
    const double a23 = (d23[0] * d23[0] + d23[1] * d23[1]) + d23[2] * d23[2];
    // D1 = a23 M12 - a12 M23, D2 = a23 M13 - a13 M23 (lambda^T Mij lambda = the left side of equation ij)
    const double A[3][3] = {{a23, a23 * (0.5 * b12), 0.0},
                            {a23 * (0.5 * b12), a23 - a12, -(a12 * (0.5 * b23))},
                            {0.0, -(a12 * (0.5 * b23)), -a12}};
    const double B[3][3] = {{a23, 0.0, a23 * (0.5 * b13)},
                            {0.0, -a13, -(a13 * (0.5 * b23))},
                            {a23 * (0.5 * b13), -(a13 * (0.5 * b23)), a23 - a13}};
    // det(A + g B) = p3 g^3 + p2 g^2 + p1 g + p0, by columns
    const double p0 = det3c(A[0][0], A[1][0], A[2][0], A[0][1], A[1][1], A[2][1], A[0][2], A[1][2], A[2][2]);
    const double p3 = det3c(B[0][0], B[1][0], B[2][0], B[0][1], B[1][1], B[2][1], B[0][2], B[1][2], B[2][2]);
    const double p1 = (det3c(B[0][0], B[1][0], B[2][0], A[0][1], A[1][1], A[2][1], A[0][2], A[1][2], A[2][2]) +
                       det3c(A[0][0], A[1][0], A[2][0], B[0][1], B[1][1], B[2][1], A[0][2], A[1][2], A[2][2])) +
                      det3c(A[0][0], A[1][0], A[2][0], A[0][1], A[1][1], A[2][1], B[0][2], B[1][2], B[2][2]);
    const double p2 = (det3c(A[0][0], A[1][0], A[2][0], B[0][1], B[1][1], B[2][1], B[0][2], B[1][2], B[2][2]) +
                       det3c(B[0][0], B[1][0], B[2][0], A[0][1], A[1][1], A[2][1], B[0][2], B[1][2], B[2][2])) +
                      det3c(B[0][0], B[1][0], B[2][0], B[0][1], B[1][1], B[2][1], A[0][2], A[1][2], A[2][2]);
    double g;
    if (fabs(p3) >= fabs(p0))
        g = cubic_root(p2 / p3, p1 / p3, p0 / p3);
    else
        g = 1.0 / cubic_root(p1 / p0, p2 / p0, p3 / p0);
    double D[3][3];
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
        for (int j = 0; j < 3; j++) D[i][j] = A[i][j] + g * B[i][j];
    // D has rank 2: eigenvalues sig1, sig2 (|sig1| >= |sig2|) and 0
    const double tr = (D[0][0] + D[1][1]) + D[2][2];
    const double mn = ((D[0][0] * D[1][1] - D[0][1] * D[1][0]) + (D[0][0] * D[2][2] - D[0][2] * D[2][0])) +
                      (D[1][1] * D[2][2] - D[1][2] * D[2][1]);
    const double h = 0.5 * tr;
    const double q = sqrt(fmax(h * h - mn, 0.0));
    const double sa = h + q, sb = h - q;
    const double sig1 = fabs(sa) >= fabs(sb) ? sa : sb, sig2 = fabs(sa) >= fabs(sb) ? sb : sa;
    double e0[3], e2[3], e1[3];
    null_vec(D, 0.0, e2);
    null_vec(D, sig1, e0);
    e1[0] = e2[1] * e0[2] - e2[2] * e0[1];
    e1[1] = e2[2] * e0[0] - e2[0] * e0[2];
    e1[2] = e2[0] * e0[1] - e2[1] * e0[0];
    const double n1 = sqrt((e1[0] * e1[0] + e1[1] * e1[1]) + e1[2] * e1[2]);
#pragma unroll
    for (int k = 0; k < 3; k++) e1[k] = e1[k] / n1;
    const double s = sqrt(-sig2 / sig1);   // NaN when sig1 sig2 > 0: no real factorisation, no solution
    // X^-1 for the pose: columns d12, d13, d12 x d13
    const double dc[3] = {d12[1] * d13[2] - d12[2] * d13[1], d12[2] * d13[0] - d12[0] * d13[2], d12[0] * d13[1] - d12[1] * d13[0]};
    const double dX = det3c(d12[0], d12[1], d12[2], d13[0], d13[1], d13[2], dc[0], dc[1], dc[2]);
    // rows of adj(Xm): Xm^-1 = adj / det, Xm = [d12 d13 dc] by columns
    double Xi[3][3];
    Xi[0][0] = (d13[1] * dc[2] - d13[2] * dc[1]) / dX;
    Xi[0][1] = (d13[2] * dc[0] - d13[0] * dc[2]) / dX;
    Xi[0][2] = (d13[0] * dc[1] - d13[1] * dc[0]) / dX;
    Xi[1][0] = (dc[1] * d12[2] - dc[2] * d12[1]) / dX;
    Xi[1][1] = (dc[2] * d12[0] - dc[0] * d12[2]) / dX;
    Xi[1][2] = (dc[0] * d12[1] - dc[1] * d12[0]) / dX;
    Xi[2][0] = (d12[1] * d13[2] - d12[2] * d13[1]) / dX;
    Xi[2][1] = (d12[2] * d13[0] - d12[0] * d13[2]) / dX;
    Xi[2][2] = (d12[0] * d13[1] - d12[1] * d13[0]) / dX;
#pragma unroll
    for (int sg = 0; sg < 2; sg++) {
        const double ss = sg == 0 ? s : -s;
        const double nv[3] = {e0[0] - ss * e1[0], e0[1] - ss * e1[1], e0[2] - ss * e1[2]};
        const double w0 = -nv[1] / nv[0], w1 = -nv[2] / nv[0];
        const double dd = a13 - a12;
        const double qa = ((dd * (w1 * w1) - a12) - (a12 * b13) * w1);
        const double qb = ((2.0 * dd) * (w0 * w1) + (a13 * b12) * w1) - (a12 * b13) * w0;
        const double qc = (dd * (w0 * w0) + a13) + (a13 * b12) * w0;
        const double disc = qb * qb - 4.0 * (qa * qc);
        const double sq = sqrt(disc);
        const double qq = -0.5 * (qb + (qb >= 0.0 ? sq : -sq));
        const double taus[2] = {qq / qa, qc / qq};
#pragma unroll
        for (int r = 0; r < 2; r++) {
            const int slot = 2 * sg + r;
            const double tau = taus[r];
            const double den = (tau * tau + b23 * tau) + 1.0;
            double l[3];
            l[1] = sqrt(a23 / den);
            l[2] = tau * l[1];
            l[0] = (w0 + w1 * tau) * l[1];
            // Newton on the three equations (a step is kept only if the residual falls)
            double Fr[3];
            double res = lam_res(l, a12, a13, a23, b12, b13, b23, Fr);
#pragma unroll
            for (int it = 0; it < 3; it++) {
                const double J00 = 2.0 * l[0] + b12 * l[1], J01 = 2.0 * l[1] + b12 * l[0];
                const double J10 = 2.0 * l[0] + b13 * l[2], J12 = 2.0 * l[2] + b13 * l[0];
                const double J21 = 2.0 * l[1] + b23 * l[2], J22 = 2.0 * l[2] + b23 * l[1];
                // J = [[J00, J01, 0], [J10, 0, J12], [0, J21, J22]]; delta = J^-1 F by Cramer
                const double dj = (J00 * (0.0 - J12 * J21) - J01 * (J10 * J22)) + 0.0;
                const double x0 = (Fr[0] * (0.0 - J12 * J21) - J01 * (Fr[1] * J22 - J12 * Fr[2])) / dj;
                const double x1 = (J00 * (Fr[1] * J22 - J12 * Fr[2]) - Fr[0] * (J10 * J22)) / dj;
                const double x2 = (J00 * (0.0 * Fr[2] - Fr[1] * J21) - J01 * (J10 * Fr[2]) + Fr[0] * (J10 * J21)) / dj;
                const double ln[3] = {l[0] - x0, l[1] - x1, l[2] - x2};
                double Fn[3];
                const double rn = lam_res(ln, a12, a13, a23, b12, b13, b23, Fn);
                if (!(rn < res)) break;
                res = rn;
#pragma unroll
                for (int k = 0; k < 3; k++) {
                    l[k] = ln[k];
                    Fr[k] = Fn[k];
                }
            }
            bool v = tau > 0.0 && den > 0.0 && l[0] > 0.0 && l[1] > 0.0 && l[2] > 0.0;
            // Y_i = l_i y_i; R = [Y1 - Y2, Y1 - Y3, (Y1 - Y2) x (Y1 - Y3)] Xm^-1, t = Y1 - R X1
            double Y[3][3];
#pragma unroll
            for (int i = 0; i < 3; i++)
#pragma unroll
                for (int k = 0; k < 3; k++) Y[i][k] = l[i] * y[i][k];
            const double y12[3] = {Y[0][0] - Y[1][0], Y[0][1] - Y[1][1], Y[0][2] - Y[1][2]};
            const double y13[3] = {Y[0][0] - Y[2][0], Y[0][1] - Y[2][1], Y[0][2] - Y[2][2]};
            const double yc[3] = {y12[1] * y13[2] - y12[2] * y13[1], y12[2] * y13[0] - y12[0] * y13[2], y12[0] * y13[1] - y12[1] * y13[0]};
#pragma unroll
            for (int i = 0; i < 3; i++)
#pragma unroll
                for (int j = 0; j < 3; j++) R[slot][3 * i + j] = (y12[i] * Xi[0][j] + y13[i] * Xi[1][j]) + yc[i] * Xi[2][j];
#pragma unroll
            for (int i = 0; i < 3; i++)
                t[slot][i] = Y[0][i] - ((R[slot][3 * i] * X[0][0] + R[slot][3 * i + 1] * X[0][1]) + R[slot][3 * i + 2] * X[0][2]);
#pragma unroll
            for (int k = 0; k < 9; k++) v = v && isfinite(R[slot][k]);
#pragma unroll
            for (int k = 0; k < 3; k++) v = v && isfinite(t[slot][k]);
            ok[slot] = v;
        }
    }
}

// hypothesis h = 4 s + rank of a target: the sample's three positions, P3P, the solution of the given rank by ascending
// |t_S|^2 (ties: slot order).  false: no hypothesis of that rank.
__device__ bool hypothesis(const RegArgs &a, int frame, int base, int n, double fx, double fy, int s, int rank, double (&Ro)[9],
                           double (&to)[3])
{
    uint64_t st = ransac_stream(a.seed, frame, s);
    int id[3];
    ransac_draw(st, n, 3, id);
    double y[3][3], X[3][3];
#pragma unroll
    for (int k = 0; k < 3; k++) {
        const long long p = (long long)base + id[k];
        const double bx = (-a.cu[p]) / fx, by = (-a.cv[p]) / fy;
        const double nr = sqrt((bx * bx + by * by) + 1.0);
        y[k][0] = bx / nr;
        y[k][1] = by / nr;
        y[k][2] = 1.0 / nr;
        X[k][0] = a.cx[p];
        X[k][1] = a.cy[p];
        X[k][2] = a.cz[p];
    }
    double R[4][9], t[4][3];
    bool ok[4];
    p3p(y, X, R, t, ok);
    double key[4];
#pragma unroll
    for (int i = 0; i < 4; i++) {
        const double k2 = (t[i][0] * t[i][0] + t[i][1] * t[i][1]) + t[i][2] * t[i][2];
        key[i] = ok[i] && isfinite(k2) ? k2 : __builtin_inf();
        ok[i] = ok[i] && isfinite(k2);
    }
    bool found = false;
#pragma unroll
    for (int i = 0; i < 4; i++) {
        int rk = 0;
#pragma unroll
        for (int j = 0; j < 4; j++) rk += (key[j] < key[i]) || (key[j] == key[i] && j < i);
        if (ok[i] && rk == rank) {
            found = true;
#pragma unroll
            for (int k = 0; k < 9; k++) Ro[k] = R[i][k];
#pragma unroll
            for (int k = 0; k < 3; k++) to[k] = t[i][k];
        }
    }
    return found;
}

// the inlier predicate (include/pgx.h): no division, no square root
__device__ __forceinline__ bool inlier(const double (&R)[9], const double (&t)[3], double fx, double fy, double ip, double X0, double X1,
                                       double X2, double cu, double cv)
{
    const double x = ((R[0] * X0 + R[1] * X1) + R[2] * X2) + t[0];
    const double y = ((R[3] * X0 + R[4] * X1) + R[5] * X2) + t[1];
    const double z = ((R[6] * X0 + R[7] * X1) + R[8] * X2) + t[2];
    const double pa = fx * x + cu * z, pb = fy * y + cv * z;
    const double e = ip * z;
    return z > 0.0 && pa * pa + pb * pb <= e * e;
}

// ---- kernels -------------------------------------------------------------------------------------------------------

__global__ __launch_bounds__(REG_NT) void k_reg_frames(RegArgs a)
{
    const double NaN = __builtin_nan("");
    for (int f = threadIdx.x; f < a.tv.n_frames; f += blockDim.x) {
        a.tv.inv[f] = -1;
        a.cnt[f] = 0;
        const double *K = a.K + (size_t)f * 4;
        const bool target = a.reg[f] != 0, kok = good_k(K);
        if (target) continue;   // numbered below, written by k_reg_refine (or below when K is bad)
        const double *R = a.Rt_in + (size_t)f * 12;
        double *o = a.Rt_out + (size_t)f * 12, *P = a.P_out + (size_t)f * 12;
        double r[12];
        bool known = kok;
        for (int k = 0; k < 12; k++) {
            r[k] = R[k];
            known = known && isfinite(r[k]);
        }
        for (int k = 0; k < 12; k++) o[k] = r[k];
        camera_matrix(K, r, known, P);
        for (int k = 0; k < 4; k++) a.frame_stats[(size_t)f * 4 + k] = -1;
        a.frame_err[2 * f] = NaN;
        a.frame_err[2 * f + 1] = NaN;
    }
    __syncthreads();
    build_slot_inverse(a.tv, a.status, PGX_ST_REG_DUP);
    if (threadIdx.x == 0) {
        int n = 0;
        for (int f = 0; f < a.tv.n_frames; f++) {
            const bool on = a.reg[f] != 0 && good_k(a.K + (size_t)f * 4);
            a.tnum[f] = on ? n : -1;
            if (on) a.tframe[n++] = f;
            if (a.reg[f] != 0 && !on) {   // BADK: failed at once
                for (int k = 0; k < 12; k++) {
                    a.Rt_out[(size_t)f * 12 + k] = NaN;
                    a.P_out[(size_t)f * 12 + k] = NaN;
                }
                a.frame_stats[(size_t)f * 4] = 0;
                a.frame_stats[(size_t)f * 4 + 1] = 0;
                a.frame_stats[(size_t)f * 4 + 2] = -1;
                a.frame_stats[(size_t)f * 4 + 3] = PGX_REG_BADK;
                a.frame_err[2 * f] = NaN;
                a.frame_err[2 * f + 1] = NaN;
            }
        }
        a.ctrl[0] = clamp_tracks(a.tv, a.status, PGX_ST_REG_CAP);
        a.ctrl[1] = n;
    }
}

__global__ __launch_bounds__(REG_NT) void k_reg_count(RegArgs a)
{
    const long long nt = a.ctrl[0];
    PGX_TRACK_LOOP(REG_G, nt)
    {
        int o0, n;
        if (!track_range(a.tv, t, o0, n) && lane == 0) atomicOr(a.status, (int)PGX_ST_REG_NODE);
        const bool pt = (!a.track_flags || a.track_flags[t] == 0) && isfinite(a.xyz[3 * t]) && isfinite(a.xyz[3 * t + 1]) &&
                        isfinite(a.xyz[3 * t + 2]);
        int bad = 0, twice = 0;
        for (int i = lane; i < n; i += REG_G) {
            const long long o = (long long)o0 + i;
            const int f = a.tv.nodes[2 * o], k = a.tv.nodes[2 * o + 1];
            int c = -1;
            if (!node_ok(a.tv, f, k)) {
                bad = 1;
            } else if (a.tnum[f] >= 0) {
                bool dup = false;
                for (int j = 0; j < n; j++)
                    if (j != i && a.tv.nodes[2 * ((long long)o0 + j)] == f) dup = true;
                if (dup) twice = 1;
                if (!dup && pt) {
                    c = a.tnum[f];
                    atomicAdd(&a.cnt[c], 1);
                }
            }
            a.cf[o] = c;
            if (a.node_inlier) a.node_inlier[o] = -1;
        }
        bad = gsum_i<REG_G>(bad);
        twice = gsum_i<REG_G>(twice);
        if (lane == 0 && bad) atomicOr(a.status, (int)PGX_ST_REG_NODE);
        if (lane == 0 && twice) atomicOr(a.status, (int)PGX_ST_REG_TWICE);
    }
}

// one workgroup per target: its correspondences in track order, S, and the SoA arrays
__global__ __launch_bounds__(REG_NT) void k_reg_csr(RegArgs a)
{
    __shared__ int s_wave[REG_NT / 64];
    __shared__ int s_base, s_end;
    __shared__ double s_red[3][REG_NT];
    const int c = blockIdx.x;
    if (c >= a.ctrl[1]) return;
    const int nt = a.ctrl[0];
    const int f = a.tframe[c];
    if (threadIdx.x == 0) {
        long long st = 0;
        for (int b = 0; b < c; b++) st += a.cnt[b];
        const long long end = st + a.cnt[c];
        const bool fits = end <= a.tv.node_cap;   // overlapping node ranges (malformed offsets) can count a node twice
        if (!fits) atomicOr(a.status, (int)PGX_ST_REG_NODE);
        a.coff[c] = fits ? (int)st : 0;
        s_base = fits ? (int)st : 0;
        s_end = fits ? (int)end : 0;
    }
    __syncthreads();
    const int start = s_base, stop = s_end;
    const int wave = threadIdx.x >> 6, ln = threadIdx.x & 63;
    for (int base = 0; base < nt; base += REG_NT) {
        const int t = base + threadIdx.x;
        int node = -1;
        if (t < nt) {
            int o0, n;
            track_range(a.tv, t, o0, n);
            for (int i = 0; i < n; i++)
                if (a.cf[(long long)o0 + i] == c) node = o0 + i;
        }
        const unsigned long long m = __ballot(node >= 0);
        if (ln == 0) s_wave[wave] = __popcll(m);
        __syncthreads();
        int pos = s_base;
        for (int w = 0; w < wave; w++) pos += s_wave[w];
        pos += __popcll(m & ((1ull << ln) - 1ull));
        if (node >= 0 && pos < stop) {
            double u, v;
            node_keypoint(a.tv, f, a.tv.nodes[2 * (long long)node + 1], u, v);
            a.corr_node[pos] = node;
            a.cx[pos] = a.xyz[3 * (long long)t];
            a.cy[pos] = a.xyz[3 * (long long)t + 1];
            a.cz[pos] = a.xyz[3 * (long long)t + 2];
            a.cu[pos] = a.K[(size_t)f * 4 + 2] - u;
            a.cv[pos] = a.K[(size_t)f * 4 + 3] - v;
        }
        __syncthreads();
        if (threadIdx.x == 0) {
            int tot = 0;
            for (int w = 0; w < REG_NT / 64; w++) tot += s_wave[w];
            s_base += tot;
        }
        __syncthreads();
    }
    const int n = (s_base < stop ? s_base : stop) - start;
    // S: per-thread sums strided by REG_NT, then a fixed tree
    double sx = 0.0, sy = 0.0, sz = 0.0;
    for (int j = threadIdx.x; j < n; j += REG_NT) {
        sx += a.cx[start + j];
        sy += a.cy[start + j];
        sz += a.cz[start + j];
    }
    s_red[0][threadIdx.x] = sx;
    s_red[1][threadIdx.x] = sy;
    s_red[2][threadIdx.x] = sz;
    __syncthreads();
    for (int m2 = REG_NT / 2; m2 > 0; m2 >>= 1) {
        if ((int)threadIdx.x < m2)
            for (int k = 0; k < 3; k++) s_red[k][threadIdx.x] = s_red[k][threadIdx.x] + s_red[k][threadIdx.x + m2];
        __syncthreads();
    }
    const double S0 = n > 0 ? s_red[0][0] / n : 0.0, S1 = n > 0 ? s_red[1][0] / n : 0.0, S2 = n > 0 ? s_red[2][0] / n : 0.0;
    for (int j = threadIdx.x; j < n; j += REG_NT) {
        a.cx[start + j] = a.cx[start + j] - S0;
        a.cy[start + j] = a.cy[start + j] - S1;
        a.cz[start + j] = a.cz[start + j] - S2;
    }
    if (threadIdx.x == 0) {
        a.nlist[c] = n;
        a.S[4 * c] = S0;
        a.S[4 * c + 1] = S1;
        a.S[4 * c + 2] = S2;
    }
}

// one thread per (target, sample) of the chunk [s0, s0 + chunk)
__global__ __launch_bounds__(REG_NT) void k_reg_hyp(RegArgs a, int s0, int chunk)
{
    const int c = blockIdx.y;
    const int ls = blockIdx.x * REG_NT + threadIdx.x;
    if (c >= a.ctrl[1] || ls >= chunk) return;
    const int s = s0 + ls;
    const int f = a.tframe[c], n = a.nlist[c];
    double *out = a.hyp + (((size_t)c * chunk + ls) * 4) * REG_HD;
    const double fx = a.K[(size_t)f * 4], fy = a.K[(size_t)f * 4 + 1];
    const double NaN = __builtin_nan("");
#pragma unroll
    for (int r = 0; r < 4; r++) {
        double R[9], t[3];
        const bool ok = s < a.n_samples && n >= 3 && hypothesis(a, f, a.coff[c], n, fx, fy, s, r, R, t);
#pragma unroll
        for (int k = 0; k < 9; k++) out[r * REG_HD + k] = ok ? R[k] : NaN;
#pragma unroll
        for (int k = 0; k < 3; k++) out[r * REG_HD + 9 + k] = ok ? t[k] : NaN;
    }
}

// the hot path: a workgroup scores 256 hypotheses of one target against all its correspondences
__global__ __launch_bounds__(REG_NT) void k_reg_score(RegArgs a, int s0, int chunk)
{
    __shared__ double s_x[REG_NT], s_y[REG_NT], s_z[REG_NT], s_u[REG_NT], s_v[REG_NT];
    __shared__ unsigned long long s_key[REG_NT / 64];
    const int c = blockIdx.y;
    if (c >= a.ctrl[1] || (4 * s0) / REG_NT + (int)blockIdx.x >= a.nblk) return;   // a last chunk may reach past n_samples
    const int lh = blockIdx.x * REG_NT + threadIdx.x;   // hypothesis within the chunk
    const int h = 4 * s0 + lh;
    const int f = a.tframe[c], n = a.nlist[c], base = a.coff[c];
    const double fx = a.K[(size_t)f * 4], fy = a.K[(size_t)f * 4 + 1], ip = a.inlier_px;
    double R[9], t[3];
    bool valid = lh < 4 * chunk && h < 4 * a.n_samples;
    if (valid) {
        const double *hp = a.hyp + ((size_t)c * chunk * 4 + lh) * REG_HD;
#pragma unroll
        for (int k = 0; k < 9; k++) R[k] = hp[k];
#pragma unroll
        for (int k = 0; k < 3; k++) t[k] = hp[9 + k];
        valid = R[0] == R[0];
    }
    int cnt = 0;
    for (int j0 = 0; j0 < n; j0 += REG_NT) {
        const int j = j0 + threadIdx.x;
        if (j < n) {
            s_x[threadIdx.x] = a.cx[base + j];
            s_y[threadIdx.x] = a.cy[base + j];
            s_z[threadIdx.x] = a.cz[base + j];
            s_u[threadIdx.x] = a.cu[base + j];
            s_v[threadIdx.x] = a.cv[base + j];
        }
        __syncthreads();
        const int m = n - j0 < REG_NT ? n - j0 : REG_NT;
        if (valid) {
#pragma unroll 4
            for (int i = 0; i < m; i++) cnt += inlier(R, t, fx, fy, ip, s_x[i], s_y[i], s_z[i], s_u[i], s_v[i]) ? 1 : 0;
        }
        __syncthreads();
    }
    const unsigned long long key = ransac_block_max<REG_NT>(ransac_key(valid, cnt, h), s_key);
    if (threadIdx.x == 0) a.best[(size_t)c * a.nblk + (4 * s0) / REG_NT + blockIdx.x] = key;
}

// cost of the pose over the inliers of (R0, t0): sum of squared pixel errors, division form
__device__ double reg_cost(const RegArgs &a, int base, int n, double fx, double fy, double ip, const double (&R0)[9], const double (&t0)[3],
                           const double (&R)[9], const double (&t)[3], double (*sh)[REG_NT / 64])
{
    double v[1] = {0.0};
    for (int j = threadIdx.x; j < n; j += REG_NT) {
        const double X0 = a.cx[base + j], X1 = a.cy[base + j], X2 = a.cz[base + j], cu = a.cu[base + j], cv = a.cv[base + j];
        if (!inlier(R0, t0, fx, fy, ip, X0, X1, X2, cu, cv)) continue;
        const double x = ((R[0] * X0 + R[1] * X1) + R[2] * X2) + t[0];
        const double y = ((R[3] * X0 + R[4] * X1) + R[5] * X2) + t[1];
        const double z = ((R[6] * X0 + R[7] * X1) + R[8] * X2) + t[2];
        const double ru = fx * (x / z) + cu, rv = fy * (y / z) + cv;
        v[0] += ru * ru + rv * rv;
    }
    block_sums<1>(v, sh);
    return v[0];
}

// one workgroup per target: the winner (the largest key over the scoring workgroups) and its hypothesis again
__global__ __launch_bounds__(REG_NT) void k_reg_pick(RegArgs a)
{
    __shared__ unsigned long long s_key[REG_NT / 64];
    const int c = blockIdx.x;
    if (c >= a.ctrl[1]) return;
    const unsigned long long key = ransac_block_max<REG_NT>(ransac_row_max<REG_NT>(a.best, c, a.nblk, 0, a.nblk), s_key);
    if (threadIdx.x != 0) return;
    const int f = a.tframe[c], n = a.nlist[c];
    double *out = a.win + (size_t)c * 16;
    int win = -1, flags = 0;
    double R[9], t[3];
    if (n < 3) {
        flags = PGX_REG_FEWPOINTS;
    } else if (key == 0ull) {
        flags = PGX_REG_NOSOLUTION;
    } else {
        const int h = ransac_key_index(key);
        if (hypothesis(a, f, a.coff[c], n, a.K[(size_t)f * 4], a.K[(size_t)f * 4 + 1], h >> 2, h & 3, R, t))
            win = h >> 2;
        else
            flags = PGX_REG_NOSOLUTION;   // not reached: the scored hypothesis exists
    }
    for (int k = 0; k < 9; k++) out[k] = win >= 0 ? R[k] : 0.0;
    for (int k = 0; k < 3; k++) out[9 + k] = win >= 0 ? t[k] : 0.0;
    a.winfo[2 * c] = win;
    a.winfo[2 * c + 1] = flags;
}

__global__ __launch_bounds__(REG_NT) void k_reg_refine(RegArgs a)
{
    __shared__ double s_sum[28][REG_NT / 64];
    const int c = blockIdx.x;
    if (c >= a.ctrl[1]) return;
    const int f = a.tframe[c], n = a.nlist[c], base = a.coff[c];
    const double fx = a.K[(size_t)f * 4], fy = a.K[(size_t)f * 4 + 1], ip = a.inlier_px;
    const double NaN = __builtin_nan("");
    const int win = a.winfo[2 * c];
    int flags = a.winfo[2 * c + 1];
    // the pose through LDS: it then lives in vector registers (scalar loads of the uniform pose run out of SGPRs)
    __shared__ double s_pose[12];
    if (threadIdx.x < 12) s_pose[threadIdx.x] = a.win[(size_t)c * 16 + threadIdx.x];
    __syncthreads();
    double R[9], t[3];
#pragma unroll
    for (int k = 0; k < 9; k++) R[k] = s_pose[k];
#pragma unroll
    for (int k = 0; k < 3; k++) t[k] = s_pose[9 + k];
    int fin = 0;
    if (win >= 0) {
        double R0[9], t0[3];
#pragma unroll
        for (int k = 0; k < 9; k++) R0[k] = R[k];
#pragma unroll
        for (int k = 0; k < 3; k++) t0[k] = t[k];
        double C = reg_cost(a, base, n, fx, fy, ip, R0, t0, R, t, s_sum);
        for (int it = 0; it < a.refine_iters; it++) {
            // normal equations over the winner's inliers: A (21, upper triangle by rows), g (6)
            double v[27];
#pragma unroll
            for (int k = 0; k < 27; k++) v[k] = 0.0;
            for (int j = threadIdx.x; j < n; j += REG_NT) {
                const double X0 = a.cx[base + j], X1 = a.cy[base + j], X2 = a.cz[base + j], cu = a.cu[base + j], cv = a.cv[base + j];
                if (!inlier(R0, t0, fx, fy, ip, X0, X1, X2, cu, cv)) continue;
                const double q0 = (R[0] * X0 + R[1] * X1) + R[2] * X2;
                const double q1 = (R[3] * X0 + R[4] * X1) + R[5] * X2;
                const double q2 = (R[6] * X0 + R[7] * X1) + R[8] * X2;
                const double x = q0 + t[0], y = q1 + t[1], z = q2 + t[2];
                const double pu = x / z, pv = y / z;
                const double r[2] = {fx * pu + cu, fy * pv + cv};
                const double am[2][3] = {{fx / z, 0.0, -(fx * pu) / z}, {0.0, fy / z, -(fy * pv) / z}};
                double J[2][6];
#pragma unroll
                for (int rr = 0; rr < 2; rr++) {
                    J[rr][0] = q1 * am[rr][2] - q2 * am[rr][1];
                    J[rr][1] = q2 * am[rr][0] - q0 * am[rr][2];
                    J[rr][2] = q0 * am[rr][1] - q1 * am[rr][0];
                    J[rr][3] = am[rr][0];
                    J[rr][4] = am[rr][1];
                    J[rr][5] = am[rr][2];
                }
                int k = 0;
#pragma unroll
                for (int p = 0; p < 6; p++)
#pragma unroll
                    for (int q = p; q < 6; q++) v[k++] += J[0][p] * J[0][q] + J[1][p] * J[1][q];
#pragma unroll
                for (int p = 0; p < 6; p++) v[21 + p] += J[0][p] * r[0] + J[1][p] * r[1];
            }
            block_sums<27>(v, s_sum);
            // Cholesky of A, then delta = -A^-1 g
            double L[6][6];
            bool pd = true;
            {
                int k = 0;
#pragma unroll
                for (int p = 0; p < 6; p++)
#pragma unroll
                    for (int q = p; q < 6; q++) {
                        L[q][p] = v[k];
                        L[p][q] = v[k];
                        k++;
                    }
            }
#pragma unroll
            for (int j = 0; j < 6; j++) {
                double d = L[j][j];
#pragma unroll
                for (int k = 0; k < j; k++) d -= L[j][k] * L[j][k];
                pd = pd && d > 0.0;
                const double lj = sqrt(d);
                L[j][j] = lj;
#pragma unroll
                for (int i = j + 1; i < 6; i++) {
                    double s = L[i][j];
#pragma unroll
                    for (int k = 0; k < j; k++) s -= L[i][k] * L[j][k];
                    L[i][j] = s / lj;
                }
            }
            if (!pd) break;
            double z6[6], d6[6];
#pragma unroll
            for (int i = 0; i < 6; i++) {
                double s = -v[21 + i];
#pragma unroll
                for (int k = 0; k < i; k++) s -= L[i][k] * z6[k];
                z6[i] = s / L[i][i];
            }
#pragma unroll
            for (int i = 5; i >= 0; i--) {
                double s = z6[i];
#pragma unroll
                for (int k = i + 1; k < 6; k++) s -= L[k][i] * d6[k];
                d6[i] = s / L[i][i];
            }
            double dn = 0.0;
#pragma unroll
            for (int k = 0; k < 6; k++) dn += d6[k] * d6[k];
            const double tn = sqrt((t[0] * t[0] + t[1] * t[1]) + t[2] * t[2]);
            if (!(sqrt(dn) > 1e-12 * (1.0 + tn))) break;
            double Rn[9], tnw[3];
            rotate_left(d6, R, Rn);
#pragma unroll
            for (int k = 0; k < 3; k++) tnw[k] = t[k] + d6[3 + k];
            const double Cn = reg_cost(a, base, n, fx, fy, ip, R0, t0, Rn, tnw, s_sum);
            if (!(Cn < C)) break;
            C = Cn;
#pragma unroll
            for (int k = 0; k < 9; k++) R[k] = Rn[k];
#pragma unroll
            for (int k = 0; k < 3; k++) t[k] = tnw[k];
        }
        // the final classification with the refined pose
        double v[2] = {0.0, 0.0};   // inliers, sum e^2
        double mx = 0.0;
        for (int j = threadIdx.x; j < n; j += REG_NT) {
            const double X0 = a.cx[base + j], X1 = a.cy[base + j], X2 = a.cz[base + j], cu = a.cu[base + j], cv = a.cv[base + j];
            const bool in = inlier(R, t, fx, fy, ip, X0, X1, X2, cu, cv);
            if (a.node_inlier) a.node_inlier[a.corr_node[base + j]] = in ? 1 : 0;
            if (!in) continue;
            const double x = ((R[0] * X0 + R[1] * X1) + R[2] * X2) + t[0];
            const double y = ((R[3] * X0 + R[4] * X1) + R[5] * X2) + t[1];
            const double z = ((R[6] * X0 + R[7] * X1) + R[8] * X2) + t[2];
            const double ru = fx * (x / z) + cu, rv = fy * (y / z) + cv;
            const double e2 = ru * ru + rv * rv;
            v[0] += 1.0;
            v[1] += e2;
            mx = nan_max(mx, sqrt(e2));
        }
        mx = gmax<64>(mx);
        block_sums<2>(v, s_sum);
        if ((threadIdx.x & 63) == 0) s_sum[2][threadIdx.x >> 6] = mx;
        __syncthreads();
        mx = nan_max(nan_max(s_sum[2][0], s_sum[2][1]), nan_max(s_sum[2][2], s_sum[2][3]));
        fin = (int)v[0];
        if (threadIdx.x == 0) {
            a.frame_err[2 * f] = fin > 0 ? sqrt(v[1] / fin) : NaN;
            a.frame_err[2 * f + 1] = fin > 0 ? mx : NaN;
        }
        if (fin < a.min_inliers) flags |= PGX_REG_FEWINLIERS;
    } else {
        for (int j = threadIdx.x; j < n; j += REG_NT)
            if (a.node_inlier) a.node_inlier[a.corr_node[base + j]] = 0;
        if (threadIdx.x == 0) {
            a.frame_err[2 * f] = NaN;
            a.frame_err[2 * f + 1] = NaN;
        }
    }
    if (threadIdx.x == 0) {
        const double *K = a.K + (size_t)f * 4;
        const double S0 = a.S[4 * c], S1 = a.S[4 * c + 1], S2 = a.S[4 * c + 2];
        double r[12];
        const bool good = flags == 0;
        for (int k = 0; k < 9; k++) r[k] = good ? R[k] : NaN;
        for (int k = 0; k < 3; k++) r[9 + k] = good ? t[k] - ((R[3 * k] * S0 + R[3 * k + 1] * S1) + R[3 * k + 2] * S2) : NaN;
        double *o = a.Rt_out + (size_t)f * 12, *P = a.P_out + (size_t)f * 12;
        for (int k = 0; k < 12; k++) o[k] = r[k];
        camera_matrix(K, r, true, P);   // NaN rows come from r itself
        int32_t *st = a.frame_stats + (size_t)f * 4;
        st[0] = n;
        st[1] = fin;
        st[2] = win;
        st[3] = flags;
    }
}

__global__ __launch_bounds__(REG_NT) void k_reg_summary(RegArgs a)
{
    __shared__ int s_acc[8];
    if (threadIdx.x < 8) s_acc[threadIdx.x] = 0;
    __syncthreads();
    int acc[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    for (int f = threadIdx.x; f < a.tv.n_frames; f += blockDim.x) {
        if (a.reg[f] == 0) continue;
        const int32_t *st = a.frame_stats + (size_t)f * 4;
        acc[0] += 1;
        acc[1] += st[3] == 0;
#pragma unroll
        for (int b = 0; b < 4; b++) acc[2 + b] += (st[3] >> b) & 1;
        acc[6] += st[0];
        acc[7] += st[1];
    }
#pragma unroll
    for (int k = 0; k < 8; k++)
        if (acc[k]) atomicAdd(&s_acc[k], acc[k]);   // integer sums: the order does not matter
    __syncthreads();
    if (threadIdx.x < 8) a.report[threadIdx.x] = s_acc[threadIdx.x];
}

int reg_chunk(int n_frames, int n_samples)
{
    return ransac_chunk(REG_CHUNK_CELLS, n_frames, 64, n_samples);   // 64 samples = 256 hypotheses: one scoring workgroup
}

// the workspace, described once: a's workspace pointers (none valid for ws = nullptr) and nblk; the bytes
size_t reg_carve(RegArgs &a, void *ws)
{
    const size_t N = (size_t)(a.tv.node_cap > 0 ? a.tv.node_cap : 1), NF = (size_t)a.tv.n_frames;
    const size_t chunk = (size_t)reg_chunk(a.tv.n_frames, a.n_samples);
    a.nblk = (int)((4ll * a.n_samples + REG_NT - 1) / REG_NT);
    WsCarver w(ws);
    a.ctrl = w.take<int32_t>(8 * 4);
    a.tv.inv = w.take<int32_t>(NF * 4);
    a.tnum = w.take<int32_t>(NF * 4);
    a.tframe = w.take<int32_t>(NF * 4);
    a.cnt = w.take<int32_t>(NF * 4);
    a.coff = w.take<int32_t>(NF * 4);
    a.nlist = w.take<int32_t>(NF * 4);
    a.cf = w.take<int32_t>(N * 4);
    a.corr_node = w.take<int32_t>(N * 4);
    a.cx = w.take<double>(N * 8);
    a.cy = w.take<double>(N * 8);
    a.cz = w.take<double>(N * 8);
    a.cu = w.take<double>(N * 8);
    a.cv = w.take<double>(N * 8);
    a.S = w.take<double>(NF * 4 * 8);
    a.win = w.take<double>(NF * 16 * 8);
    a.winfo = w.take<int32_t>(NF * 2 * 4);
    a.hyp = w.take<double>(NF * chunk * 4 * REG_HD * 8);
    a.best = w.take<unsigned long long>(NF * (size_t)a.nblk * 8);
    return w.total();
}

} // namespace

size_t pgx_register_ws_bytes(const RegArgs &a)
{
    RegArgs b = a;
    return reg_carve(b, nullptr);
}

void pgx_launch_register(hipStream_t s, RegArgs a, void *ws)
{
    reg_carve(a, ws);
    const int n_frames = a.tv.n_frames, chunk = reg_chunk(n_frames, a.n_samples);
    const long long want = ((long long)a.tv.max_tracks * REG_G + REG_NT - 1) / REG_NT;
    const int grid = (int)(want < 1 ? 1 : (want > REG_GRID_MAX ? REG_GRID_MAX : want));
    hipLaunchKernelGGL(k_reg_frames, dim3(1), dim3(REG_NT), 0, s, a);
    hipLaunchKernelGGL(k_reg_count, dim3(grid), dim3(REG_NT), 0, s, a);
    hipLaunchKernelGGL(k_reg_csr, dim3(n_frames), dim3(REG_NT), 0, s, a);
    for (int s0 = 0; s0 < a.n_samples; s0 += chunk) {
        hipLaunchKernelGGL(k_reg_hyp, dim3((chunk + REG_NT - 1) / REG_NT, n_frames), dim3(REG_NT), 0, s, a, s0, chunk);
        hipLaunchKernelGGL(k_reg_score, dim3(4 * chunk / REG_NT, n_frames), dim3(REG_NT), 0, s, a, s0, chunk);
    }
    hipLaunchKernelGGL(k_reg_pick, dim3(n_frames), dim3(REG_NT), 0, s, a);
    hipLaunchKernelGGL(k_reg_refine, dim3(n_frames), dim3(REG_NT), 0, s, a);
    hipLaunchKernelGGL(k_reg_summary, dim3(1), dim3(REG_NT), 0, s, a);
}
