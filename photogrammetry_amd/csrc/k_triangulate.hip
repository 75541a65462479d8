// k_triangulate.hip -- multi-view triangulation of the track graph's tracks (pgx_triangulate_tracks_dev; include/pgx.h).
//
// The reference triangulates the keypoint pairs of one image pair (CameraPoseEstimation.cs:96-202) and hands the points to
// Utils.CreatePointCloud.  Here every track of pgx_tracks_dev / pgx_tracks_split_dev becomes one point, over all its views.
//
// Kernels (three launches, all on the caller's stream; n_tracks is read on the device):
//   k_tri_frames   one workgroup: per frame the camera's state (centre C = -M^-1 p4, sign det M, ||m3||, known), the
//                  slot -> frame inverse (PGX_ST_TRI_DUP) and the number of tracks to process (PGX_ST_TRI_CAP)
//   k_tri_tracks   persistent, grid-stride over the tracks in three phases by length: tracks of more than 32 nodes get a
//                  whole wave (G = 64 lanes), 9..32 nodes a quarter wave (G = 16), 0..8 nodes G = 4 lanes.  Lane l of a
//                  group takes the observations l, l + G, ...; every per-track sum is a per-lane sum followed by an xor
//                  butterfly over the G lanes, which leaves identical bits in every lane (a + b == b + a) and depends on the
//                  track's length only -- so the result does not depend on the grid, the slot layout or the run.  Each
//                  pass re-reads its observations (8 B node, 8 B keypoint, 96 B camera: L1/L2 resident); nothing per
//                  observation is kept in registers, so no array is indexed at run time.  The 4x4 Gram matrix's cyclic
//                  Jacobi and the 3x3 solve are redundant in the G lanes, fully unrolled over constant indices.
//   k_tri_summary  one workgroup: the per-workgroup counters of k_tri_tracks (no same-address atomics over the grid)
//                  summed into d_summary.
// DESIGN.md section 15 has the lane mapping's measurements.
#include "pgx_stage_args.h"

namespace {

constexpr int TRI_NT = 256;          // threads per workgroup of every kernel here
constexpr int TRI_GRID_MAX = 1024;   // workgroups of k_tri_tracks (4 per CU), at most
constexpr int TRI_JACOBI_SWEEPS = 8; // cyclic sweeps over the 6 pairs of the 4x4 Gram matrix (quadratic convergence: 3-4 suffice)
constexpr int CAM_STRIDE = 8;        // doubles per frame in the camera table: C (3), sign det M, ||m3||, known (1 / 0), 2 unused

// observation o of d_nodes: true if it is used (valid node, known camera); bad = the node itself is invalid.  The node
// test and the keypoint fetch (and tri_phase's offsets test) stay written out here, not node_ok / node_keypoint /
// track_range of pgx_trackgraph.h: k_tri_tracks sits at the SGPR limit, and either helper's shape makes the register
// allocator spill scalars (tests/test_triangulate_codegen.py pins zero spills).
__device__ __forceinline__ bool tri_obs(const TriArgs &a, long long o, int &f, double &u, double &v, bool &bad)
{
    const int fr = a.tv.nodes[2 * o], k = a.tv.nodes[2 * o + 1];
    bad = false;
    if (fr < 0 || fr >= a.tv.n_frames || k < 0 || k >= a.tv.stride) { bad = true; return false; }
    const int s = a.tv.inv[fr];
    if (s < 0) { bad = true; return false; }
    if (a.cam[(size_t)fr * CAM_STRIDE + 5] == 0.0) return false;
    const pgx_keypoint p = a.tv.kp[(size_t)s * a.tv.stride + k];
    f = fr;
    u = (double)p.x;
    v = (double)p.y;
    return true;
}

// P'_f = [M | p4 + M S] (the camera in the frame shifted to S)
__device__ __forceinline__ void shifted_camera(const TriArgs &a, int f, double S0, double S1, double S2, double (&Q)[12])
{
    const double *p = a.P + (size_t)f * 12;
#pragma unroll
    for (int r = 0; r < 3; r++) {
        Q[4 * r + 0] = p[4 * r + 0];
        Q[4 * r + 1] = p[4 * r + 1];
        Q[4 * r + 2] = p[4 * r + 2];
        Q[4 * r + 3] = p[4 * r + 3] + (p[4 * r + 0] * S0 + p[4 * r + 1] * S1 + p[4 * r + 2] * S2);
    }
}

// one Jacobi rotation of the symmetric A (zeroes A[p][q]), accumulated into the eigenvector columns of V
template <int p, int q> __device__ __forceinline__ void jacobi_rot(double (&A)[4][4], double (&V)[4][4])
{
    const double apq = A[p][q];
    if (apq == 0.0) return;
    const double theta = (A[q][q] - A[p][p]) / (2.0 * apq);
    const double t = (theta >= 0.0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
    const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const double akp = A[k][p], akq = A[k][q];
        A[k][p] = c * akp - s * akq;
        A[k][q] = s * akp + c * akq;
    }
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const double apk = A[p][k], aqk = A[q][k];
        A[p][k] = c * apk - s * aqk;
        A[q][k] = s * apk + c * aqk;
    }
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const double vkp = V[k][p], vkq = V[k][q];
        V[k][p] = c * vkp - s * vkq;
        V[k][q] = s * vkp + c * vkq;
    }
}

// per-track results and the group leader's counters
__device__ __forceinline__ void write_track(const TriArgs &a, long long t, double x, double y, double z, double rms, double mx, double par,
                                           int fl, int used, int (&acc)[8])
{
    a.xyz[3 * t + 0] = x;
    a.xyz[3 * t + 1] = y;
    a.xyz[3 * t + 2] = z;
    a.quality[3 * t + 0] = rms;
    a.quality[3 * t + 1] = mx;
    a.quality[3 * t + 2] = par;
    a.flags[t] = fl;
    acc[1] += fl == 0;
#pragma unroll
    for (int b = 0; b < 5; b++) acc[2 + b] += (fl >> b) & 1;
    acc[7] += used;
}

__device__ __forceinline__ int len_class(int n) { return n > 32 ? 2 : (n > 8 ? 1 : 0); }

// every track of length class CLS, G lanes per track
template <int G, int CLS> __device__ void tri_phase(const TriArgs &a, long long nt, int (&acc)[8])
{
    const double NaN = __builtin_nan("");
    PGX_TRACK_LOOP(G, nt)
    {
        const int o0 = a.tv.offsets[t], o1 = a.tv.offsets[t + 1];
        const bool malformed = o0 < 0 || o1 < o0 || (long long)o1 > a.tv.node_cap;
        const int n = malformed ? 0 : o1 - o0;
        if (len_class(n) != CLS) continue;
        if (malformed && lane == 0) atomicOr(a.status, (int)PGX_ST_TRI_NODE);

        // pass 1: used observations and the mean of their camera centres
        int cnt = 0;
        double s0 = 0.0, s1 = 0.0, s2 = 0.0;
        for (int i = lane; i < n; i += G) {
            int f;
            double u, v;
            bool bad;
            if (tri_obs(a, (long long)o0 + i, f, u, v, bad)) {
                const double *c = a.cam + (size_t)f * CAM_STRIDE;
                cnt++;
                s0 += c[0];
                s1 += c[1];
                s2 += c[2];
            }
            if (bad) atomicOr(a.status, (int)PGX_ST_TRI_NODE);
        }
        cnt = gsum_i<G>(cnt);
        if (cnt < 2) {
            if (a.node_err)
                for (int i = lane; i < n; i += G) a.node_err[(long long)o0 + i] = NaN;
            if (lane == 0) write_track(a, t, NaN, NaN, NaN, NaN, NaN, NaN, PGX_TRI_FEWVIEWS, cnt, acc);
            continue;
        }
        s0 = gsum<G>(s0);
        s1 = gsum<G>(s1);
        s2 = gsum<G>(s2);
        const double S0 = s0 / cnt, S1 = s1 / cnt, S2 = s2 / cnt;

        // pass 2: Gram matrix of the unit-norm rows in the shifted frame
        double g[10];
#pragma unroll
        for (int k = 0; k < 10; k++) g[k] = 0.0;
        for (int i = lane; i < n; i += G) {
            int f;
            double u, v;
            bool bad;
            if (!tri_obs(a, (long long)o0 + i, f, u, v, bad)) continue;
            double Q[12];
            shifted_camera(a, f, S0, S1, S2, Q);
            double r1[4], r2[4];
#pragma unroll
            for (int k = 0; k < 4; k++) {
                r1[k] = u * Q[8 + k] - Q[k];
                r2[k] = v * Q[8 + k] - Q[4 + k];
            }
            const double n1 = sqrt(r1[0] * r1[0] + r1[1] * r1[1] + r1[2] * r1[2] + r1[3] * r1[3]);
            const double n2 = sqrt(r2[0] * r2[0] + r2[1] * r2[1] + r2[2] * r2[2] + r2[3] * r2[3]);
#pragma unroll
            for (int k = 0; k < 4; k++) {
                r1[k] = r1[k] / n1;
                r2[k] = r2[k] / n2;
            }
            int e = 0;
#pragma unroll
            for (int j = 0; j < 4; j++)
#pragma unroll
                for (int k = j; k < 4; k++, e++) {
                    g[e] += r1[j] * r1[k];
                    g[e] += r2[j] * r2[k];
                }
        }
#pragma unroll
        for (int k = 0; k < 10; k++) g[k] = gsum<G>(g[k]);
        double A[4][4], V[4][4];
        {
            int e = 0;
#pragma unroll
            for (int j = 0; j < 4; j++)
#pragma unroll
                for (int k = j; k < 4; k++, e++) { A[j][k] = g[e]; A[k][j] = g[e]; }
#pragma unroll
            for (int j = 0; j < 4; j++)
#pragma unroll
                for (int k = 0; k < 4; k++) V[j][k] = j == k ? 1.0 : 0.0;
        }
#pragma unroll 1
        for (int sw = 0; sw < TRI_JACOBI_SWEEPS; sw++) {
            jacobi_rot<0, 1>(A, V);
            jacobi_rot<0, 2>(A, V);
            jacobi_rot<0, 3>(A, V);
            jacobi_rot<1, 2>(A, V);
            jacobi_rot<1, 3>(A, V);
            jacobi_rot<2, 3>(A, V);
        }
        double v0 = V[0][0], v1 = V[1][0], v2 = V[2][0], v3 = V[3][0], best = A[0][0];
#pragma unroll
        for (int c = 1; c < 4; c++)
            if (A[c][c] < best) { best = A[c][c]; v0 = V[0][c]; v1 = V[1][c]; v2 = V[2][c]; v3 = V[3][c]; }
        if (!(isfinite(v0) && isfinite(v1) && isfinite(v2) && isfinite(v3)) || fabs(v3) <= 1e-12) {
            if (a.node_err)
                for (int i = lane; i < n; i += G) a.node_err[(long long)o0 + i] = NaN;
            if (lane == 0) write_track(a, t, NaN, NaN, NaN, NaN, NaN, NaN, PGX_TRI_DEGENERATE, cnt, acc);
            continue;
        }
        double X0 = v0 / v3, X1 = v1 / v3, X2 = v2 / v3;   // in the shifted frame

        // Gauss-Newton: each pass is the cost (and, while steps remain, the normal equations) at the current point
        if (a.refine_iters > 0) {
            double P0 = X0, P1 = X1, P2 = X2, cost_prev = 0.0;
            for (int it = 0;; it++) {
                const bool step = it < a.refine_iters;
                double c = 0.0, h[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0}, gv[3] = {0.0, 0.0, 0.0};
                for (int i = lane; i < n; i += G) {
                    int f;
                    double u, v;
                    bool bad;
                    if (!tri_obs(a, (long long)o0 + i, f, u, v, bad)) continue;
                    double Q[12];
                    shifted_camera(a, f, S0, S1, S2, Q);
                    const double x = Q[0] * X0 + Q[1] * X1 + Q[2] * X2 + Q[3];
                    const double y = Q[4] * X0 + Q[5] * X1 + Q[6] * X2 + Q[7];
                    const double z = Q[8] * X0 + Q[9] * X1 + Q[10] * X2 + Q[11];
                    const double pu = x / z, pv = y / z, ru = pu - u, rv = pv - v;
                    c += ru * ru + rv * rv;
                    if (step) {
                        double ju[3], jv[3];
#pragma unroll
                        for (int k = 0; k < 3; k++) {
                            ju[k] = (Q[k] - pu * Q[8 + k]) / z;
                            jv[k] = (Q[4 + k] - pv * Q[8 + k]) / z;
                        }
                        int e = 0;
#pragma unroll
                        for (int j = 0; j < 3; j++)
#pragma unroll
                            for (int k = j; k < 3; k++, e++) {
                                h[e] += ju[j] * ju[k];
                                h[e] += jv[j] * jv[k];
                            }
#pragma unroll
                        for (int k = 0; k < 3; k++) {
                            gv[k] += ju[k] * ru;
                            gv[k] += jv[k] * rv;
                        }
                    }
                }
                c = gsum<G>(c);
                if (it > 0 && !(c < cost_prev)) { X0 = P0; X1 = P1; X2 = P2; break; }
                if (!step) break;
#pragma unroll
                for (int k = 0; k < 6; k++) h[k] = gsum<G>(h[k]);
#pragma unroll
                for (int k = 0; k < 3; k++) gv[k] = gsum<G>(gv[k]);
                // d = -H^-1 g by the adjugate; h = (00, 01, 02, 11, 12, 22)
                const double c00 = h[3] * h[5] - h[4] * h[4], c01 = h[2] * h[4] - h[1] * h[5], c02 = h[1] * h[4] - h[2] * h[3];
                const double c11 = h[0] * h[5] - h[2] * h[2], c12 = h[1] * h[2] - h[0] * h[4], c22 = h[0] * h[3] - h[1] * h[1];
                const double det = h[0] * c00 + h[1] * c01 + h[2] * c02;
                const double d0 = -(c00 * gv[0] + c01 * gv[1] + c02 * gv[2]) / det;
                const double d1 = -(c01 * gv[0] + c11 * gv[1] + c12 * gv[2]) / det;
                const double d2 = -(c02 * gv[0] + c12 * gv[1] + c22 * gv[2]) / det;
                const double W0 = S0 + X0, W1 = S1 + X1, W2 = S2 + X2;
                if (sqrt(d0 * d0 + d1 * d1 + d2 * d2) <= 1e-12 * (1.0 + sqrt(W0 * W0 + W1 * W1 + W2 * W2))) break;
                P0 = X0; P1 = X1; P2 = X2;
                cost_prev = c;
                X0 = X0 + d0; X1 = X1 + d1; X2 = X2 + d2;
            }
        }

        // quality: reprojection errors, depths, the widest pair of rays
        double se = 0.0, me = 0.0, cmax = 0.0;
        int behind = 0;
        for (int i = lane; i < n; i += G) {
            const long long o = (long long)o0 + i;
            int f;
            double u, v;
            bool bad;
            if (!tri_obs(a, o, f, u, v, bad)) {
                if (a.node_err) a.node_err[o] = NaN;
                continue;
            }
            double Q[12];
            shifted_camera(a, f, S0, S1, S2, Q);
            const double x = Q[0] * X0 + Q[1] * X1 + Q[2] * X2 + Q[3];
            const double y = Q[4] * X0 + Q[5] * X1 + Q[6] * X2 + Q[7];
            const double z = Q[8] * X0 + Q[9] * X1 + Q[10] * X2 + Q[11];
            const double ru = x / z - u, rv = y / z - v;
            const double e = sqrt(ru * ru + rv * rv);
            if (a.node_err) a.node_err[o] = e;
            se += e * e;
            me = nan_max(me, e);
            const double *ci = a.cam + (size_t)f * CAM_STRIDE;
            behind |= ci[3] * z / ci[4] <= 0.0;
            double a0 = (ci[0] - S0) - X0, a1 = (ci[1] - S1) - X1, a2 = (ci[2] - S2) - X2;
            const double na = sqrt(a0 * a0 + a1 * a1 + a2 * a2);
            a0 = a0 / na; a1 = a1 / na; a2 = a2 / na;
            for (int j = i + 1; j < n; j++) {
                int fj;
                double uj, vj;
                bool badj;
                if (!tri_obs(a, (long long)o0 + j, fj, uj, vj, badj)) continue;
                const double *cj = a.cam + (size_t)fj * CAM_STRIDE;
                double b0 = (cj[0] - S0) - X0, b1 = (cj[1] - S1) - X1, b2 = (cj[2] - S2) - X2;
                const double nb = sqrt(b0 * b0 + b1 * b1 + b2 * b2);
                b0 = b0 / nb - a0; b1 = b1 / nb - a1; b2 = b2 / nb - a2;
                const double ch = b0 * b0 + b1 * b1 + b2 * b2;   // |d_i - d_j|^2 = (2 sin(angle / 2))^2
                cmax = ch > cmax ? ch : cmax;                     // a NaN chord (a centre on the point) counts as 0
            }
        }
        se = gsum<G>(se);
        me = gmax<G>(me);
        cmax = gmax<G>(cmax);
        behind = gsum_i<G>(behind);
        if (lane == 0) {
            const double par = 2.0 * asin(fmin(1.0, sqrt(cmax) * 0.5)) * (180.0 / M_PI);
            const int fl = (behind ? PGX_TRI_BEHIND : 0) | (par < a.min_par ? PGX_TRI_PARALLAX : 0) |
                           (!(me <= a.max_reproj) ? PGX_TRI_REPROJ : 0);
            write_track(a, t, S0 + X0, S1 + X1, S2 + X2, sqrt(se / cnt), me, par, fl, cnt, acc);
        }
    }
}

__global__ __launch_bounds__(TRI_NT) void k_tri_frames(TriArgs a)
{
    for (int f = threadIdx.x; f < a.tv.n_frames; f += blockDim.x) {
        const double *p = a.P + (size_t)f * 12;
        bool fin = true;
#pragma unroll
        for (int k = 0; k < 12; k++) fin = fin && isfinite(p[k]);
        const double m00 = p[0], m01 = p[1], m02 = p[2], m10 = p[4], m11 = p[5], m12 = p[6], m20 = p[8], m21 = p[9], m22 = p[10];
        // cofactors; M^-1 = adj(M) / det, adj = the cofactor matrix transposed
        const double k00 = m11 * m22 - m12 * m21, k01 = m12 * m20 - m10 * m22, k02 = m10 * m21 - m11 * m20;
        const double k10 = m02 * m21 - m01 * m22, k11 = m00 * m22 - m02 * m20, k12 = m01 * m20 - m00 * m21;
        const double k20 = m01 * m12 - m02 * m11, k21 = m02 * m10 - m00 * m12, k22 = m00 * m11 - m01 * m10;
        const double det = m00 * k00 + m01 * k01 + m02 * k02;
        const bool known = fin && det != 0.0;
        double *c = a.cam + (size_t)f * CAM_STRIDE;
        c[0] = -(k00 * p[3] + k10 * p[7] + k20 * p[11]) / det;
        c[1] = -(k01 * p[3] + k11 * p[7] + k21 * p[11]) / det;
        c[2] = -(k02 * p[3] + k12 * p[7] + k22 * p[11]) / det;
        c[3] = det > 0.0 ? 1.0 : -1.0;
        c[4] = sqrt(m20 * m20 + m21 * m21 + m22 * m22);
        c[5] = known ? 1.0 : 0.0;
        c[6] = 0.0;
        c[7] = 0.0;
        a.tv.inv[f] = -1;
    }
    if (threadIdx.x == 0) a.meta[0] = clamp_tracks(a.tv, a.status, PGX_ST_TRI_CAP);
    __syncthreads();
    build_slot_inverse(a.tv, a.status, PGX_ST_TRI_DUP);
}

__global__ __launch_bounds__(TRI_NT) void k_tri_tracks(TriArgs a)
{
    __shared__ int s_acc[8];
    if (threadIdx.x < 8) s_acc[threadIdx.x] = 0;
    __syncthreads();
    const long long nt = a.meta[0];
    int acc[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    tri_phase<64, 2>(a, nt, acc);   // the longest tracks first: they finish last
    tri_phase<16, 1>(a, nt, acc);
    tri_phase<4, 0>(a, nt, acc);
#pragma unroll
    for (int k = 1; k < 8; k++)
        if (acc[k]) atomicAdd(&s_acc[k], acc[k]);
    __syncthreads();
    if (threadIdx.x < 8) a.part[(size_t)blockIdx.x * 8 + threadIdx.x] = s_acc[threadIdx.x];
}

__global__ __launch_bounds__(TRI_NT) void k_tri_summary(TriArgs a, int nblk)
{
    __shared__ int s_sum[TRI_NT / 8][8];
    const int k = threadIdx.x & 7, sub = threadIdx.x >> 3;
    int v = 0;
    for (int b = sub; b < nblk; b += TRI_NT / 8) v += a.part[(size_t)b * 8 + k];
    s_sum[sub][k] = v;
    __syncthreads();
    if (threadIdx.x < 8) {
        int tot = 0;
        for (int j = 0; j < TRI_NT / 8; j++) tot += s_sum[j][threadIdx.x];
        a.summary[threadIdx.x] = threadIdx.x == 0 ? a.meta[0] : tot;
    }
}

int tri_grid(int max_tracks)
{
    const long long want = ((long long)max_tracks + 3) / 4;   // a whole wave per track if every track were long
    return (int)(want < 1 ? 1 : (want > TRI_GRID_MAX ? TRI_GRID_MAX : want));
}

// the workspace, described once: a's workspace pointers (none valid for ws = nullptr) and the bytes
size_t tri_carve(TriArgs &a, void *ws)
{
    const int n_frames = a.tv.n_frames;
    WsCarver w(ws);
    a.cam = w.take<double>((size_t)n_frames * CAM_STRIDE * sizeof(double));
    a.part = w.take<int32_t>((size_t)TRI_GRID_MAX * 8 * sizeof(int32_t));
    a.tv.inv = w.take<int32_t>((size_t)n_frames * sizeof(int32_t));
    a.meta = w.take<int32_t>(256);
    return w.total();
}

} // namespace

size_t pgx_triangulate_ws_bytes(const TriArgs &a)
{
    TriArgs b = a;
    return tri_carve(b, nullptr);
}

void pgx_launch_triangulate(hipStream_t s, TriArgs a, void *ws)
{
    tri_carve(a, ws);
    const int grid = tri_grid(a.tv.max_tracks);
    hipLaunchKernelGGL(k_tri_frames, dim3(1), dim3(TRI_NT), 0, s, a);
    hipLaunchKernelGGL(k_tri_tracks, dim3(grid), dim3(TRI_NT), 0, s, a);
    hipLaunchKernelGGL(k_tri_summary, dim3(1), dim3(TRI_NT), 0, s, a, grid);
}
