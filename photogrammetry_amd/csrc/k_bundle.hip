// k_bundle.hip -- bundle adjustment of cameras and track points (pgx_bundle_adjust_dev; include/pgx.h).
//
// Levenberg-Marquardt on the Huber reprojection cost of the tracks that take part, float64 throughout.  Every kernel of the
// iteration first reads the device control block (BaCtrl) and returns at once when the solve has stopped, so the host
// enqueues all max_iters iterations up front and never syncs (the live[] pattern of pgx_tracks_split_dev).
//
// Once per call:
//   k_ba_frames   one workgroup: K / Rt validation, the slot -> frame inverse, free frames numbered in frame order, the
//                 control block's initial state, the working cameras (a copy of Rt_in)
//   k_ba_setup    per track (G lanes): which nodes are used, whether the track takes part, the per-node free-camera index,
//                 per-camera observation counts (integer atomics: the counts do not depend on the order)
//   k_ba_csr      one workgroup per free camera: its used observations ordered by track (a block scan over the tracks)
//   k_ba_lin + k_ba_start   the first linearisation and the start cost C0
// Per iteration (max_iters times, each a no-op once `done`):
//   k_ba_lin      per track (G lanes, only after an accepted step): residuals, Huber weights, the 2x6 / 2x3 Jacobian blocks
//                 of every observation in a free frame (kept per node), V_t, g_t and the track's cost
//   k_ba_vinv     per track: (V_t + lambda D_t)^-1, or the non-PD flag
//   k_ba_schur    one workgroup per free camera a: the block row S_ab (b <= a) of the reduced system and its right-hand side,
//                 accumulated in the order of a's observation list (track order), 36 sums per thread b
//   k_ba_solve    one workgroup: blocked Cholesky (6 x 6 blocks) of S in place, both triangular solves, the trial cameras
//   k_ba_back     per track (G lanes): back-substitution for delta X, the trial point and the trial cost
//   k_ba_decide   one workgroup: fixed-order sums over the tracks, accept / reject, lambda, the trace row, the stop test
// At the end: k_ba_final (per track: xyz_out, node_err, z <= 0 count) and k_ba_out (Rt_out, P_out, report).
//
// Determinism: per-track sums are xor butterflies over G = 16 lanes (their bits depend on the track's length only), the
// reduced system's sums run in track order, and the sums over tracks are strided by 1024 and tree-reduced in a fixed shape.
// Nothing depends on the grid, max_tracks, the slot layout or the run.  DESIGN.md section 16 has the measurements.
#include "pgx_stage_args.h"

// what BaArgs::ctrl points to
struct BaCtrl {
    double lam, C, cam_dx2, cam_x2;
    int it, acc, reason, done, relin, sel, pdfail, nonpd;
    int n_free, n_fixed, err, nt, n_part, n_used, zneg, pad;
};

namespace {

constexpr int BA_G = 16;          // lanes per track in the per-track kernels
constexpr int BA_NT = 256;        // threads per workgroup of the per-track, per-camera and frame kernels
constexpr int BA_RED = 1024;      // threads of the reducing kernels (k_ba_start, k_ba_decide, k_ba_solve)
constexpr int BA_GRID_MAX = 1024; // workgroups of a per-track kernel, at most
constexpr int BA_MAX_FREE = 128;  // free frames, at most
constexpr int BA_LD = 6 * BA_MAX_FREE;  // leading dimension of S
constexpr int BA_CH = 32;         // tracks per chunk of k_ba_schur
constexpr int BA_ND = 21;         // doubles per node: Jc [2][6], Jp [2][3], r [2], w
constexpr int FS_UNKNOWN = -1, FS_FIXED = -2;   // frame state; >= 0: the free frame's number

// fixed-shape sum of v over the BA_RED threads of the workgroup (sh: BA_RED doubles of LDS); the result is in every thread
__device__ double block_sum(double v, double *sh)
{
    sh[threadIdx.x] = v;
    __syncthreads();
    for (int m = BA_RED / 2; m > 0; m >>= 1) {
        if ((int)threadIdx.x < m) sh[threadIdx.x] = sh[threadIdx.x] + sh[threadIdx.x + m];
        __syncthreads();
    }
    const double r = sh[0];
    __syncthreads();
    return r;
}

// rho(s) and the IRLS weight of a squared residual s under Huber delta (delta = +inf: s and 1)
__device__ __forceinline__ void huber(double s, double delta, double &rho, double &w)
{
    if (s <= delta * delta) {
        rho = s;
        w = 1.0;
    } else {
        const double rs = sqrt(s);
        rho = 2.0 * delta * rs - delta * delta;
        w = delta / rs;
    }
}

// one used observation: the residual, and the Jacobian rows wrt the point (jp) and the camera (jc = (omega, tau))
struct Obs {
    double ru, rv, z, jp[2][3], jc[2][6];
};

__device__ __forceinline__ void observe(const double *Rt, const double *K, const double *X, double ku, double kv, Obs &o)
{
    const double q0 = (Rt[0] * X[0] + Rt[1] * X[1]) + Rt[2] * X[2];
    const double q1 = (Rt[3] * X[0] + Rt[4] * X[1]) + Rt[5] * X[2];
    const double q2 = (Rt[6] * X[0] + Rt[7] * X[1]) + Rt[8] * X[2];
    const double x = q0 + Rt[9], y = q1 + Rt[10], z = q2 + Rt[11];
    const double pu = x / z, pv = y / z;
    o.ru = (K[0] * pu + K[2]) - ku;
    o.rv = (K[1] * pv + K[3]) - kv;
    o.z = z;
    // d(u, v)/d(x, y, z)
    const double a[2][3] = {{K[0] / z, 0.0, -(K[0] * pu) / z}, {0.0, K[1] / z, -(K[1] * pv) / z}};
    const double q[3] = {q0, q1, q2};
#pragma unroll
    for (int r = 0; r < 2; r++) {
#pragma unroll
        for (int c = 0; c < 3; c++) o.jp[r][c] = (a[r][0] * Rt[c] + a[r][1] * Rt[3 + c]) + a[r][2] * Rt[6 + c];
        // d/d omega = a . (-[q]x) = q x a
        o.jc[r][0] = q[1] * a[r][2] - q[2] * a[r][1];
        o.jc[r][1] = q[2] * a[r][0] - q[0] * a[r][2];
        o.jc[r][2] = q[0] * a[r][1] - q[1] * a[r][0];
        o.jc[r][3] = a[r][0];
        o.jc[r][4] = a[r][1];
        o.jc[r][5] = a[r][2];
    }
}

__device__ __forceinline__ void projection_only(const double *Rt, const double *K, const double *X, double ku, double kv, double &ru,
                                                double &rv, double &z)
{
    const double x = ((Rt[0] * X[0] + Rt[1] * X[1]) + Rt[2] * X[2]) + Rt[9];
    const double y = ((Rt[3] * X[0] + Rt[4] * X[1]) + Rt[5] * X[2]) + Rt[10];
    z = ((Rt[6] * X[0] + Rt[7] * X[1]) + Rt[8] * X[2]) + Rt[11];
    ru = (K[0] * (x / z) + K[2]) - ku;
    rv = (K[1] * (y / z) + K[3]) - kv;
}

// keypoint of node o (a used node: node_ok)
__device__ __forceinline__ void node_kp(const BaArgs &a, long long o, int &f, double &ku, double &kv)
{
    f = a.tv.nodes[2 * o];
    node_keypoint(a.tv, f, a.tv.nodes[2 * o + 1], ku, kv);
}

// ---- once per call ---------------------------------------------------------------------------------------------------

__global__ __launch_bounds__(BA_NT) void k_ba_frames(BaArgs a)
{
    for (int f = threadIdx.x; f < a.tv.n_frames; f += blockDim.x) {
        const double *K = a.K + (size_t)f * 4, *R = a.Rt_in + (size_t)f * 12;
        bool fin = K[0] != 0.0 && K[1] != 0.0;
#pragma unroll
        for (int k = 0; k < 4; k++) fin = fin && isfinite(K[k]);
#pragma unroll
        for (int k = 0; k < 12; k++) fin = fin && isfinite(R[k]);
        bool known = fin;
        if (fin) {
            double dev = 0.0;
#pragma unroll
            for (int i = 0; i < 3; i++)
#pragma unroll
                for (int j = 0; j < 3; j++) {
                    const double d = ((R[3 * i] * R[3 * j] + R[3 * i + 1] * R[3 * j + 1]) + R[3 * i + 2] * R[3 * j + 2]) - (i == j ? 1.0 : 0.0);
                    dev = fmax(dev, fabs(d));
                }
            const double det = R[0] * (R[4] * R[8] - R[5] * R[7]) - R[1] * (R[3] * R[8] - R[5] * R[6]) + R[2] * (R[3] * R[7] - R[4] * R[6]);
            if (!(dev <= 1e-9) || !(det > 0.0)) {
                atomicOr(a.status, (int)PGX_ST_BA_ROT);
                known = false;
            }
        }
        a.fstate[f] = known ? (a.fixed[f] != 0 ? FS_FIXED : 0) : FS_UNKNOWN;
        for (int k = 0; k < 12; k++) a.cams[(size_t)f * 12 + k] = R[k];
        a.tv.inv[f] = -1;
    }
    for (int c = threadIdx.x; c < BA_MAX_FREE; c += blockDim.x) {
        a.cam_cnt[c] = 0;
        a.free_frame[c] = -1;
    }
    __syncthreads();
    build_slot_inverse(a.tv, a.status, PGX_ST_BA_DUP);
    __syncthreads();
    if (threadIdx.x == 0) {
        int n_free = 0, n_fixed = 0;
        for (int f = 0; f < a.tv.n_frames; f++) {
            const int st = a.fstate[f];
            if (st == FS_FIXED) n_fixed++;
            if (st >= 0) {
                if (n_free < BA_MAX_FREE) a.free_frame[n_free] = f;
                a.fstate[f] = n_free < BA_MAX_FREE ? n_free : FS_UNKNOWN;   // beyond 128: no iteration runs anyway
                n_free++;
            }
        }
        int err = 0;
        if (n_free > BA_MAX_FREE) {
            atomicOr(a.status, (int)PGX_ST_BA_FREE);
            err = 1;
        }
        if (n_fixed == 0) {
            atomicOr(a.status, (int)PGX_ST_BA_NOFIX);
            err = 1;
        }
        const int nt = clamp_tracks(a.tv, a.status, PGX_ST_BA_CAP);
        BaCtrl *c = a.ctrl;
        c->lam = a.lambda0;
        c->C = 0.0;
        c->cam_dx2 = 0.0;
        c->cam_x2 = 0.0;
        c->it = 0;
        c->acc = 0;
        c->reason = 0;
        c->done = 0;
        c->relin = 0;
        c->sel = 0;
        c->pdfail = 0;
        c->nonpd = 0;
        c->n_free = n_free;
        c->n_fixed = n_fixed;
        c->err = err;
        c->nt = nt;
        c->n_part = 0;
        c->n_used = 0;
        c->zneg = 0;
        c->pad = 0;
    }
}

__global__ __launch_bounds__(BA_NT) void k_ba_setup(BaArgs a)
{
    const long long nt = a.ctrl->nt;
    const int err = a.ctrl->err;
    PGX_TRACK_LOOP(BA_G, nt)
    {
        int o0, n;
        if (!track_range(a.tv, t, o0, n) && lane == 0) atomicOr(a.status, (int)PGX_ST_BA_NODE);
        int used = 0, bad = 0, dup = 0;
        for (int i = lane; i < n; i += BA_G) {
            const long long o = (long long)o0 + i;
            const int f = a.tv.nodes[2 * o], k = a.tv.nodes[2 * o + 1];
            if (!node_ok(a.tv, f, k)) {
                bad = 1;
                continue;
            }
            used += a.fstate[f] != FS_UNKNOWN;
            for (int j = 0; j < i; j++)   // two nodes in one frame: the track does not take part
                if (a.tv.nodes[2 * ((long long)o0 + j)] == f) dup = 1;
        }
        used = gsum_i<BA_G>(used);
        const int b1 = gsum_i<BA_G>(bad), b2 = gsum_i<BA_G>(dup);
        if ((b1 || b2) && lane == 0) atomicOr(a.status, (int)PGX_ST_BA_NODE);
        const double x0 = a.xyz_in[3 * t], x1 = a.xyz_in[3 * t + 1], x2 = a.xyz_in[3 * t + 2];
        const bool takes = !err && (!a.track_flags || a.track_flags[t] == 0) && isfinite(x0) && isfinite(x1) && isfinite(x2) &&
                           used >= 2 && b2 == 0;
        for (int i = lane; i < n; i += BA_G) {
            const long long o = (long long)o0 + i;
            const int f = a.tv.nodes[2 * o], k = a.tv.nodes[2 * o + 1];
            int c = -2;
            if (takes && node_ok(a.tv, f, k) && a.fstate[f] != FS_UNKNOWN) {
                c = a.fstate[f] >= 0 ? a.fstate[f] : -1;
                if (c >= 0) atomicAdd(&a.cam_cnt[c], 1);
            }
            a.ncf[o] = c;
        }
        if (lane == 0) {
            a.X[3 * t] = x0;
            a.X[3 * t + 1] = x1;
            a.X[3 * t + 2] = x2;
            a.part[t] = takes ? used : 0;
            if (takes) {
                atomicAdd(&a.ctrl->n_part, 1);
                atomicAdd(&a.ctrl->n_used, used);
            }
        }
    }
}

// one workgroup per free camera: its observations (node, track) in track order
__global__ __launch_bounds__(BA_NT) void k_ba_csr(BaArgs a)
{
    __shared__ int s_wave[BA_NT / 64 + 1];
    __shared__ int s_base;
    const int cam = blockIdx.x;
    if (a.ctrl->err || cam >= a.ctrl->n_free) return;
    const int nt = a.ctrl->nt;
    if (threadIdx.x == 0) {
        long long st = 0, tot = 0;
        for (int b = 0; b < a.ctrl->n_free; b++) {
            if (b < cam) st += a.cam_cnt[b];
            tot += a.cam_cnt[b];
        }
        a.csr_off[cam] = (int)st;
        s_base = tot > a.tv.node_cap ? -1 : (int)st;   // overlapping node ranges (malformed offsets): k_ba_start stops the call
    }
    __syncthreads();
    if (s_base < 0) return;
    const int wave = threadIdx.x >> 6, ln = threadIdx.x & 63;
    for (int base = 0; base < nt; base += BA_NT) {
        const int t = base + threadIdx.x;
        int node = -1;
        if (t < nt && a.part[t] > 0) {
            int o0, n;
            track_range(a.tv, t, o0, n);
            for (int i = 0; i < n; i++)
                if (a.ncf[(long long)o0 + i] == cam) node = o0 + i;
        }
        const unsigned long long m = __ballot(node >= 0);
        if (ln == 0) s_wave[wave] = __popcll(m);
        __syncthreads();
        int pos = s_base;
        for (int w = 0; w < wave; w++) pos += s_wave[w];
        pos += __popcll(m & ((1ull << ln) - 1ull));
        if (node >= 0) {
            a.csr_node[pos] = node;
            a.csr_track[pos] = t;
        }
        __syncthreads();
        if (threadIdx.x == 0) {
            int tot = 0;
            for (int w = 0; w < BA_NT / 64; w++) tot += s_wave[w];
            s_base += tot;
        }
        __syncthreads();
    }
}

// ---- per iteration ---------------------------------------------------------------------------------------------------

// linearisation at the current state (before the first iteration: always; afterwards: after an accepted step)
__global__ __launch_bounds__(BA_NT) void k_ba_lin(BaArgs a, int first)
{
    const BaCtrl *c = a.ctrl;
    if (!first && (c->done || !c->relin)) return;
    const long long nt = c->nt;
    const int sel = c->sel;
    const double *cams = a.cams + (size_t)sel * a.tv.n_frames * 12;
    const double *Xs = a.X + (size_t)sel * a.tv.max_tracks * 3;
    PGX_TRACK_LOOP(BA_G, nt)
    {
        if (a.part[t] == 0) {
            if (lane == 0) a.tcost[t] = 0.0;
            continue;
        }
        int o0, n;
        track_range(a.tv, t, o0, n);
        const double X[3] = {Xs[3 * t], Xs[3 * t + 1], Xs[3 * t + 2]};
        double v[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0}, gv[3] = {0.0, 0.0, 0.0}, cost = 0.0;
        for (int i = lane; i < n; i += BA_G) {
            const long long o = (long long)o0 + i;
            const int cf = a.ncf[o];
            if (cf == -2) continue;
            int f;
            double ku, kv;
            node_kp(a, o, f, ku, kv);
            Obs ob;
            observe(cams + (size_t)f * 12, a.K + (size_t)f * 4, X, ku, kv, ob);
            double rho, w;
            huber(ob.ru * ob.ru + ob.rv * ob.rv, a.huber, rho, w);
            cost += rho;
            int e = 0;
#pragma unroll
            for (int j = 0; j < 3; j++)
#pragma unroll
                for (int k = j; k < 3; k++, e++) v[e] += w * (ob.jp[0][j] * ob.jp[0][k] + ob.jp[1][j] * ob.jp[1][k]);
#pragma unroll
            for (int j = 0; j < 3; j++) gv[j] += w * (ob.jp[0][j] * ob.ru + ob.jp[1][j] * ob.rv);
            if (cf >= 0) {
                double *d = a.nd + o * BA_ND;
#pragma unroll
                for (int k = 0; k < 6; k++) {
                    d[k] = ob.jc[0][k];
                    d[6 + k] = ob.jc[1][k];
                }
#pragma unroll
                for (int k = 0; k < 3; k++) {
                    d[12 + k] = ob.jp[0][k];
                    d[15 + k] = ob.jp[1][k];
                }
                d[18] = ob.ru;
                d[19] = ob.rv;
                d[20] = w;
            }
        }
#pragma unroll
        for (int k = 0; k < 6; k++) v[k] = gsum<BA_G>(v[k]);
#pragma unroll
        for (int k = 0; k < 3; k++) gv[k] = gsum<BA_G>(gv[k]);
        cost = gsum<BA_G>(cost);
        if (lane == 0) {
#pragma unroll
            for (int k = 0; k < 6; k++) a.V[6 * t + k] = v[k];
#pragma unroll
            for (int k = 0; k < 3; k++) a.g[3 * t + k] = gv[k];
            a.tcost[t] = cost;
        }
    }
}

// the start: C0, trace[0] and the rest of the trace NaN, the stop test before any step
__global__ __launch_bounds__(BA_RED) void k_ba_start(BaArgs a)
{
    __shared__ double sh[BA_RED];
    BaCtrl *c = a.ctrl;
    const int nt = c->nt;
    double s = 0.0;
    for (int t = threadIdx.x; t < nt; t += BA_RED) s += a.tcost[t];
    const double C = block_sum(s, sh);
    const double NaN = __builtin_nan("");
    for (int i = threadIdx.x; i <= a.max_iters; i += BA_RED) {
        a.trace[2 * i] = i == 0 ? C : NaN;
        a.trace[2 * i + 1] = i == 0 ? c->lam : NaN;
    }
    if (threadIdx.x == 0) {
        long long tot = 0;
        for (int b = 0; b < c->n_free && b < BA_MAX_FREE; b++) tot += a.cam_cnt[b];
        if (tot > a.tv.node_cap) {
            atomicOr(a.status, (int)PGX_ST_BA_NODE);
            c->err = 1;
        }
        c->C = C;
        int reason = 0;
        if (c->err || c->n_part == 0) reason = 0;
        else if (C == 0.0) reason = 2;
        else if (c->lam > 1e16) reason = 4;
        else if (a.max_iters == 0) reason = 1;
        else reason = -1;
        c->reason = reason < 0 ? 0 : reason;
        c->done = reason >= 0;
    }
}

__global__ __launch_bounds__(BA_NT) void k_ba_vinv(BaArgs a)
{
    BaCtrl *c = a.ctrl;
    if (c->done) return;
    const int nt = c->nt;
    const double lam = c->lam;
    for (int t = blockIdx.x * blockDim.x + threadIdx.x; t < nt; t += gridDim.x * blockDim.x) {
        if (a.part[t] == 0) continue;
        const double *v = a.V + 6 * (size_t)t;   // (00, 01, 02, 11, 12, 22)
        const double a00 = v[0] + lam * fmin(fmax(v[0], 1e-6), 1e32), a11 = v[3] + lam * fmin(fmax(v[3], 1e-6), 1e32);
        const double a22 = v[5] + lam * fmin(fmax(v[5], 1e-6), 1e32), a01 = v[1], a02 = v[2], a12 = v[4];
        // Cholesky pivots: all > 0 <=> positive definite
        const double l00 = sqrt(a00);
        const double l10 = a01 / l00, l20 = a02 / l00;
        const double d1 = a11 - l10 * l10;
        const double l11 = sqrt(d1);
        const double l21 = (a12 - l20 * l10) / l11;
        const double d2 = (a22 - l20 * l20) - l21 * l21;
        if (!(a00 > 0.0) || !(d1 > 0.0) || !(d2 > 0.0)) {
            atomicOr(&c->pdfail, 1);
            continue;
        }
        const double c00 = a11 * a22 - a12 * a12, c01 = a02 * a12 - a01 * a22, c02 = a01 * a12 - a02 * a11;
        const double c11 = a00 * a22 - a02 * a02, c12 = a01 * a02 - a00 * a12, c22 = a00 * a11 - a01 * a01;
        const double det = (a00 * c00 + a01 * c01) + a02 * c02;
        double *o = a.Vi + 6 * (size_t)t;
        o[0] = c00 / det;
        o[1] = c01 / det;
        o[2] = c02 / det;
        o[3] = c11 / det;
        o[4] = c12 / det;
        o[5] = c22 / det;
    }
}

// y = Vi x for the packed symmetric 3x3 Vi
__device__ __forceinline__ void sym3(const double *m, const double *x, double *y)
{
    y[0] = (m[0] * x[0] + m[1] * x[1]) + m[2] * x[2];
    y[1] = (m[1] * x[0] + m[3] * x[1]) + m[4] * x[2];
    y[2] = (m[2] * x[0] + m[4] * x[1]) + m[5] * x[2];
}

// W = w Jc^T Jp (6 x 3) of node data d
__device__ __forceinline__ void w_block(const double *d, double (&W)[6][3])
{
    const double w = d[20];
#pragma unroll
    for (int r = 0; r < 6; r++)
#pragma unroll
        for (int k = 0; k < 3; k++) W[r][k] = w * (d[r] * d[12 + k] + d[6 + r] * d[15 + k]);
}

// one workgroup per free camera a: S_ab for b <= a (thread b), the right-hand side (thread BA_MAX_FREE)
__global__ __launch_bounds__(BA_NT) void k_ba_schur(BaArgs a)
{
    __shared__ int s_tab[BA_CH][BA_MAX_FREE];
    __shared__ double s_Y[BA_CH][18];
    __shared__ double s_Yg[BA_CH][6];
    __shared__ int s_node[BA_CH];
    const BaCtrl *c = a.ctrl;
    const int cam = blockIdx.x;
    if (c->done || c->pdfail || cam >= c->n_free) return;
    const int nf = c->n_free;
    const double lam = c->lam;
    const int beg = a.csr_off[cam], len = a.cam_cnt[cam];
    const int tid = threadIdx.x, b = tid;
    const bool owner = b <= cam;   // thread b < BA_MAX_FREE owns block (cam, b)
    double acc[36], ud[6], rh[6];
#pragma unroll
    for (int k = 0; k < 36; k++) acc[k] = 0.0;
#pragma unroll
    for (int k = 0; k < 6; k++) {
        ud[k] = 0.0;
        rh[k] = 0.0;
    }
    for (int base = 0; base < len; base += BA_CH) {
        const int nch = len - base < BA_CH ? len - base : BA_CH;
        for (int i = tid; i < BA_CH * BA_MAX_FREE; i += BA_NT) (&s_tab[0][0])[i] = -1;
        __syncthreads();
        // the chunk's tracks: every free node into s_tab (one wave per track); Y = W_a Vi and Y g_t (one thread per track)
        for (int k = tid >> 6; k < nch; k += BA_NT / 64) {
            const int t = a.csr_track[beg + base + k];
            int o0, n;
            track_range(a.tv, t, o0, n);
            for (int i = tid & 63; i < n; i += 64) {
                const int cf = a.ncf[(long long)o0 + i];
                if (cf >= 0) s_tab[k][cf] = o0 + i;
            }
        }
        if (tid < nch) {
            const int k = tid, t = a.csr_track[beg + base + k], o = a.csr_node[beg + base + k];
            s_node[k] = o;
            double W[6][3];
            w_block(a.nd + (size_t)o * BA_ND, W);
            const double *vi = a.Vi + 6 * (size_t)t, *gt = a.g + 3 * (size_t)t;
            for (int r = 0; r < 6; r++) {
                double y[3];
                sym3(vi, W[r], y);
                s_Y[k][3 * r] = y[0];
                s_Y[k][3 * r + 1] = y[1];
                s_Y[k][3 * r + 2] = y[2];
                s_Yg[k][r] = (y[0] * gt[0] + y[1] * gt[1]) + y[2] * gt[2];
            }
        }
        __syncthreads();
        if (b < BA_MAX_FREE && owner) {
            for (int k = 0; k < nch; k++) {
                const int o = s_tab[k][b];
                if (o < 0) continue;
                const double *d = a.nd + (size_t)o * BA_ND;
                double W[6][3];
                w_block(d, W);
#pragma unroll
                for (int r = 0; r < 6; r++)
#pragma unroll
                    for (int q = 0; q < 6; q++)
                        acc[6 * r + q] -= (s_Y[k][3 * r] * W[q][0] + s_Y[k][3 * r + 1] * W[q][1]) + s_Y[k][3 * r + 2] * W[q][2];
                if (b == cam) {
                    const double w = d[20];
#pragma unroll
                    for (int r = 0; r < 6; r++)
#pragma unroll
                        for (int q = 0; q < 6; q++) {
                            const double u = w * (d[r] * d[q] + d[6 + r] * d[6 + q]);
                            acc[6 * r + q] += u;
                            if (r == q) ud[r] += u;
                        }
                }
            }
        } else if (b == BA_MAX_FREE) {
            for (int k = 0; k < nch; k++) {
                const double *d = a.nd + (size_t)s_node[k] * BA_ND;
                const double w = d[20];
#pragma unroll
                for (int r = 0; r < 6; r++) rh[r] += s_Yg[k][r] - w * (d[r] * d[18] + d[6 + r] * d[19]);
            }
        }
        __syncthreads();
    }
    if (b < nf && owner) {
        double *S = a.S + (size_t)(6 * cam) * BA_LD + 6 * b;
#pragma unroll
        for (int r = 0; r < 6; r++)
#pragma unroll
            for (int q = 0; q < 6; q++) {
                double v = acc[6 * r + q];
                if (b == cam && r == q) v += lam * fmin(fmax(ud[r], 1e-6), 1e32);
                S[(size_t)r * BA_LD + q] = v;
            }
    } else if (b == BA_MAX_FREE) {
#pragma unroll
        for (int r = 0; r < 6; r++) a.rhs[6 * cam + r] = rh[r];
    }
}

// one workgroup: blocked Cholesky of the lower triangle of S in place, L L^T dc = rhs, the trial cameras
__global__ __launch_bounds__(BA_RED) void k_ba_solve(BaArgs a)
{
    __shared__ double s_b[BA_LD];
    __shared__ int s_fail;
    BaCtrl *c = a.ctrl;
    if (c->done || c->pdfail) return;
    const int nf = c->n_free, n = 6 * nf, tid = threadIdx.x;
    double *S = a.S;
    if (tid == 0) s_fail = 0;
    for (int i = tid; i < n; i += BA_RED) s_b[i] = a.rhs[i];
    __syncthreads();
    for (int kb = 0; kb < nf; kb++) {
        const int k0 = 6 * kb;
        if (tid == 0) {
            for (int j = 0; j < 6; j++) {
                double d = S[(size_t)(k0 + j) * BA_LD + k0 + j];
                for (int m = 0; m < j; m++) d -= S[(size_t)(k0 + j) * BA_LD + k0 + m] * S[(size_t)(k0 + j) * BA_LD + k0 + m];
                if (!(d > 0.0)) {
                    s_fail = 1;
                    break;
                }
                const double l = sqrt(d);
                S[(size_t)(k0 + j) * BA_LD + k0 + j] = l;
                for (int i = j + 1; i < 6; i++) {
                    double e = S[(size_t)(k0 + i) * BA_LD + k0 + j];
                    for (int m = 0; m < j; m++) e -= S[(size_t)(k0 + i) * BA_LD + k0 + m] * S[(size_t)(k0 + j) * BA_LD + k0 + m];
                    S[(size_t)(k0 + i) * BA_LD + k0 + j] = e / l;
                }
            }
        }
        __syncthreads();
        if (s_fail) break;
        // panel: rows below the block
        for (int i = k0 + 6 + tid; i < n; i += BA_RED) {
            double *Li = S + (size_t)i * BA_LD + k0;
            for (int j = 0; j < 6; j++) {
                const double *Lj = S + (size_t)(k0 + j) * BA_LD + k0;
                double e = Li[j];
                for (int m = 0; m < j; m++) e -= Li[m] * Lj[m];
                Li[j] = e / Lj[j];
            }
        }
        __syncthreads();
        // trailing update of the lower triangle
        const int k1 = k0 + 6;
        for (int i = k1 + (tid >> 5); i < n; i += BA_RED / 32) {
            const double *Li = S + (size_t)i * BA_LD + k0;
            const double li[6] = {Li[0], Li[1], Li[2], Li[3], Li[4], Li[5]};
            for (int j = k1 + (tid & 31); j <= i; j += 32) {
                const double *Lj = S + (size_t)j * BA_LD + k0;
                double s = 0.0;
#pragma unroll
                for (int m = 0; m < 6; m++) s += li[m] * Lj[m];
                S[(size_t)i * BA_LD + j] -= s;
            }
        }
        __syncthreads();
    }
    if (s_fail) {
        if (tid == 0) c->pdfail = 1;
        return;
    }
    // L y = rhs
    for (int kb = 0; kb < nf; kb++) {
        const int k0 = 6 * kb;
        if (tid == 0)
            for (int j = 0; j < 6; j++) {
                double e = s_b[k0 + j];
                for (int m = 0; m < j; m++) e -= S[(size_t)(k0 + j) * BA_LD + k0 + m] * s_b[k0 + m];
                s_b[k0 + j] = e / S[(size_t)(k0 + j) * BA_LD + k0 + j];
            }
        __syncthreads();
        for (int i = k0 + 6 + tid; i < n; i += BA_RED) {
            const double *Li = S + (size_t)i * BA_LD + k0;
            double s = 0.0;
#pragma unroll
            for (int m = 0; m < 6; m++) s += Li[m] * s_b[k0 + m];
            s_b[i] -= s;
        }
        __syncthreads();
    }
    // L^T dc = y
    for (int kb = nf - 1; kb >= 0; kb--) {
        const int k0 = 6 * kb;
        if (tid == 0)
            for (int j = 5; j >= 0; j--) {
                double e = s_b[k0 + j];
                for (int m = j + 1; m < 6; m++) e -= S[(size_t)(k0 + m) * BA_LD + k0 + j] * s_b[k0 + m];
                s_b[k0 + j] = e / S[(size_t)(k0 + j) * BA_LD + k0 + j];
            }
        __syncthreads();
        for (int i = tid; i < k0; i += BA_RED) {
            double s = 0.0;
#pragma unroll
            for (int m = 0; m < 6; m++) s += S[(size_t)(k0 + m) * BA_LD + i] * s_b[k0 + m];
            s_b[i] -= s;
        }
        __syncthreads();
    }
    for (int i = tid; i < n; i += BA_RED) a.dc[i] = s_b[i];
    const int sel = c->sel;
    const double *cur = a.cams + (size_t)sel * a.tv.n_frames * 12;
    double *trial = a.cams + (size_t)(1 - sel) * a.tv.n_frames * 12;
    for (int f = tid; f < a.tv.n_frames; f += BA_RED) {
        const int st = a.fstate[f];
        const double *R = cur + (size_t)f * 12;
        double *T = trial + (size_t)f * 12;
        if (st >= 0) {
            rotate_left(s_b + 6 * st, R, T);
            for (int k = 0; k < 3; k++) T[9 + k] = R[9 + k] + s_b[6 * st + 3 + k];
        } else {
            for (int k = 0; k < 12; k++) T[k] = R[k];
        }
    }
    if (tid == 0) {
        double dx2 = 0.0, x2 = 0.0;
        for (int i = 0; i < n; i++) dx2 += s_b[i] * s_b[i];
        for (int cf = 0; cf < nf; cf++) {
            const double *R = cur + (size_t)a.free_frame[cf] * 12;
            x2 += (R[9] * R[9] + R[10] * R[10]) + R[11] * R[11];
        }
        c->cam_dx2 = dx2;
        c->cam_x2 = x2;
    }
}

// back-substitution, the trial point and the trial cost per track
__global__ __launch_bounds__(BA_NT) void k_ba_back(BaArgs a)
{
    const BaCtrl *c = a.ctrl;
    if (c->done || c->pdfail) return;
    const long long nt = c->nt;
    const int sel = c->sel;
    const double *Xs = a.X + (size_t)sel * a.tv.max_tracks * 3;
    double *Xt = a.X + (size_t)(1 - sel) * a.tv.max_tracks * 3;
    const double *trial = a.cams + (size_t)(1 - sel) * a.tv.n_frames * 12;
    PGX_TRACK_LOOP(BA_G, nt)
    {
        if (a.part[t] == 0) {
            if (lane == 0) {
                a.tcost[t] = 0.0;
                a.tdx[t] = 0.0;
                a.tx[t] = 0.0;
            }
            continue;
        }
        int o0, n;
        track_range(a.tv, t, o0, n);
        // sum over free nodes of W_a^T dc_a = w Jp^T (Jc dc_a)
        double s[3] = {0.0, 0.0, 0.0};
        for (int i = lane; i < n; i += BA_G) {
            const long long o = (long long)o0 + i;
            const int cf = a.ncf[o];
            if (cf < 0) continue;
            const double *d = a.nd + o * BA_ND, *dc = a.dc + 6 * cf;
            double e0 = 0.0, e1 = 0.0;
#pragma unroll
            for (int k = 0; k < 6; k++) {
                e0 += d[k] * dc[k];
                e1 += d[6 + k] * dc[k];
            }
            const double w = d[20];
#pragma unroll
            for (int k = 0; k < 3; k++) s[k] += w * (d[12 + k] * e0 + d[15 + k] * e1);
        }
#pragma unroll
        for (int k = 0; k < 3; k++) s[k] = gsum<BA_G>(s[k]);
        const double *gt = a.g + 3 * (size_t)t;
        const double r[3] = {-gt[0] - s[0], -gt[1] - s[1], -gt[2] - s[2]};
        double dX[3];
        sym3(a.Vi + 6 * (size_t)t, r, dX);
        const double X[3] = {Xs[3 * t] + dX[0], Xs[3 * t + 1] + dX[1], Xs[3 * t + 2] + dX[2]};
        double cost = 0.0;
        for (int i = lane; i < n; i += BA_G) {
            const long long o = (long long)o0 + i;
            if (a.ncf[o] == -2) continue;
            int f;
            double ku, kv, ru, rv, z, rho, w;
            node_kp(a, o, f, ku, kv);
            projection_only(trial + (size_t)f * 12, a.K + (size_t)f * 4, X, ku, kv, ru, rv, z);
            huber(ru * ru + rv * rv, a.huber, rho, w);
            cost += rho;
        }
        cost = gsum<BA_G>(cost);
        if (lane == 0) {
            Xt[3 * t] = X[0];
            Xt[3 * t + 1] = X[1];
            Xt[3 * t + 2] = X[2];
            a.tcost[t] = cost;
            a.tdx[t] = (dX[0] * dX[0] + dX[1] * dX[1]) + dX[2] * dX[2];
            a.tx[t] = (Xs[3 * t] * Xs[3 * t] + Xs[3 * t + 1] * Xs[3 * t + 1]) + Xs[3 * t + 2] * Xs[3 * t + 2];
        }
    }
}

__global__ __launch_bounds__(BA_RED) void k_ba_decide(BaArgs a)
{
    __shared__ double sh[BA_RED];
    BaCtrl *c = a.ctrl;
    if (c->done) return;   // uniform: every thread reads the same word before anyone writes it
    const int nt = c->nt, pdfail = c->pdfail;
    double cn = 0.0, dx2 = 0.0, x2 = 0.0;
    if (!pdfail) {
        double s0 = 0.0, s1 = 0.0, s2 = 0.0;
        for (int t = threadIdx.x; t < nt; t += BA_RED) {
            s0 += a.tcost[t];
            s1 += a.tdx[t];
            s2 += a.tx[t];
        }
        cn = block_sum(s0, sh);
        dx2 = block_sum(s1, sh);
        x2 = block_sum(s2, sh);
    }
    if (threadIdx.x != 0) return;
    const int it = c->it + 1;
    double C = c->C, lam = c->lam;
    int reason = -1, accepted = 0;
    if (pdfail) {
        c->nonpd++;
        lam = lam * 10.0;
    } else if (sqrt(c->cam_dx2 + dx2) <= 1e-12 * (1.0 + sqrt(c->cam_x2 + x2))) {
        reason = 3;
    } else if (cn < C) {
        accepted = 1;
        const double dec = C - cn;
        const bool small = dec <= 1e-12 * C;
        C = cn;
        lam = fmax(lam / 10.0, 1e-12);
        c->acc++;
        c->sel = 1 - c->sel;
        if (small || C == 0.0) reason = 2;
    } else {
        lam = lam * 10.0;
    }
    if (reason < 0) {
        if (lam > 1e16) reason = 4;
        else if (it >= a.max_iters) reason = 1;
    }
    c->it = it;
    c->C = C;
    c->lam = lam;
    c->relin = accepted;
    c->pdfail = 0;
    a.trace[2 * it] = C;
    a.trace[2 * it + 1] = lam;
    if (reason >= 0) {
        c->reason = reason;
        c->done = 1;
    }
}

// ---- outputs -----------------------------------------------------------------------------------------------------------

__global__ __launch_bounds__(BA_NT) void k_ba_final(BaArgs a)
{
    const BaCtrl *c = a.ctrl;
    const long long nt = c->nt;
    const int sel = c->sel;
    const double *cams = a.cams + (size_t)sel * a.tv.n_frames * 12;
    const double *Xs = a.X + (size_t)sel * a.tv.max_tracks * 3;
    const double NaN = __builtin_nan("");
    PGX_TRACK_LOOP(BA_G, nt)
    {
        int o0, n;
        track_range(a.tv, t, o0, n);
        const bool takes = a.part[t] > 0;
        double X[3];
#pragma unroll
        for (int k = 0; k < 3; k++) X[k] = takes ? Xs[3 * t + k] : a.xyz_in[3 * t + k];
        int zneg = 0;
        for (int i = lane; i < n; i += BA_G) {
            const long long o = (long long)o0 + i;
            double e = NaN;
            if (takes && a.ncf[o] != -2) {
                int f;
                double ku, kv, ru, rv, z;
                node_kp(a, o, f, ku, kv);
                projection_only(cams + (size_t)f * 12, a.K + (size_t)f * 4, X, ku, kv, ru, rv, z);
                e = sqrt(ru * ru + rv * rv);
                zneg += !(z > 0.0);
            }
            if (a.node_err) a.node_err[o] = e;
        }
        zneg = gsum_i<BA_G>(zneg);
        if (lane == 0) {
#pragma unroll
            for (int k = 0; k < 3; k++) a.xyz_out[3 * t + k] = X[k];
            if (zneg) atomicAdd(&a.ctrl->zneg, zneg);
        }
    }
}

__global__ __launch_bounds__(BA_NT) void k_ba_out(BaArgs a)
{
    const BaCtrl *c = a.ctrl;
    const double *cams = a.cams + (size_t)c->sel * a.tv.n_frames * 12;
    for (int f = threadIdx.x; f < a.tv.n_frames; f += blockDim.x) {
        const double *R = cams + (size_t)f * 12, *K = a.K + (size_t)f * 4;
        double *o = a.Rt_out + (size_t)f * 12, *P = a.P_out + (size_t)f * 12;
        const bool known = a.fstate[f] != FS_UNKNOWN;
        double r[12];
        for (int k = 0; k < 12; k++) r[k] = R[k];
        for (int k = 0; k < 12; k++) o[k] = r[k];
        camera_matrix(K, r, known, P);
    }
    if (threadIdx.x == 0) {
        a.report[0] = c->it;
        a.report[1] = c->acc;
        a.report[2] = c->reason;
        a.report[3] = c->n_free;
        a.report[4] = c->n_part;
        a.report[5] = c->n_used;
        a.report[6] = c->zneg;
        a.report[7] = c->nonpd;
    }
}

// the workspace, described once: a's workspace pointers (none valid for ws = nullptr) and the bytes
size_t ba_carve(BaArgs &a, void *ws)
{
    const int n_frames = a.tv.n_frames;
    const size_t T = (size_t)(a.tv.max_tracks > 0 ? a.tv.max_tracks : 1), N = (size_t)(a.tv.node_cap > 0 ? a.tv.node_cap : 1);
    WsCarver w(ws);
    a.ctrl = w.take<BaCtrl>(sizeof(BaCtrl));
    a.fstate = w.take<int32_t>((size_t)n_frames * 4);
    a.tv.inv = w.take<int32_t>((size_t)n_frames * 4);
    a.free_frame = w.take<int32_t>(BA_MAX_FREE * 4);
    a.cam_cnt = w.take<int32_t>(BA_MAX_FREE * 4);
    a.csr_off = w.take<int32_t>(BA_MAX_FREE * 4);
    a.cams = w.take<double>((size_t)2 * n_frames * 12 * 8);
    a.S = w.take<double>((size_t)BA_LD * BA_LD * 8);
    a.rhs = w.take<double>(BA_LD * 8);
    a.dc = w.take<double>(BA_LD * 8);
    a.X = w.take<double>(2 * T * 3 * 8);
    a.V = w.take<double>(T * 6 * 8);
    a.g = w.take<double>(T * 3 * 8);
    a.Vi = w.take<double>(T * 6 * 8);
    a.tcost = w.take<double>(T * 8);
    a.tdx = w.take<double>(T * 8);
    a.tx = w.take<double>(T * 8);
    a.part = w.take<int32_t>(T * 4);
    a.nd = w.take<double>(N * BA_ND * 8);
    a.ncf = w.take<int32_t>(N * 4);
    a.csr_node = w.take<int32_t>(N * 4);
    a.csr_track = w.take<int32_t>(N * 4);
    return w.total();
}

int track_grid(int max_tracks)
{
    const long long want = ((long long)max_tracks * BA_G + BA_NT - 1) / BA_NT;
    return (int)(want < 1 ? 1 : (want > BA_GRID_MAX ? BA_GRID_MAX : want));
}

} // namespace

size_t pgx_bundle_ws_bytes(const BaArgs &a)
{
    BaArgs b = a;
    return ba_carve(b, nullptr);
}

void pgx_launch_bundle(hipStream_t s, BaArgs a, void *ws)
{
    ba_carve(a, ws);
    const int grid = track_grid(a.tv.max_tracks);
    hipLaunchKernelGGL(k_ba_frames, dim3(1), dim3(BA_NT), 0, s, a);
    hipLaunchKernelGGL(k_ba_setup, dim3(grid), dim3(BA_NT), 0, s, a);
    hipLaunchKernelGGL(k_ba_csr, dim3(BA_MAX_FREE), dim3(BA_NT), 0, s, a);
    hipLaunchKernelGGL(k_ba_lin, dim3(grid), dim3(BA_NT), 0, s, a, 1);
    hipLaunchKernelGGL(k_ba_start, dim3(1), dim3(BA_RED), 0, s, a);
    for (int i = 0; i < a.max_iters; i++) {
        if (i > 0) hipLaunchKernelGGL(k_ba_lin, dim3(grid), dim3(BA_NT), 0, s, a, 0);
        hipLaunchKernelGGL(k_ba_vinv, dim3(grid), dim3(BA_NT), 0, s, a);
        hipLaunchKernelGGL(k_ba_schur, dim3(BA_MAX_FREE), dim3(BA_NT), 0, s, a);
        hipLaunchKernelGGL(k_ba_solve, dim3(1), dim3(BA_RED), 0, s, a);
        hipLaunchKernelGGL(k_ba_back, dim3(grid), dim3(BA_NT), 0, s, a);
        hipLaunchKernelGGL(k_ba_decide, dim3(1), dim3(BA_RED), 0, s, a);
    }
    hipLaunchKernelGGL(k_ba_final, dim3(grid), dim3(BA_NT), 0, s, a);
    hipLaunchKernelGGL(k_ba_out, dim3(1), dim3(BA_NT), 0, s, a);
}
