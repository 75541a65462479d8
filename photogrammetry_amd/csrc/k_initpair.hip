// k_initpair.hip -- the start of a reconstruction: relative pose per image pair from verification's F and the intrinsics,
// and the choice of the initial pair (pgx_init_pair_dev; include/pgx.h).
//
// Per image pair: E = K_a^T F K_b, its four (R, t) decompositions (cyclic Jacobi on G^T G, G = E^T), each scored on the pair's
// candidate matches by the sign of the two ray depths (front) and by the ray angle (wide), the winner by front count.  Over
// the pairs: the unflagged pair with the most wide points.  float64 throughout, no fused multiply-add (the library's
// -ffp-contract=off); every count is an integer, so neither the grid nor the order of the sums reaches a result.
//
// Kernels (all on the caller's stream):
//   k_init_setup   one thread per pair: the flags SKIPPED, BADINPUT and DEGENERATE, E, the decomposition, R1, R2 and t to the
//                  workspace with the two frames' intrinsics, the four candidates to d_cand_Rt, d_sigma, the counters zeroed
//   k_init_score   the hot path: ceil(stride / INIT_ROWS) workgroups per pair walk its match list; a lane takes an entry, gathers its two
//                  keypoints and scores it against R1 and R2 with t and -t at once (the products with -t are the exact
//                  negatives, so candidates 1 and 3 cost two comparisons); no division, no square root; ballots count per
//                  wave, one lane per wave adds its nine integers to the pair's counters (integer atomics: no order)
//   k_init_finish  one thread per pair: the winner, FEWFRONT and FEWPOINTS, d_Rt_pair, d_pair_stats
//   k_init_pick    one workgroup: the report, the choice (two integer keys: the wide count then the smaller frame of a,
//                  and the smaller frame of b then the smaller m), the per-frame arrays
// DESIGN.md section 21 has the measurements.
#include "pgx_stage_args.h"
#include "pgx_eig.h"

namespace {

constexpr int INIT_NT = 256;   // threads per workgroup of every kernel here
static_assert(INIT_NT == 256, "block_sum_i (pgx_trackgraph.h) adds up four waves");
constexpr int INIT_ROWS = 2048;   // list entries per scoring workgroup before a pair gets another one
constexpr int INIT_WS_D = 32;     // doubles per pair: R1 [9], R2 [9], t [3], K_a [4], K_b [4], 3 spare
constexpr int INIT_WS_I = 12;     // ints per pair: flags, frame of a, frame of b, n, front [4], wide [4]

__device__ __forceinline__ double dot3(double a0, double a1, double a2, double b0, double b1, double b2)
{
    return (a0 * b0 + a1 * b1) + a2 * b2;
}

// column 0 (w0), 1 (w1) or 2 of V by selections: no run-time index, so V stays in registers
__device__ __forceinline__ void pick_col(const double (&V)[3][3], bool w0, bool w1, double (&v)[3])
{
#pragma unroll
    for (int i = 0; i < 3; i++) v[i] = w0 ? V[i][0] : (w1 ? V[i][1] : V[i][2]);
}

// ---- kernels -------------------------------------------------------------------------------------------------------

__global__ __launch_bounds__(INIT_NT) void k_init_setup(InitArgs a)
{
    const int m = blockIdx.x * INIT_NT + threadIdx.x;
    if (m >= a.M) return;
    const double NaN = __builtin_nan("");
    const int sa = a.pairlist[2 * (size_t)m], sb = a.pairlist[2 * (size_t)m + 1];
    int flags = 0, fa = -1, fb = -1;
    if (sa < 0 || sa >= a.nslots || sb < 0 || sb >= a.nslots || sa == sb) {
        flags = PGX_INIT_SKIPPED;
    } else {
        fa = a.frame_ids ? a.frame_ids[sa] : sa;
        fb = a.frame_ids ? a.frame_ids[sb] : sb;
        if (fa < 0 || fa >= a.n_frames || fb < 0 || fb >= a.n_frames) flags = PGX_INIT_SKIPPED;
    }
    double Fm[9], Ka[4], Kb[4];
#pragma unroll
    for (int k = 0; k < 9; k++) Fm[k] = a.F[(size_t)m * 9 + k];
#pragma unroll
    for (int k = 0; k < 4; k++) {
        Ka[k] = flags ? NaN : a.K[(size_t)fa * 4 + k];
        Kb[k] = flags ? NaN : a.K[(size_t)fb * 4 + k];
    }
    if (!flags) {
        bool ok = Ka[0] != 0.0 && Ka[1] != 0.0 && Kb[0] != 0.0 && Kb[1] != 0.0;
#pragma unroll
        for (int k = 0; k < 9; k++) ok = ok && isfinite(Fm[k]);
#pragma unroll
        for (int k = 0; k < 4; k++) ok = ok && isfinite(Ka[k]) && isfinite(Kb[k]);
        if (!ok) flags = PGX_INIT_BADINPUT;
    }
    double R1[9], R2[9], t[3], sig = NaN;
#pragma unroll
    for (int k = 0; k < 9; k++) R1[k] = R2[k] = NaN;
    t[0] = t[1] = t[2] = NaN;
    if (!flags) {
        // A = K_a^T F, E = A K_b, G = E^T
        double A[9], E[9], G[3][3];
#pragma unroll
        for (int j = 0; j < 3; j++) {
            A[j] = Ka[0] * Fm[j];
            A[3 + j] = Ka[1] * Fm[3 + j];
            A[6 + j] = (Ka[2] * Fm[j] + Ka[3] * Fm[3 + j]) + Fm[6 + j];
        }
#pragma unroll
        for (int i = 0; i < 3; i++) {
            E[3 * i] = A[3 * i] * Kb[0];
            E[3 * i + 1] = A[3 * i + 1] * Kb[1];
            E[3 * i + 2] = (A[3 * i] * Kb[2] + A[3 * i + 1] * Kb[3]) + A[3 * i + 2];
        }
        double nn = 0.0;
#pragma unroll
        for (int i = 0; i < 3; i++)
#pragma unroll
            for (int j = 0; j < 3; j++) {
                G[i][j] = E[3 * j + i];
                nn += G[i][j] * G[i][j];
            }
        const double nr = sqrt(nn);
        bool ok = true;
#pragma unroll
        for (int i = 0; i < 3; i++)
#pragma unroll
            for (int j = 0; j < 3; j++) {
                G[i][j] = G[i][j] / nr;
                ok = ok && isfinite(G[i][j]);
            }
        double B[3][3], V[3][3];
#pragma unroll
        for (int i = 0; i < 3; i++)
#pragma unroll
            for (int j = 0; j < 3; j++) B[i][j] = ok ? dot3(G[0][i], G[1][i], G[2][i], G[0][j], G[1][j], G[2][j]) : (i == j ? 1.0 : 0.0);
        jacobi_eig<3>(B, V);
        const double l0 = B[0][0], l1 = B[1][1], l2 = B[2][2];
        // rank by eigenvalue descending, ties to the lower column
        const int r0 = (l1 > l0) + (l2 > l0), r1 = (l0 >= l1) + (l2 > l1);   // column 2 is what the two leave
        double v1[3], v2[3];
        pick_col(V, r0 == 0, r1 == 0, v1);
        pick_col(V, r0 == 1, r1 == 1, v2);
        const double la = r0 == 0 ? l0 : (r1 == 0 ? l1 : l2), lb = r0 == 1 ? l0 : (r1 == 1 ? l1 : l2);
        const double s1 = sqrt(la > 0.0 ? la : 0.0), s2 = sqrt(lb > 0.0 ? lb : 0.0);
        ok = ok && isfinite(la) && isfinite(lb) && isfinite(l0) && isfinite(l1) && isfinite(l2);
        sig = ok ? s2 / s1 : NaN;
        ok = ok && s2 > 1e-6 * s1;
        double u1[3], u2[3], w[3];
#pragma unroll
        for (int i = 0; i < 3; i++) {
            u1[i] = dot3(G[i][0], G[i][1], G[i][2], v1[0], v1[1], v1[2]) / s1;
            w[i] = dot3(G[i][0], G[i][1], G[i][2], v2[0], v2[1], v2[2]);
        }
        const double pr = dot3(u1[0], u1[1], u1[2], w[0], w[1], w[2]);
#pragma unroll
        for (int i = 0; i < 3; i++) w[i] = w[i] - pr * u1[i];
        const double wn = sqrt(dot3(w[0], w[1], w[2], w[0], w[1], w[2]));
#pragma unroll
        for (int i = 0; i < 3; i++) u2[i] = w[i] / wn;
        const double v3[3] = {v1[1] * v2[2] - v1[2] * v2[1], v1[2] * v2[0] - v1[0] * v2[2], v1[0] * v2[1] - v1[1] * v2[0]};
        const double u3[3] = {u1[1] * u2[2] - u1[2] * u2[1], u1[2] * u2[0] - u1[0] * u2[2], u1[0] * u2[1] - u1[1] * u2[0]};
#pragma unroll
        for (int i = 0; i < 3; i++) {
#pragma unroll
            for (int j = 0; j < 3; j++) {
                R1[3 * i + j] = (u2[i] * v1[j] - u1[i] * v2[j]) + u3[i] * v3[j];
                R2[3 * i + j] = (u1[i] * v2[j] - u2[i] * v1[j]) + u3[i] * v3[j];
                ok = ok && isfinite(R1[3 * i + j]) && isfinite(R2[3 * i + j]);
            }
            t[i] = u3[i];
            ok = ok && isfinite(t[i]);
        }
        if (!ok) {
            flags = PGX_INIT_DEGENERATE;
#pragma unroll
            for (int k = 0; k < 9; k++) R1[k] = R2[k] = NaN;
            t[0] = t[1] = t[2] = NaN;
        }
    }
    double *wd = a.wd + (size_t)m * INIT_WS_D;
#pragma unroll
    for (int k = 0; k < 9; k++) {
        wd[k] = R1[k];
        wd[9 + k] = R2[k];
    }
#pragma unroll
    for (int k = 0; k < 3; k++) wd[18 + k] = t[k];
#pragma unroll
    for (int k = 0; k < 4; k++) {
        wd[21 + k] = Ka[k];
        wd[25 + k] = Kb[k];
    }
    int32_t *wi = a.wi + (size_t)m * INIT_WS_I;
    wi[0] = flags;
    wi[1] = fa;
    wi[2] = fb;
#pragma unroll
    for (int k = 3; k < INIT_WS_I; k++) wi[k] = 0;
    if (a.sigma) a.sigma[m] = sig;
    if (a.cand_Rt) {
        double *o = a.cand_Rt + (size_t)m * 48;
#pragma unroll
        for (int k = 0; k < 9; k++) {
            o[k] = R1[k];
            o[12 + k] = R1[k];
            o[24 + k] = R2[k];
            o[36 + k] = R2[k];
        }
#pragma unroll
        for (int k = 0; k < 3; k++) {
            o[9 + k] = t[k];
            o[21 + k] = -t[k];
            o[33 + k] = t[k];
            o[45 + k] = -t[k];
        }
    }
}

// the score of one rotation on one match (include/pgx.h): fp, fm = front with t and with -t, wide = the ray angle test
__device__ __forceinline__ void score_rot(const double (&R)[9], double t0, double t1, double t2, double cos2, double ga0, double ga1,
                                          double ga2, double gb0, double gb1, double gb2, double s_a, double s_b, bool &fp, bool &fm,
                                          bool &wide)
{
    const double p0 = dot3(R[0], R[1], R[2], ga0, ga1, ga2);
    const double p1 = dot3(R[3], R[4], R[5], ga0, ga1, ga2);
    const double p2 = dot3(R[6], R[7], R[8], ga0, ga1, ga2);
    const double a11 = dot3(p0, p1, p2, p0, p1, p2);
    const double c = dot3(p0, p1, p2, gb0, gb1, gb2);
    const double a12 = -c;
    const double a22 = dot3(gb0, gb1, gb2, gb0, gb1, gb2);
    const double r1 = -dot3(p0, p1, p2, t0, t1, t2);
    const double r2 = dot3(gb0, gb1, gb2, t0, t1, t2);
    const double det = a11 * a22 - a12 * a12;
    const double na = r1 * a22 - a12 * r2;
    const double nb = a11 * r2 - a12 * r1;
    const double da = na * s_a, db = nb * s_b;
    fp = det > 0.0 && da > 0.0 && db > 0.0;
    fm = det > 0.0 && da < 0.0 && db < 0.0;   // -t: r1, r2, na and nb are the exact negatives
    wide = (c * s_a) * s_b <= 0.0 || c * c <= cos2 * (a11 * a22);
}

// the hot path: a.split workgroups per pair walk its list
__global__ __launch_bounds__(INIT_NT) void k_init_score(InitArgs a)
{
    const int m = blockIdx.y;
    int32_t *wi = a.wi + (size_t)m * INIT_WS_I;
    const int flags = wi[0];
    if (flags & PGX_INIT_SKIPPED) return;
    const bool score = flags == 0;
    const int sa = a.pairlist[2 * (size_t)m], sb = a.pairlist[2 * (size_t)m + 1];
    int ca = a.counts[sa], cb = a.counts[sb];
    ca = ca < 0 ? 0 : (ca > a.stride ? a.stride : ca);
    cb = cb < 0 ? 0 : (cb > a.stride ? a.stride : cb);
    const pgx_keypoint *kpa = a.kp + (size_t)sa * a.stride, *kpb = a.kp + (size_t)sb * a.stride;
    const pgx_pair *ml = a.matches + (size_t)m * a.stride;
    const double *wd = a.wd + (size_t)m * INIT_WS_D;
    double R1[9], R2[9];
#pragma unroll
    for (int k = 0; k < 9; k++) {
        R1[k] = wd[k];
        R2[k] = wd[9 + k];
    }
    const double t0 = wd[18], t1 = wd[19], t2 = wd[20];
    const double fxa = wd[21], fya = wd[22], cxa = wd[23], cya = wd[24];
    const double fxb = wd[25], fyb = wd[26], cxb = wd[27], cyb = wd[28];
    const double s_a = fxa * fya, s_b = fxb * fyb;
    int cnt[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};   // n, front [4], wide [4]: per wave, the same in every lane
    for (int e0 = blockIdx.x * INIT_NT; e0 < ca; e0 += a.split * INIT_NT) {
        const int e = e0 + threadIdx.x;
        bool cand = false;
        pgx_pair p = {0, 0, 0};
        if (e < ca) {
            p = ml[e];
            cand = p.dist <= a.max_dist && p.dist != PGX_DIST_NONE && (unsigned)p.k1 < (unsigned)ca && (unsigned)p.k2 < (unsigned)cb;
        }
        bool f[4] = {false, false, false, false}, w[4] = {false, false, false, false};
        if (cand && score) {
            const pgx_keypoint qa = kpa[p.k1], qb = kpb[p.k2];
            const double ga0 = ((double)qa.x - cxa) * fya, ga1 = ((double)qa.y - cya) * fxa;
            const double gb0 = ((double)qb.x - cxb) * fyb, gb1 = ((double)qb.y - cyb) * fxb;
            bool wd1, wd2;
            score_rot(R1, t0, t1, t2, a.cos2, ga0, ga1, s_a, gb0, gb1, s_b, s_a, s_b, f[0], f[1], wd1);
            score_rot(R2, t0, t1, t2, a.cos2, ga0, ga1, s_a, gb0, gb1, s_b, s_a, s_b, f[2], f[3], wd2);
            w[0] = f[0] && wd1;
            w[1] = f[1] && wd1;
            w[2] = f[2] && wd2;
            w[3] = f[3] && wd2;
        }
        cnt[0] += __popcll(__ballot(cand));
#pragma unroll
        for (int k = 0; k < 4; k++) {
            cnt[1 + k] += __popcll(__ballot(f[k]));
            cnt[5 + k] += __popcll(__ballot(w[k]));
        }
    }
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (int k = 0; k < 9; k++)
            if (cnt[k]) atomicAdd(&wi[3 + k], cnt[k]);   // integer sums: the order does not matter
    }
}

// one thread per pair: the winner and the two count flags
__global__ __launch_bounds__(INIT_NT) void k_init_finish(InitArgs a)
{
    const int m = blockIdx.x * INIT_NT + threadIdx.x;
    if (m >= a.M) return;
    const double NaN = __builtin_nan("");
    const int32_t *wi = a.wi + (size_t)m * INIT_WS_I;
    const double *wd = a.wd + (size_t)m * INIT_WS_D;
    int flags = wi[0];
    const int n = wi[3];
    int win = -1, wide = 0;
    if (flags == 0) {
        win = 0;
        int best = wi[4];
#pragma unroll
        for (int c = 1; c < 4; c++)
            if (wi[4 + c] > best) {
                best = wi[4 + c];
                win = c;
            }
        wide = wi[8 + win];
        if ((double)best < a.min_front_frac * (double)n) flags |= PGX_INIT_FEWFRONT;
        if (wide < a.min_points) flags |= PGX_INIT_FEWPOINTS;
    }
    double *o = a.Rt_pair + (size_t)m * 12;
    const double *R = wd + (win >= 2 ? 9 : 0);
    for (int k = 0; k < 9; k++) o[k] = win >= 0 ? R[k] : NaN;
    for (int k = 0; k < 3; k++) o[9 + k] = win >= 0 ? ((win & 1) ? -wd[18 + k] : wd[18 + k]) : NaN;
    int32_t *st = a.pair_stats + (size_t)m * 8;
    st[0] = n;
    for (int c = 0; c < 4; c++) st[1 + c] = wi[4 + c];
    st[5] = wide;
    st[6] = win;
    st[7] = flags;
}

// one workgroup: the report, the choice, the per-frame arrays
__global__ __launch_bounds__(INIT_NT) void k_init_pick(InitArgs a)
{
    __shared__ unsigned long long s_key[INIT_NT / 64];
    __shared__ unsigned long long s_pick[2];
    __shared__ int s_cnt[INIT_NT / 64];
    const double NaN = __builtin_nan("");
    int acc[5] = {0, 0, 0, 0, 0};
    unsigned long long key = 0;   // (wide + 1) << 32 | ~frame of a: ransac_key with the frame as the index
    for (int m = threadIdx.x; m < a.M; m += INIT_NT) {
        const int fl = a.pair_stats[(size_t)m * 8 + 7];
        acc[0] += fl == 0;
        acc[1] += (fl & (PGX_INIT_SKIPPED | PGX_INIT_BADINPUT)) != 0;
        acc[2] += (fl & PGX_INIT_DEGENERATE) != 0;
        acc[3] += (fl & PGX_INIT_FEWFRONT) != 0;
        acc[4] += (fl & PGX_INIT_FEWPOINTS) != 0;
        const unsigned long long k = ransac_key(fl == 0, a.pair_stats[(size_t)m * 8 + 5], a.wi[(size_t)m * INIT_WS_I + 1]);
        key = k > key ? k : key;
    }
#pragma unroll
    for (int k = 0; k < 5; k++) acc[k] = block_sum_i(acc[k], s_cnt);
    key = ransac_block_max<INIT_NT>(key, s_key);
    if (threadIdx.x == 0) s_pick[0] = key;
    __syncthreads();
    const unsigned long long key1 = s_pick[0];
    unsigned long long key2 = 0;   // ~frame of b << 32 | ~m among the pairs that hold key1
    if (key1 != 0ull)
        for (int m = threadIdx.x; m < a.M; m += INIT_NT) {
            const int fl = a.pair_stats[(size_t)m * 8 + 7];
            if (ransac_key(fl == 0, a.pair_stats[(size_t)m * 8 + 5], a.wi[(size_t)m * INIT_WS_I + 1]) != key1) continue;
            const unsigned long long k = ((unsigned long long)(0xFFFFFFFFu - (unsigned)a.wi[(size_t)m * INIT_WS_I + 2]) << 32) |
                                         (unsigned long long)(0xFFFFFFFFu - (unsigned)m);
            key2 = k > key2 ? k : key2;
        }
    __syncthreads();   // s_key is reused
    key2 = ransac_block_max<INIT_NT>(key2, s_key);
    if (threadIdx.x == 0) s_pick[1] = key2;
    __syncthreads();
    const int ms = key1 != 0ull ? ransac_key_index(s_pick[1]) : -1;
    int fa = -1, fb = -1;
    double rt[12];
#pragma unroll
    for (int k = 0; k < 12; k++) rt[k] = NaN;
    if (ms >= 0) {
        fa = a.wi[(size_t)ms * INIT_WS_I + 1];
        fb = a.wi[(size_t)ms * INIT_WS_I + 2];
#pragma unroll
        for (int k = 0; k < 12; k++) rt[k] = a.Rt_pair[(size_t)ms * 12 + k];
    }
    if (threadIdx.x == 0) {
        a.report[0] = a.M;
#pragma unroll
        for (int k = 0; k < 5; k++) a.report[1 + k] = acc[k];
        a.report[6] = ms;
        a.report[7] = ms >= 0 ? ransac_key_count(key1) : 0;
    }
    const double eye[12] = {1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0};
    for (int f = threadIdx.x; f < a.n_frames; f += INIT_NT) {
        const bool isa = ms >= 0 && f == fa, isb = ms >= 0 && f == fb;
        double r[12], P[12];
#pragma unroll
        for (int k = 0; k < 12; k++) r[k] = isa ? eye[k] : rt[k];
        camera_matrix(a.K + (size_t)f * 4, r, isa || isb, P);
#pragma unroll
        for (int k = 0; k < 12; k++) {
            a.Rt_out[(size_t)f * 12 + k] = isa || isb ? r[k] : NaN;
            a.P_out[(size_t)f * 12 + k] = P[k];
        }
        a.fixed_out[f] = isa ? 1 : 0;
        a.register_out[f] = 0;
    }
    __syncthreads();   // the zeros above are in memory before the marks below
    if (ms >= 0)
        for (int s = threadIdx.x; s < a.nslots; s += INIT_NT) {
            const int f = a.frame_ids ? a.frame_ids[s] : s;
            if (f >= 0 && f < a.n_frames && f != fa && f != fb) a.register_out[f] = 1;
        }
}

size_t init_carve(InitArgs &a, void *ws)
{
    const size_t Mc = (size_t)(a.M > 0 ? a.M : 1);
    WsCarver w(ws);
    a.wd = w.take<double>(Mc * INIT_WS_D * 8);
    a.wi = w.take<int32_t>(Mc * INIT_WS_I * 4);
    return w.total();
}

} // namespace

size_t pgx_init_pair_ws_bytes(const InitArgs &a)
{
    InitArgs b = a;
    return init_carve(b, nullptr);
}

void pgx_launch_init_pair(hipStream_t s, InitArgs a, void *ws)
{
    const int M = a.M, stride = a.stride;
    a.split = (stride + INIT_ROWS - 1) / INIT_ROWS;
    init_carve(a, ws);
    // the second grid dimension holds 65535 workgroups: longer pair lists go in slices (the kernels of a slice see its pointers)
    for (int m0 = 0; m0 < M; m0 += 65535) {
        InitArgs b = a;
        b.M = M - m0 < 65535 ? M - m0 : 65535;
        b.matches = a.matches + (size_t)m0 * stride;
        b.pairlist = a.pairlist + 2 * (size_t)m0;
        b.F = a.F + 9 * (size_t)m0;
        b.Rt_pair = a.Rt_pair + 12 * (size_t)m0;
        b.sigma = a.sigma ? a.sigma + m0 : nullptr;
        b.cand_Rt = a.cand_Rt ? a.cand_Rt + 48 * (size_t)m0 : nullptr;
        b.pair_stats = a.pair_stats + 8 * (size_t)m0;
        b.wd = a.wd + (size_t)m0 * INIT_WS_D;
        b.wi = a.wi + (size_t)m0 * INIT_WS_I;
        const int nb = (b.M + INIT_NT - 1) / INIT_NT;
        hipLaunchKernelGGL(k_init_setup, dim3(nb), dim3(INIT_NT), 0, s, b);
        hipLaunchKernelGGL(k_init_score, dim3(a.split, b.M), dim3(INIT_NT), 0, s, b);
        hipLaunchKernelGGL(k_init_finish, dim3(nb), dim3(INIT_NT), 0, s, b);
    }
    hipLaunchKernelGGL(k_init_pick, dim3(1), dim3(INIT_NT), 0, s, a);
}
