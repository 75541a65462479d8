// k_verify.hip -- two-view geometric verification of match lists by epipolar RANSAC (pgx_verify_pairs_dev; include/pgx.h).
//
// Per image pair: the candidates of its match list (the entries pgx_tracks_dev would link), the fundamental matrix with
// the most inliers among n_samples normalised 8-point fits with rank 2 enforced, up to refit_iters refits on the inlier
// set, and the list with everything but the final inliers rejected.  float64 throughout, no fused multiply-add (the
// library's -ffp-contract=off), convention h_a^T F h_b = 0 -- the guided matcher's.
//
// Kernels (all on the caller's stream):
//   k_ver_cand     one workgroup per pair: the candidates in list order (a block scan), their position per entry, and the
//                  SoA arrays x, y (frame a), u, v (frame b)
//   k_ver_samples  one thread per (pair, sample) of a chunk of samples: the sample's 8 positions, the fit, F (NaN = none).
//                  G (9x9) lives in registers and the eigenvectors in LDS, one 9x9 block per thread: together they do not
//                  fit the 256 vector registers a lane can compute on
//   k_ver_score    the hot path: one thread per hypothesis, a workgroup covers 256 hypotheses of one pair and walks the
//                  pair's candidates through LDS (every lane reads the same address: a broadcast).  The predicate has no
//                  division and no square root (18 multiplications, 15 additions); the counts are integers in registers; the
//                  workgroup's best key (pgx_ransac.h: inliers, then the smallest s) and its number of valid samples go to its own slot,
//                  no atomics
//   k_ver_pick     one workgroup per pair: the chunk's best key against the pair's running best (keys are distinct per
//                  sample, so the order of the chunks does not matter); a better one brings its F along
//   k_ver_refit    one workgroup per pair: the flags, up to refit_iters refits (the sums of the means, of the mean distances
//                  and the 45 sums of G as per-lane partials, xor butterflies per wave, four waves in a fixed order; the two
//                  eigen-solves on one lane; rescoring by all lanes), the final F and count
//   k_ver_write    per entry: d_out, d_inlier (the predicate at the final F), and the pair's d_stats
//   k_ver_summary  one workgroup: the report, integer sums over all pairs
// Pairs run in chunks of pgx_set_match_chunk pairs and samples in chunks of max(2^16 / pairs, 256) samples, so that the
// workspace stays bounded; neither changes a result.  DESIGN.md section 20 has the measurements.
#include "pgx_stage_args.h"
#include "pgx_eig.h"

namespace {

constexpr int VER_NT = 256;    // threads per workgroup of every kernel here but k_ver_samples
static_assert(VER_NT == 256, "block_sums (pgx_trackgraph.h) adds up four waves");
constexpr int VER_SNT = 64;    // threads per workgroup of k_ver_samples (41 KB of LDS: one 9x9 block per thread)
// (pair x sample) cells per chunk of samples; a chunk is never below one scoring workgroup per pair, so the hypothesis
// buffer holds max(2^16, 256 M) cells of 72 bytes: 37 MB at the default 2048 pairs per workspace, 75 MB at 4096
constexpr long long VER_CHUNK_CELLS = 1 << 16;

// the inlier predicate (include/pgx.h): no division, no square root
__device__ __forceinline__ bool inlier(const double (&F)[9], double T, double x, double y, double u, double v)
{
    const double m0 = (F[0] * u + F[1] * v) + F[2];
    const double m1 = (F[3] * u + F[4] * v) + F[5];
    const double m2 = (F[6] * u + F[7] * v) + F[8];
    const double e = (x * m0 + y * m1) + m2;
    const double l0 = (F[0] * x + F[3] * y) + F[6];
    const double l1 = (F[1] * x + F[4] * y) + F[7];
    const double d = ((l0 * l0 + l1 * l1) + m0 * m0) + m1 * m1;
    return d > 0.0 && e * e <= T * d;
}

// the 9 products of one correspondence in normalised coordinates
__device__ __forceinline__ void fit_row(double sa, double ta0, double ta1, double sb, double tb0, double tb1, double x, double y,
                                        double u, double v, double (&r)[9])
{
    const double a0 = sa * x + ta0, a1 = sa * y + ta1, b0 = sb * u + tb0, b1 = sb * v + tb1;
    r[0] = a0 * b0;
    r[1] = a0 * b1;
    r[2] = a0;
    r[3] = a1 * b0;
    r[4] = a1 * b1;
    r[5] = a1;
    r[6] = b0;
    r[7] = b1;
    r[8] = 1.0;
}

// steps 5 to 10 of the fit: G (destroyed) and the two normalisations T = [[s, 0, t0], [0, s, t1], [0, 0, 1]] -> F with unit
// Frobenius norm; false for a non-finite entry.  V is the caller's 9x9 block for the eigenvectors.
__device__ __forceinline__ bool fit_finish(double (&G)[9][9], double (&V)[9][9], double sa, double ta0, double ta1, double sb,
                                           double tb0, double tb1, double (&F)[9])
{
    double f[9];
    smallest_eigvec_in<9>(G, V, f);
    double B[3][3], V3[3][3], v3[3];
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
        for (int j = 0; j < 3; j++) B[i][j] = (f[i] * f[j] + f[3 + i] * f[3 + j]) + f[6 + i] * f[6 + j];
    smallest_eigvec_in<3>(B, V3, v3);
    double h[9];
#pragma unroll
    for (int i = 0; i < 3; i++) {
        const double w = (f[3 * i] * v3[0] + f[3 * i + 1] * v3[1]) + f[3 * i + 2] * v3[2];
#pragma unroll
        for (int j = 0; j < 3; j++) h[3 * i + j] = f[3 * i + j] - w * v3[j];
    }
    // Ta^T Fh' Tb
    double m[9];
#pragma unroll
    for (int j = 0; j < 3; j++) {
        m[j] = sa * h[j];
        m[3 + j] = sa * h[3 + j];
        m[6 + j] = (ta0 * h[j] + ta1 * h[3 + j]) + h[6 + j];
    }
    double nn = 0.0;
#pragma unroll
    for (int i = 0; i < 3; i++) {
        F[3 * i] = m[3 * i] * sb;
        F[3 * i + 1] = m[3 * i + 1] * sb;
        F[3 * i + 2] = (m[3 * i] * tb0 + m[3 * i + 1] * tb1) + m[3 * i + 2];
    }
#pragma unroll
    for (int k = 0; k < 9; k++) nn += F[k] * F[k];
    const double nr = sqrt(nn);
    bool ok = true;
#pragma unroll
    for (int k = 0; k < 9; k++) {
        F[k] = F[k] / nr;
        ok = ok && isfinite(F[k]);
    }
    return ok;
}

// ---- kernels -------------------------------------------------------------------------------------------------------

// one workgroup per pair: the candidates in list order
__global__ __launch_bounds__(VER_NT) void k_ver_cand(VerArgs a)
{
    __shared__ int s_wave[VER_NT / 64];
    const int m = blockIdx.x;
    const int fa = a.pairlist[2 * m], fb = a.pairlist[2 * m + 1];
    int ca = a.counts[fa], cb = a.counts[fb];
    ca = ca < 0 ? 0 : (ca > a.stride ? a.stride : ca);
    cb = cb < 0 ? 0 : (cb > a.stride ? a.stride : cb);
    const pgx_keypoint *kpa = a.kp + (size_t)fa * a.stride, *kpb = a.kp + (size_t)fb * a.stride;
    const size_t base = (size_t)m * a.stride;
    const int wave = threadIdx.x >> 6, ln = threadIdx.x & 63;
    int done = 0;
    for (int e0 = 0; e0 < ca; e0 += VER_NT) {
        const int e = e0 + threadIdx.x;
        bool cand = false;
        pgx_pair p = {0, 0, 0};
        if (e < ca) {
            p = a.matches[base + e];
            cand = p.dist <= a.max_dist && p.dist != PGX_DIST_NONE && (unsigned)p.k1 < (unsigned)ca && (unsigned)p.k2 < (unsigned)cb;
        }
        const unsigned long long bal = __ballot(cand);
        if (ln == 0) s_wave[wave] = __popcll(bal);
        __syncthreads();
        int pos = done, tot = 0;
        for (int w = 0; w < VER_NT / 64; w++) {
            pos += w < wave ? s_wave[w] : 0;
            tot += s_wave[w];
        }
        pos += __popcll(bal & ((1ull << ln) - 1ull));
        if (cand) {
            a.x[base + pos] = (double)kpa[p.k1].x;
            a.y[base + pos] = (double)kpa[p.k1].y;
            a.u[base + pos] = (double)kpb[p.k2].x;
            a.v[base + pos] = (double)kpb[p.k2].y;
        }
        if (e < ca) a.cpos[base + e] = cand ? pos : -1;
        done += tot;
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        a.ncand[m] = done;
        a.run[m] = 0ull;
        a.run_valid[m] = 0;
    }
}

// one thread per (pair, sample) of the chunk [s0, s0 + chunk)
__global__ __launch_bounds__(VER_SNT) void k_ver_samples(VerArgs a, int s0, int chunk)
{
    __shared__ double s_V[VER_SNT][9][9];
    const int m = blockIdx.y;
    const int ls = blockIdx.x * VER_SNT + threadIdx.x;
    const int s = s0 + ls;
    if (ls >= chunk || s >= a.n_samples) return;
    const int n = a.ncand[m];
    const size_t base = (size_t)m * a.stride;
    const double NaN = __builtin_nan("");
    double F[9];
    bool ok = n >= 8;
    if (ok) {
        const int fa = a.pairlist[2 * m], fb = a.pairlist[2 * m + 1];
        uint64_t st = ransac_stream(a.seed, fa, s) ^ (uint64_t)(uint32_t)fb * 0x9E3779B97F4A7C15ull;   // the pair is (fa, fb)
        int id[8];
        ransac_draw(st, n, 8, id);
        double px[8], py[8], pu[8], pv[8];
        double cax = 0.0, cay = 0.0, cbx = 0.0, cby = 0.0;
#pragma unroll
        for (int k = 0; k < 8; k++) {
            px[k] = a.x[base + id[k]];
            py[k] = a.y[base + id[k]];
            pu[k] = a.u[base + id[k]];
            pv[k] = a.v[base + id[k]];
            cax += px[k];
            cay += py[k];
            cbx += pu[k];
            cby += pv[k];
        }
        cax = cax / 8.0;
        cay = cay / 8.0;
        cbx = cbx / 8.0;
        cby = cby / 8.0;
        double da = 0.0, db = 0.0;
#pragma unroll
        for (int k = 0; k < 8; k++) {
            const double ax = px[k] - cax, ay = py[k] - cay, bx = pu[k] - cbx, by = pv[k] - cby;
            da += sqrt(ax * ax + ay * ay);
            db += sqrt(bx * bx + by * by);
        }
        da = da / 8.0;
        db = db / 8.0;
        ok = da > 0.0 && db > 0.0;
        const double sa = sqrt(2.0) / da, sb = sqrt(2.0) / db;
        const double ta0 = -(sa * cax), ta1 = -(sa * cay), tb0 = -(sb * cbx), tb1 = -(sb * cby);
        double G[9][9];
#pragma unroll
        for (int i = 0; i < 9; i++)
#pragma unroll
            for (int j = 0; j < 9; j++) G[i][j] = 0.0;
#pragma unroll
        for (int k = 0; k < 8; k++) {
            double r[9];
            fit_row(sa, ta0, ta1, sb, tb0, tb1, px[k], py[k], pu[k], pv[k], r);
#pragma unroll
            for (int i = 0; i < 9; i++)
#pragma unroll
                for (int j = i; j < 9; j++) G[i][j] += r[i] * r[j];
        }
#pragma unroll
        for (int i = 0; i < 9; i++)
#pragma unroll
            for (int j = 0; j < i; j++) G[i][j] = G[j][i];
        ok = fit_finish(G, s_V[threadIdx.x], sa, ta0, ta1, sb, tb0, tb1, F) && ok;
    }
    double *out = a.hyp + ((size_t)m * chunk + ls) * 9;
#pragma unroll
    for (int k = 0; k < 9; k++) out[k] = ok ? F[k] : NaN;
    if (a.sample_F) {
        double *sf = a.sample_F + ((size_t)m * a.n_samples + s) * 9;
#pragma unroll
        for (int k = 0; k < 9; k++) sf[k] = ok ? F[k] : NaN;
    }
}

// the hot path: a workgroup scores 256 hypotheses of one pair against all its candidates
__global__ __launch_bounds__(VER_NT) void k_ver_score(VerArgs a, int s0, int chunk)
{
    __shared__ double s_x[VER_NT], s_y[VER_NT], s_u[VER_NT], s_v[VER_NT];
    __shared__ unsigned long long s_key[VER_NT / 64];
    __shared__ int s_nv[VER_NT / 64];
    const int m = blockIdx.y;
    const int gb = s0 / VER_NT + (int)blockIdx.x;   // scoring workgroup of the pair
    if (gb >= a.nblk) return;                       // a last chunk may reach past n_samples
    const int ls = blockIdx.x * VER_NT + threadIdx.x;
    const int s = s0 + ls;
    const int n = a.ncand[m];
    const size_t base = (size_t)m * a.stride;
    const double T = a.inlier_px * a.inlier_px;
    double F[9];
    const bool live = ls < chunk && s < a.n_samples;
    bool valid = live;
    if (live) {
        const double *hp = a.hyp + ((size_t)m * chunk + ls) * 9;
#pragma unroll
        for (int k = 0; k < 9; k++) F[k] = hp[k];
        valid = F[0] == F[0];
    }
    int cnt = 0;
    for (int j0 = 0; j0 < n; j0 += VER_NT) {
        const int j = j0 + threadIdx.x;
        if (j < n) {
            s_x[threadIdx.x] = a.x[base + j];
            s_y[threadIdx.x] = a.y[base + j];
            s_u[threadIdx.x] = a.u[base + j];
            s_v[threadIdx.x] = a.v[base + j];
        }
        __syncthreads();
        const int mm = n - j0 < VER_NT ? n - j0 : VER_NT;
        if (valid) {
#pragma unroll 4
            for (int i = 0; i < mm; i++) cnt += inlier(F, T, s_x[i], s_y[i], s_u[i], s_v[i]) ? 1 : 0;
        }
        __syncthreads();
    }
    if (live && a.sample_count) a.sample_count[(size_t)m * a.n_samples + s] = valid ? cnt : -1;
    const int nv = __popcll(__ballot(valid));
    if ((threadIdx.x & 63) == 0) s_nv[threadIdx.x >> 6] = nv;
    const unsigned long long key = ransac_block_max<VER_NT>(ransac_key(valid, cnt, s), s_key);   // its barrier covers s_nv
    if (threadIdx.x == 0) {
        a.best[(size_t)m * a.nblk + gb] = key;
        a.nvalid[(size_t)m * a.nblk + gb] = (s_nv[0] + s_nv[1]) + (s_nv[2] + s_nv[3]);
    }
}

// one workgroup per pair: the chunk's best key against the running best
__global__ __launch_bounds__(VER_NT) void k_ver_pick(VerArgs a, int s0, int chunk)
{
    __shared__ unsigned long long s_key[VER_NT / 64];
    __shared__ int s_nv[VER_NT / 64];
    const int m = blockIdx.x;
    const int b0 = s0 / VER_NT;
    int b1 = b0 + chunk / VER_NT;
    b1 = b1 < a.nblk ? b1 : a.nblk;
    unsigned long long key = 0;
    int nv = 0;
    for (int b = b0 + threadIdx.x; b < b1; b += VER_NT) {   // ransac_row_max written out: the valid counts ride along
        const unsigned long long k = a.best[(size_t)m * a.nblk + b];
        key = k > key ? k : key;
        nv += a.nvalid[(size_t)m * a.nblk + b];
    }
    key = ransac_wave_max(key);
    nv = gsum_i<64>(nv);
    if ((threadIdx.x & 63) == 0) {
        s_key[threadIdx.x >> 6] = key;
        s_nv[threadIdx.x >> 6] = nv;
    }
    __syncthreads();
    if (threadIdx.x != 0) return;
    for (int w = 1; w < VER_NT / 64; w++) {   // ransac_block_max written out, like the scan
        key = s_key[w] > key ? s_key[w] : key;
        nv += s_nv[w];
    }
    a.run_valid[m] += nv;
    if (key > a.run[m]) {
        a.run[m] = key;
        const int s = ransac_key_index(key);
        const double *hp = a.hyp + ((size_t)m * chunk + (s - s0)) * 9;
        for (int k = 0; k < 9; k++) a.win[(size_t)m * 9 + k] = hp[k];
    }
}

__global__ __launch_bounds__(VER_NT) void k_ver_refit(VerArgs a)
{
    __shared__ double s_sum[45][VER_NT / 64];
    __shared__ double s_V[9][9];
    __shared__ double s_F[9];
    __shared__ int s_cnt[VER_NT / 64];
    __shared__ int s_ok;
    const int m = blockIdx.x;
    const int n = a.ncand[m];
    const size_t base = (size_t)m * a.stride;
    const double T = a.inlier_px * a.inlier_px;
    const double NaN = __builtin_nan("");
    const unsigned long long key = a.run[m];
    int flags = 0, win = -1, wcount = 0;
    if (n < 8) {
        flags = PGX_VER_FEWMATCHES;
    } else if (key == 0ull) {
        flags = PGX_VER_NOMODEL;
    } else {
        win = ransac_key_index(key);
        wcount = ransac_key_count(key);
    }
    // F through LDS: it then lives in vector registers
    if (threadIdx.x < 9) s_F[threadIdx.x] = a.win[(size_t)m * 9 + threadIdx.x];
    __syncthreads();
    double F[9];
#pragma unroll
    for (int k = 0; k < 9; k++) F[k] = s_F[k];
    __syncthreads();
    int cur = wcount, kept = 0;
    if (win >= 0) {
        for (int it = 0; it < a.refit_iters; it++) {
            if (cur < 8) break;
            const double dn = (double)cur;
            double c4[4] = {0.0, 0.0, 0.0, 0.0};
            for (int j = threadIdx.x; j < n; j += VER_NT) {
                const double x = a.x[base + j], y = a.y[base + j], u = a.u[base + j], v = a.v[base + j];
                if (!inlier(F, T, x, y, u, v)) continue;
                c4[0] += x;
                c4[1] += y;
                c4[2] += u;
                c4[3] += v;
            }
            block_sums<4>(c4, s_sum);
            const double cax = c4[0] / dn, cay = c4[1] / dn, cbx = c4[2] / dn, cby = c4[3] / dn;
            double d2[2] = {0.0, 0.0};
            for (int j = threadIdx.x; j < n; j += VER_NT) {
                const double x = a.x[base + j], y = a.y[base + j], u = a.u[base + j], v = a.v[base + j];
                if (!inlier(F, T, x, y, u, v)) continue;
                const double ax = x - cax, ay = y - cay, bx = u - cbx, by = v - cby;
                d2[0] += sqrt(ax * ax + ay * ay);
                d2[1] += sqrt(bx * bx + by * by);
            }
            block_sums<2>(d2, s_sum);
            const double da = d2[0] / dn, db = d2[1] / dn;
            const double sa = sqrt(2.0) / da, sb = sqrt(2.0) / db;
            const double ta0 = -(sa * cax), ta1 = -(sa * cay), tb0 = -(sb * cbx), tb1 = -(sb * cby);
            double g[45];
#pragma unroll
            for (int k = 0; k < 45; k++) g[k] = 0.0;
            for (int j = threadIdx.x; j < n; j += VER_NT) {
                const double x = a.x[base + j], y = a.y[base + j], u = a.u[base + j], v = a.v[base + j];
                if (!inlier(F, T, x, y, u, v)) continue;
                double r[9];
                fit_row(sa, ta0, ta1, sb, tb0, tb1, x, y, u, v, r);
                int k = 0;
#pragma unroll
                for (int p = 0; p < 9; p++)
#pragma unroll
                    for (int q = p; q < 9; q++) g[k++] += r[p] * r[q];
            }
            block_sums<45>(g, s_sum);
            if (threadIdx.x == 0) {
                double G[9][9], Fn[9];
                int k = 0;
#pragma unroll
                for (int p = 0; p < 9; p++)
#pragma unroll
                    for (int q = p; q < 9; q++) {
                        G[p][q] = g[k];
                        G[q][p] = g[k];
                        k++;
                    }
                const bool ok = fit_finish(G, s_V, sa, ta0, ta1, sb, tb0, tb1, Fn) && da > 0.0 && db > 0.0;
#pragma unroll
                for (int q = 0; q < 9; q++) s_F[q] = Fn[q];
                s_ok = ok ? 1 : 0;
            }
            __syncthreads();
            double Fn[9];
#pragma unroll
            for (int k = 0; k < 9; k++) Fn[k] = s_F[k];
            const bool ok = s_ok != 0;
            __syncthreads();
            int c = 0;
            if (ok)
                for (int j = threadIdx.x; j < n; j += VER_NT)
                    c += inlier(Fn, T, a.x[base + j], a.y[base + j], a.u[base + j], a.v[base + j]) ? 1 : 0;
            c = block_sum_i(c, s_cnt);
            if (!ok || c <= cur) break;
            cur = c;
            kept++;
#pragma unroll
            for (int k = 0; k < 9; k++) F[k] = Fn[k];
        }
        if (cur < a.min_inliers) flags |= PGX_VER_FEWINLIERS;
    }
    if (threadIdx.x < 9) {
        double f = NaN;
#pragma unroll
        for (int k = 0; k < 9; k++) f = (int)threadIdx.x == k && win >= 0 ? F[k] : f;
        a.F[(size_t)m * 9 + threadIdx.x] = f;
        if (a.F32) a.F32[(size_t)m * 9 + threadIdx.x] = (float)f;
    }
    if (threadIdx.x == 0) {
        int32_t *st = a.winfo + (size_t)m * 8;
        st[0] = n;
        st[1] = win >= 0 ? wcount : 0;
        st[2] = win >= 0 ? cur : 0;
        st[3] = win;
        st[4] = flags;
        st[5] = kept;
        st[6] = a.run_valid[m];
        st[7] = 0;
    }
}

// per entry: d_out and d_inlier; the pair's d_stats
__global__ __launch_bounds__(VER_NT) void k_ver_write(VerArgs a)
{
    __shared__ double s_F[9];
    const int m = blockIdx.y;
    const int fa = a.pairlist[2 * m];
    int ca = a.counts[fa];
    ca = ca < 0 ? 0 : (ca > a.stride ? a.stride : ca);
    const size_t base = (size_t)m * a.stride;
    const int32_t *st = a.winfo + (size_t)m * 8;
    if (blockIdx.x == 0 && threadIdx.x < 8) a.stats[(size_t)m * 8 + threadIdx.x] = st[threadIdx.x];
    if (threadIdx.x < 9) s_F[threadIdx.x] = a.F[(size_t)m * 9 + threadIdx.x];
    __syncthreads();
    const int e = blockIdx.x * VER_NT + threadIdx.x;
    if (e >= ca) return;
    double F[9];
#pragma unroll
    for (int k = 0; k < 9; k++) F[k] = s_F[k];
    const bool accepted = st[4] == 0;
    const double T = a.inlier_px * a.inlier_px;
    const int pos = a.cpos[base + e];
    const pgx_pair p = a.matches[base + e];
    int flag = -1;
    if (pos >= 0) flag = inlier(F, T, a.x[base + pos], a.y[base + pos], a.u[base + pos], a.v[base + pos]) ? 1 : 0;   // NaN F: 0
    pgx_pair o = p;
    if (!(accepted && flag == 1)) {
        o.k2 = -1;
        o.dist = PGX_DIST_NONE;
    }
    a.out[base + e] = o;
    if (a.inlier) a.inlier[base + e] = flag;
}

// the report over all M pairs of the call
__global__ __launch_bounds__(VER_NT) void k_ver_summary(const int32_t *stats, int M, int32_t *report)
{
    __shared__ int s_acc[8];
    if (threadIdx.x < 8) s_acc[threadIdx.x] = 0;
    __syncthreads();
    int acc[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    for (int m = threadIdx.x; m < M; m += blockDim.x) {
        const int32_t *st = stats + (size_t)m * 8;
        acc[0] += 1;
        acc[1] += st[4] == 0;
#pragma unroll
        for (int b = 0; b < 3; b++) acc[2 + b] += (st[4] >> b) & 1;
        acc[5] += st[0];
        acc[6] += st[4] == 0 ? st[2] : 0;
    }
#pragma unroll
    for (int k = 0; k < 8; k++)
        if (acc[k]) atomicAdd(&s_acc[k], acc[k]);   // integer sums: the order does not matter
    __syncthreads();
    if (threadIdx.x < 8) report[threadIdx.x] = s_acc[threadIdx.x];
}

} // namespace

// samples per chunk for a workspace of M pairs: the caller sizes the workspace and runs every launch that shares it with
// this one value (a shorter last chunk of pairs would otherwise get a longer chunk of samples than the workspace holds)
int pgx_verify_chunk(int M, int n_samples)
{
    return ransac_chunk(VER_CHUNK_CELLS, M, VER_NT, n_samples);   // 256 samples: one scoring workgroup
}

namespace {

// the workspace of M pairs at `chunk` samples per chunk, described once: a's workspace pointers (none valid for ws =
// nullptr) and nblk; the bytes, which grow with M
size_t ver_carve(VerArgs &a, void *ws, int M, int stride, int n_samples, int chunk)
{
    const size_t Mc = (size_t)(M > 0 ? M : 1), N = Mc * (size_t)stride;
    a.nblk = (n_samples + VER_NT - 1) / VER_NT;
    WsCarver w(ws);
    a.ncand = w.take<int32_t>(Mc * 4);
    a.cpos = w.take<int32_t>(N * 4);
    a.x = w.take<double>(N * 8);
    a.y = w.take<double>(N * 8);
    a.u = w.take<double>(N * 8);
    a.v = w.take<double>(N * 8);
    a.hyp = w.take<double>(Mc * (size_t)chunk * 9 * 8);
    a.best = w.take<unsigned long long>(Mc * (size_t)a.nblk * 8);
    a.nvalid = w.take<int32_t>(Mc * (size_t)a.nblk * 4);
    a.run = w.take<unsigned long long>(Mc * 8);
    a.run_valid = w.take<int32_t>(Mc * 4);
    a.win = w.take<double>(Mc * 9 * 8);
    a.winfo = w.take<int32_t>(Mc * 8 * 4);
    return w.total();
}

} // namespace

size_t pgx_verify_ws_bytes(int M, int stride, int n_samples, int chunk)
{
    VerArgs a;
    return ver_carve(a, nullptr, M, stride, n_samples, chunk);
}

// M pairs that share one workspace of at least pgx_verify_ws_bytes(M, stride, n_samples, chunk) bytes (a chunk of the call's
// pairs; the pointers are the chunk's), chunk a multiple of 256
void pgx_launch_verify(hipStream_t s, VerArgs a, int M, int chunk, void *ws)
{
    if (M <= 0) return;
    ver_carve(a, ws, M, a.stride, a.n_samples, chunk);
    hipLaunchKernelGGL(k_ver_cand, dim3(M), dim3(VER_NT), 0, s, a);
    for (int s0 = 0; s0 < a.n_samples; s0 += chunk) {
        hipLaunchKernelGGL(k_ver_samples, dim3(chunk / VER_SNT, M), dim3(VER_SNT), 0, s, a, s0, chunk);
        hipLaunchKernelGGL(k_ver_score, dim3(chunk / VER_NT, M), dim3(VER_NT), 0, s, a, s0, chunk);
        hipLaunchKernelGGL(k_ver_pick, dim3(M), dim3(VER_NT), 0, s, a, s0, chunk);
    }
    hipLaunchKernelGGL(k_ver_refit, dim3(M), dim3(VER_NT), 0, s, a);
    hipLaunchKernelGGL(k_ver_write, dim3((a.stride + VER_NT - 1) / VER_NT, M), dim3(VER_NT), 0, s, a);
}

void pgx_launch_verify_summary(hipStream_t s, const int32_t *d_stats, int M, int32_t *d_report)
{
    hipLaunchKernelGGL(k_ver_summary, dim3(1), dim3(VER_NT), 0, s, d_stats, M, d_report);
}
