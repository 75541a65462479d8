// k_denseviews.hip -- the plan of the dense stage from the sparse model: per reference frame its source frames (d_views) and
// the depth interval to sweep (d_range), the two tables pgx_depth_maps_dev takes (pgx_dense_views_dev; the rule is in
// include/pgx.h).  Not in the reference.
//
// Kernels (seven launches and one memset, all on the caller's stream; n_tracks is read on the device):
//   k_dvw_frames   one workgroup: per frame the third row of P, C = -(M^-1 p4), sign det M, ||m3|| and known in one table row
//                  (k_cns_frames' arithmetic), the frame -> first row map of d_refs, the tracks to process, the zeroed report
//   k_dvw_count    persistent, grid-stride over the tracks in k_cns_write's three length classes (more than 32 nodes a whole
//                  wave, 9..32 nodes 16 lanes, 0..8 nodes 4 lanes), lanes over NODES: z per used node, the used nodes per frame
//                  in an LDS histogram (n_frames <= DVW_LDS_FRAMES; global atomics beyond) flushed once per workgroup
//   k_dvw_scan     one workgroup: the exclusive scan of the per-frame counts = the frames' buckets in the z workspace
//   k_dvw_scatter  the walk of k_dvw_count twice: the workgroup's own counts per frame (LDS), one atomic per frame and
//                  workgroup to reserve its part of the bucket, then the z values to LDS-counted places in it.  The order
//                  inside a bucket varies from run to run; an order statistic of the multiset does not.
//   k_dvw_pairs    persistent over the tracks in the same classes: i walks the track's nodes (group-uniform), the lanes take
//                  the j > i.  A pair adds (1 | good << 32) to the cells (row of a, b) and (row of b, a) of the rows d_refs
//                  names: in LDS while R * n_frames <= DVW_LDS_CELLS (one 64-bit LDS atomic per cell and pair, one global
//                  64-bit atomic per non-zero cell and workgroup at the end), else in the global table directly
//   k_dvw_select   one workgroup per reference: the candidates' count, S rounds of a block argmax over the key (good, shared,
//                  -frame) below the previous winner, and an 8-bit radix select (8 passes over the 64-bit patterns, which
//                  order as positive doubles do) of the two order statistics at once in the frame's bucket
// Counters are integers throughout.  DESIGN.md section 27 has the measurements.
#include "pgx_stage_args.h"

namespace {

constexpr int DVW_NT = 256;              // threads per workgroup of every kernel here
constexpr int DVW_GRID_MAX = 1024;       // workgroups of k_dvw_count and k_dvw_scatter (4 per CU), at most
constexpr int DVW_PAIR_GRID_MAX = 256;   // workgroups of k_dvw_pairs (1 per CU): each one flushes up to DVW_LDS_CELLS cells
constexpr int DVW_LDS_FRAMES = 4096;     // n_frames up to which the per-frame counts of a workgroup live in LDS (16 KiB)
constexpr int DVW_LDS_CELLS = 4096;      // R * n_frames up to which the pair counts of a workgroup live in LDS (32 KiB)
constexpr int DVW_CAM = 12;              // doubles per frame: P's third row (4), C (3), sign det M, ||m3||, known (1 / 0), unused (2)
constexpr int DC_C = 4, DC_SGN = 7, DC_NRM = 8, DC_KNOWN = 9;
constexpr int DVW_NOROW = 0x7FFFFFFF;    // rowof: no row of d_refs names the frame
// meta (ints): [0] tracks to process

__device__ __forceinline__ int dvw_class(int n) { return n > 32 ? 2 : (n > 8 ? 1 : 0); }

// track t is used: its point in X
__device__ __forceinline__ bool dvw_track(const DvwArgs &a, long long t, double (&X)[3])
{
    if (a.track_flags && a.track_flags[t] != 0) return false;
#pragma unroll
    for (int k = 0; k < 3; k++) X[k] = a.xyz[3 * t + k];
    return isfinite(X[0]) && isfinite(X[1]) && isfinite(X[2]);
}

// node o of a used track with the point X is used: its frame and its depth there.  report: a frame outside [0, n_frames) is
// raised in the status word (one of the walks does)
template <bool REPORT> __device__ __forceinline__ bool dvw_node(const DvwArgs &a, long long o, const double (&X)[3], int &f, double &z)
{
    f = a.tv.nodes[2 * o];
    if (f < 0 || f >= a.tv.n_frames) {
        if (REPORT) atomicOr(a.status, (int)PGX_ST_DVW_NODE);
        return false;
    }
    const double *c = a.cam + (size_t)f * DVW_CAM;
    if (c[DC_KNOWN] == 0.0) return false;
    z = (c[DC_SGN] * (((c[0] * X[0] + c[1] * X[1]) + c[2] * X[2]) + c[3])) / c[DC_NRM];
    return z > 0.0;
}

// fn(frame, z) for every used node of every used track of length class CLS, G lanes per track; used: the used tracks that
// this thread led
template <int G, int CLS, bool REPORT, class Fn> __device__ __forceinline__ void dvw_walk(const DvwArgs &a, long long nt, int &used, Fn fn)
{
    PGX_TRACK_LOOP(G, nt)
    {
        int o0, n;
        const bool wellformed = track_range(a.tv, t, o0, n);
        if (dvw_class(n) != CLS) continue;
        if (REPORT && !wellformed && lane == 0) atomicOr(a.status, (int)PGX_ST_DVW_NODE);
        double X[3];
        if (!dvw_track(a, t, X)) continue;
        used += lane == 0;
        for (int b = lane; b < n; b += G) {
            int f;
            double z;
            if (dvw_node<REPORT>(a, (long long)o0 + b, X, f, z)) fn(f, z);
        }
    }
}

template <bool REPORT, class Fn> __device__ __forceinline__ void dvw_walk_all(const DvwArgs &a, long long nt, int &used, Fn fn)
{
    dvw_walk<64, 2, REPORT>(a, nt, used, fn);
    dvw_walk<16, 1, REPORT>(a, nt, used, fn);
    dvw_walk<4, 0, REPORT>(a, nt, used, fn);
}

__global__ __launch_bounds__(DVW_NT) void k_dvw_frames(DvwArgs a)
{
    const int nf = a.tv.n_frames;
    for (int f = threadIdx.x; f < nf; f += blockDim.x) {
        const double *p = a.P + (size_t)f * 12;
        bool fin = true;
#pragma unroll
        for (int k = 0; k < 12; k++) fin = fin && isfinite(p[k]);
        const double m00 = p[0], m01 = p[1], m02 = p[2], m10 = p[4], m11 = p[5], m12 = p[6], m20 = p[8], m21 = p[9], m22 = p[10];
        // cofactors; M^-1 = adj(M) / det, adj = the cofactor matrix transposed (k_cns_frames' order of operations)
        const double k00 = m11 * m22 - m12 * m21, k01 = m12 * m20 - m10 * m22, k02 = m10 * m21 - m11 * m20;
        const double k10 = m02 * m21 - m01 * m22, k11 = m00 * m22 - m02 * m20, k12 = m01 * m20 - m00 * m21;
        const double k20 = m01 * m12 - m02 * m11, k21 = m02 * m10 - m00 * m12, k22 = m00 * m11 - m01 * m10;
        const double det = (m00 * k00 + m01 * k01) + m02 * k02;
        double iv[9];
        iv[0] = k00 / det; iv[1] = k10 / det; iv[2] = k20 / det;
        iv[3] = k01 / det; iv[4] = k11 / det; iv[5] = k21 / det;
        iv[6] = k02 / det; iv[7] = k12 / det; iv[8] = k22 / det;
        double *c = a.cam + (size_t)f * DVW_CAM;
        c[0] = m20; c[1] = m21; c[2] = m22; c[3] = p[11];
#pragma unroll
        for (int r = 0; r < 3; r++) c[DC_C + r] = -((iv[3 * r] * p[3] + iv[3 * r + 1] * p[7]) + iv[3 * r + 2] * p[11]);
        c[DC_SGN] = det > 0.0 ? 1.0 : -1.0;
        c[DC_NRM] = sqrt((m20 * m20 + m21 * m21) + m22 * m22);
        c[DC_KNOWN] = fin && det != 0.0 ? 1.0 : 0.0;
        c[10] = c[11] = 0.0;
        a.fcnt[f] = 0;
        a.rowof[f] = DVW_NOROW;
    }
    if (threadIdx.x == 0) {
        const int nt = clamp_tracks(a.tv, a.status, PGX_ST_DVW_CAP);
        a.meta[0] = nt;
        a.report[0] = nt;
    }
    if (threadIdx.x >= 1 && threadIdx.x < 8) a.report[threadIdx.x] = 0;
    __syncthreads();
    for (int r = threadIdx.x; r < a.R; r += blockDim.x) {
        const int f = a.refs ? a.refs[r] : r;
        if (f >= 0 && f < nf) atomicMin(&a.rowof[f], r);
    }
}

__global__ __launch_bounds__(DVW_NT) void k_dvw_count(DvwArgs a)
{
    __shared__ int s_h[DVW_LDS_FRAMES];
    __shared__ int s_acc[2];
    const int nf = a.tv.n_frames;
    const bool lds = nf <= DVW_LDS_FRAMES;
    if (lds)
        for (int f = threadIdx.x; f < nf; f += DVW_NT) s_h[f] = 0;
    if (threadIdx.x < 2) s_acc[threadIdx.x] = 0;
    __syncthreads();
    int tracks = 0, nodes = 0;
    dvw_walk_all<true>(a, a.meta[0], tracks, [&](int f, double) {
        nodes++;
        if (lds) atomicAdd(&s_h[f], 1);
        else atomicAdd(&a.fcnt[f], 1);
    });
    if (tracks) atomicAdd(&s_acc[0], tracks);
    if (nodes) atomicAdd(&s_acc[1], nodes);
    __syncthreads();
    if (lds)
        for (int f = threadIdx.x; f < nf; f += DVW_NT)
            if (s_h[f]) atomicAdd(&a.fcnt[f], s_h[f]);
    if (threadIdx.x < 2 && s_acc[threadIdx.x]) atomicAdd(&a.report[1 + threadIdx.x], s_acc[threadIdx.x]);
}

// fbase[f] = the used nodes of the frames before f, fbase[n_frames] = all of them, neither beyond the workspace's node_cap
// entries (only tracks that overlap, whose malformed offsets are reported, can have more); fcur = fbase
__global__ __launch_bounds__(DVW_NT) void k_dvw_scan(DvwArgs a)
{
    __shared__ long long sh[DVW_NT / 64];
    const int nf = a.tv.n_frames;
    const long long cap = a.tv.node_cap;
    const long long carry = block_scan_array<long long, DVW_NT>(
        nf, sh, [&](int f) { return (long long)(unsigned)a.fcnt[f]; }, [&](int f, long long x) { a.fbase[f] = a.fcur[f] = (int)(x < cap ? x : cap); });
    if (threadIdx.x == 0) a.fbase[nf] = (int)(carry < cap ? carry : cap);
}

__global__ __launch_bounds__(DVW_NT) void k_dvw_scatter(DvwArgs a)
{
    __shared__ int s_h[DVW_LDS_FRAMES];
    const int nf = a.tv.n_frames;
    const bool lds = nf <= DVW_LDS_FRAMES;
    const long long nt = a.meta[0];
    int tracks = 0;
    if (lds) {
        for (int f = threadIdx.x; f < nf; f += DVW_NT) s_h[f] = 0;
        __syncthreads();
        dvw_walk_all<false>(a, nt, tracks, [&](int f, double) { atomicAdd(&s_h[f], 1); });
        __syncthreads();
        for (int f = threadIdx.x; f < nf; f += DVW_NT)
            if (s_h[f]) s_h[f] = atomicAdd(&a.fcur[f], s_h[f]);   // from here on: the workgroup's next place in the bucket
        __syncthreads();
    }
    dvw_walk_all<false>(a, nt, tracks, [&](int f, double z) {
        const int pos = lds ? atomicAdd(&s_h[f], 1) : atomicAdd(&a.fcur[f], 1);
        if (pos >= a.fbase[f] && pos < a.fbase[f + 1]) a.zb[pos] = z;
    });
}

// the cells of one pair: (row of a, b) and (row of b, a) where d_refs names the frame
template <bool LDS>
__device__ __forceinline__ void dvw_cells(const DvwArgs &a, unsigned long long *s_cell, int ra, int fa, int rb, int fb, unsigned long long inc)
{
    const int nf = a.tv.n_frames;
    if constexpr (LDS) {
        if (ra != DVW_NOROW) atomicAdd(&s_cell[ra * nf + fb], inc);
        if (rb != DVW_NOROW) atomicAdd(&s_cell[rb * nf + fa], inc);
    } else {
        if (ra != DVW_NOROW) atomicAdd(&a.cells[(size_t)ra * nf + fb], inc);
        if (rb != DVW_NOROW) atomicAdd(&a.cells[(size_t)rb * nf + fa], inc);
    }
}

template <int G, int CLS, bool LDS> __device__ __forceinline__ void dvw_pair_phase(const DvwArgs &a, long long nt, unsigned long long *s_cell, int &pairs)
{
    PGX_TRACK_LOOP(G, nt)
    {
        int o0, n;
        track_range(a.tv, t, o0, n);
        if (dvw_class(n) != CLS) continue;
        double X[3];
        if (!dvw_track(a, t, X)) continue;
        for (int i = 0; i + 1 < n; i++) {   // group-uniform
            int fa, fb;
            double z;
            if (!dvw_node<false>(a, (long long)o0 + i, X, fa, z)) continue;
            const double *ca = a.cam + (size_t)fa * DVW_CAM + DC_C;
            const double ri[3] = {ca[0] - X[0], ca[1] - X[1], ca[2] - X[2]};
            const double na = (ri[0] * ri[0] + ri[1] * ri[1]) + ri[2] * ri[2];
            const int ra = a.rowof[fa];
            for (int j = i + 1 + lane; j < n; j += G) {
                if (!dvw_node<false>(a, (long long)o0 + j, X, fb, z) || fb == fa) continue;
                const double *cb = a.cam + (size_t)fb * DVW_CAM + DC_C;
                const double rj[3] = {cb[0] - X[0], cb[1] - X[1], cb[2] - X[2]};
                const double d = (ri[0] * rj[0] + ri[1] * rj[1]) + ri[2] * rj[2];
                const double nb = (rj[0] * rj[0] + rj[1] * rj[1]) + rj[2] * rj[2];
                const double dd = d * d, nn = na * nb;
                const bool good = d > 0.0 && dd <= a.cmin2 * nn && dd >= a.cmax2 * nn;
                pairs++;
                dvw_cells<LDS>(a, s_cell, ra, fa, a.rowof[fb], fb, good ? (1ull << 32) | 1ull : 1ull);
            }
        }
    }
}

template <bool LDS> __global__ __launch_bounds__(DVW_NT) void k_dvw_pairs(DvwArgs a)
{
    __shared__ unsigned long long s_cell[LDS ? DVW_LDS_CELLS : 1];
    __shared__ int s_pairs;
    const int ncell = a.R * a.tv.n_frames;   // LDS: at most DVW_LDS_CELLS
    if (LDS)
        for (int i = threadIdx.x; i < ncell; i += DVW_NT) s_cell[i] = 0;
    if (threadIdx.x == 0) s_pairs = 0;
    __syncthreads();
    const long long nt = a.meta[0];
    int pairs = 0;
    dvw_pair_phase<64, 2, LDS>(a, nt, s_cell, pairs);
    dvw_pair_phase<16, 1, LDS>(a, nt, s_cell, pairs);
    dvw_pair_phase<4, 0, LDS>(a, nt, s_cell, pairs);
    if (pairs) atomicAdd(&s_pairs, pairs);
    __syncthreads();
    if (LDS)
        for (int i = threadIdx.x; i < ncell; i += DVW_NT)
            if (s_cell[i]) atomicAdd(&a.cells[i], s_cell[i]);
    if (threadIdx.x == 0 && s_pairs) atomicAdd(&a.report[3], s_pairs);
}

// A source candidate as the argmax sees it: good, and sb = shared << 16 | (65535 - frame), which is at least 1 (frames end at
// 65534); sb == 0: none.  The order of the sources is (good, sb) descending.
__device__ __forceinline__ bool dvw_before(int xg, unsigned long long xsb, int yg, unsigned long long ysb)
{
    return xg > yg || (xg == yg && xsb > ysb);
}

// the first candidate of the workgroup's, in every thread.  sg, ssb: DVW_NT / 64 entries each
__device__ __forceinline__ void dvw_block_first(int &g, unsigned long long &sb, int *sg, unsigned long long *ssb)
{
#pragma unroll
    for (int m = 1; m < 64; m <<= 1) {
        const int og = __shfl_xor(g, m, 64);
        const unsigned long long osb = __shfl_xor(sb, m, 64);
        if (dvw_before(og, osb, g, sb)) { g = og; sb = osb; }
    }
    if ((threadIdx.x & 63) == 0) { sg[threadIdx.x >> 6] = g; ssb[threadIdx.x >> 6] = sb; }
    __syncthreads();
    g = sg[0]; sb = ssb[0];
#pragma unroll
    for (int w = 1; w < DVW_NT / 64; w++)
        if (dvw_before(sg[w], ssb[w], g, sb)) { g = sg[w]; sb = ssb[w]; }
    __syncthreads();
}

// one more value for bin `bin` of hist from every lane with m set.  A wave whose lanes with m set all name one bin (the first
// passes, where the depths share their exponent) adds once.
__device__ __forceinline__ void dvw_hist_add(bool m, int bin, int *hist)
{
    const unsigned long long mb = __ballot(m);
    if (mb == 0) return;
    const int first = __ffsll((long long)mb) - 1;
    const int b0 = __shfl(bin, first, 64);
    if (__ballot(m && bin == b0) == mb) {
        if ((int)(threadIdx.x & 63) == first) atomicAdd(&hist[b0], __popcll(mb));
    } else if (m) {
        atomicAdd(&hist[bin], 1);
    }
}

// the bin that holds rank rk of the histogram (one bin per thread), and the rank inside it: into *s_pre and *s_rank
__device__ __forceinline__ void dvw_pick_bin(const int *hist, unsigned long long pre, long long rk, int *s_scan, unsigned long long *s_pre,
                                             long long *s_rank)
{
    const int h = hist[threadIdx.x];
    int tot;
    const int e = block_excl_scan<int, DVW_NT>(h, s_scan, tot);
    if ((long long)e <= rk && rk < (long long)e + h) {
        *s_pre = (pre << 8) | (unsigned long long)threadIdx.x;
        *s_rank = rk - e;
    }
}

// One workgroup: the patterns of ranks r0 and r1 (both < n) among the n patterns z, by eight passes of eight bits from the
// top, both ranks in every pass.
__device__ __forceinline__ void dvw_select2(const unsigned long long *z, int n, long long rk0, long long rk1, unsigned long long &out0,
                                            unsigned long long &out1, int (*s_hist)[DVW_NT], int *s_scan, unsigned long long *s_pre,
                                            long long *s_rank)
{
    unsigned long long pre0 = 0, pre1 = 0;
    for (int pass = 0; pass < 8; pass++) {
        const int sh = 56 - 8 * pass;
        s_hist[0][threadIdx.x] = s_hist[1][threadIdx.x] = 0;
        __syncthreads();
        for (int i0 = 0; i0 < n; i0 += DVW_NT) {   // the same trips in every thread: the ballots see whole waves
            const int i = i0 + threadIdx.x;
            const unsigned long long v = i < n ? z[i] : 0ull;
            const unsigned long long top = pass == 0 ? 0ull : v >> (sh + 8);   // the bits the passes before fixed
            const int bin = (int)((v >> sh) & 255ull);
            dvw_hist_add(i < n && top == pre0, bin, s_hist[0]);
            dvw_hist_add(i < n && top == pre1, bin, s_hist[1]);
        }
        __syncthreads();
        dvw_pick_bin(s_hist[0], pre0, rk0, s_scan, &s_pre[0], &s_rank[0]);
        dvw_pick_bin(s_hist[1], pre1, rk1, s_scan, &s_pre[1], &s_rank[1]);
        __syncthreads();
        pre0 = s_pre[0]; pre1 = s_pre[1];
        rk0 = s_rank[0]; rk1 = s_rank[1];
        __syncthreads();
    }
    out0 = pre0;
    out1 = pre1;
}

__global__ __launch_bounds__(DVW_NT) void k_dvw_select(DvwArgs a)
{
    static_assert(DVW_NT == 256, "one thread per bin of the radix select");
    __shared__ int s_hist[2][DVW_NT];
    __shared__ int s_scan[DVW_NT / 64];
    __shared__ unsigned long long s_pre[2];
    __shared__ long long s_rank[2];
    __shared__ int s_kg[DVW_NT / 64];
    __shared__ unsigned long long s_ksb[DVW_NT / 64];
    const double NaN = __builtin_nan("");
    const int r = blockIdx.x, nf = a.tv.n_frames, S = a.S;
    const int f = a.refs ? a.refs[r] : r;
    int32_t *views = a.views + (size_t)r * (1 + S);
    const bool known = f >= 0 && f < nf && a.cam[(size_t)f * DVW_CAM + DC_KNOWN] != 0.0;
    if (threadIdx.x == 0) views[0] = f;
    if (!known) {   // -1 throughout, no other bit
        if ((int)threadIdx.x < S) views[1 + threadIdx.x] = -1;
        if (threadIdx.x == 0) {
            a.range[2 * r] = a.range[2 * r + 1] = NaN;
            a.ref_stats[4 * r] = a.ref_stats[4 * r + 1] = a.ref_stats[4 * r + 2] = 0;
            a.ref_stats[4 * r + 3] = PGX_DVW_NOCAMERA;
        }
        if (a.pair_counts)
            for (int b = threadIdx.x; b < nf; b += DVW_NT) {
                a.pair_counts[2 * ((size_t)r * nf + b)] = 0;
                a.pair_counts[2 * ((size_t)r * nf + b) + 1] = 0;
            }
        return;
    }
    const unsigned long long *cells = a.cells + (size_t)a.rowof[f] * nf;   // the first row that names f counted for all of them

    // the candidates, and the row of pair counts
    int ncand = 0;
    for (int b = threadIdx.x; b < nf; b += DVW_NT) {
        const unsigned long long c = cells[b];
        const int shared = (int)(unsigned)c, good = (int)(unsigned)(c >> 32);
        if (a.pair_counts) {
            a.pair_counts[2 * ((size_t)r * nf + b)] = shared;
            a.pair_counts[2 * ((size_t)r * nf + b) + 1] = good;
        }
        ncand += b != f && a.cam[(size_t)b * DVW_CAM + DC_KNOWN] != 0.0 && shared >= a.min_shared;
    }
    ncand = block_sum_i(ncand, s_scan);

    // the sources: round k takes the first candidate behind the winner of round k - 1
    int pg = 0, chosen = 0;
    unsigned long long psb = 0;   // the previous winner; none in round 0
    for (int k = 0; k < S; k++) {
        int bg = 0;
        unsigned long long bsb = 0;
        if (k == chosen)   // a round without a winner ends the search
            for (int b = threadIdx.x; b < nf; b += DVW_NT) {
                const unsigned long long c = cells[b];
                const int shared = (int)(unsigned)c, good = (int)(unsigned)(c >> 32);
                const unsigned long long sb = ((unsigned long long)(unsigned)shared << 16) | (unsigned long long)(65535 - b);
                if (b == f || a.cam[(size_t)b * DVW_CAM + DC_KNOWN] == 0.0 || shared < a.min_shared) continue;
                if (k > 0 && !dvw_before(pg, psb, good, sb)) continue;
                if (dvw_before(good, sb, bg, bsb)) { bg = good; bsb = sb; }
            }
        dvw_block_first(bg, bsb, s_kg, s_ksb);
        if (bsb != 0) {
            pg = bg;
            psb = bsb;
            chosen++;
        }
        if (threadIdx.x == 0) views[1 + k] = bsb != 0 ? 65535 - (int)(bsb & 0xFFFFull) : -1;
    }

    // the range: two order statistics of the frame's bucket
    const int na = a.fcnt[f], nsel = a.fbase[f + 1] - a.fbase[f];   // equal unless tracks overlap
    double zn = NaN, zf = NaN;
    if (na >= a.min_points && nsel > 0) {
        const long long i_near = ((long long)(nsel - 1) * a.q_near_pm) / 1000, i_far = ((long long)(nsel - 1) * a.q_far_pm + 999) / 1000;
        unsigned long long pn, pf;
        dvw_select2(reinterpret_cast<const unsigned long long *>(a.zb + a.fbase[f]), nsel, i_near, i_far, pn, pf, s_hist, s_scan, s_pre, s_rank);
        zn = __longlong_as_double((long long)pn) / a.grow;
        zf = __longlong_as_double((long long)pf) * a.grow;
    }
    if (threadIdx.x == 0) {
        const bool finite = isfinite(zn) && isfinite(zf);
        a.range[2 * r] = zn;
        a.range[2 * r + 1] = zf;
        a.ref_stats[4 * r] = na;
        a.ref_stats[4 * r + 1] = ncand;
        a.ref_stats[4 * r + 2] = chosen;
        a.ref_stats[4 * r + 3] = (na < a.min_points ? PGX_DVW_FEWPOINTS : 0) | (chosen < S ? PGX_DVW_FEWVIEWS : 0) |
                                 (finite && !(zn < zf) ? PGX_DVW_NARROW : 0);
        if (finite) atomicAdd(&a.report[4], 1);
        if (chosen == S) atomicAdd(&a.report[5], 1);
        if (chosen > 0) atomicAdd(&a.report[6], 1);
    }
}

int dvw_grid(int max_tracks, int most)
{
    const long long want = ((long long)max_tracks + 3) / 4;   // a whole wave per track if every track were long
    return (int)(want < 1 ? 1 : (want > most ? most : want));
}

// the workspace, described once: a's workspace pointers (none valid for ws = nullptr) and the bytes
size_t dvw_carve(DvwArgs &a, void *ws)
{
    WsCarver w(ws);
    const size_t nf = a.tv.n_frames, nc = a.tv.node_cap < 1 ? 1 : (size_t)a.tv.node_cap;
    a.cells = w.take<unsigned long long>((size_t)a.R * nf * sizeof(unsigned long long));
    a.cam = w.take<double>(nf * DVW_CAM * sizeof(double));
    a.zb = w.take<double>(nc * sizeof(double));
    a.rowof = w.take<int32_t>(nf * sizeof(int32_t));
    a.fcnt = w.take<int32_t>(nf * sizeof(int32_t));
    a.fbase = w.take<int32_t>((nf + 1) * sizeof(int32_t));
    a.fcur = w.take<int32_t>(nf * sizeof(int32_t));
    a.meta = w.take<int32_t>(256);
    return w.total();
}

} // namespace

size_t pgx_dense_views_ws_bytes(const DvwArgs &a)
{
    DvwArgs b = a;
    return dvw_carve(b, nullptr);
}

void pgx_launch_dense_views(pgx_ctx *ctx, hipStream_t s, DvwArgs a, void *ws)
{
    dvw_carve(a, ws);
    const int grid = dvw_grid(a.tv.max_tracks, DVW_GRID_MAX), pgrid = dvw_grid(a.tv.max_tracks, DVW_PAIR_GRID_MAX);
    // the profiling groups of the stage's parts (pgx_profile_get; nothing is recorded while profiling is off)
    {
        ProfScope ps(ctx, "dense_views_nodes", s);
        hipLaunchKernelGGL(k_dvw_frames, dim3(1), dim3(DVW_NT), 0, s, a);
        hipLaunchKernelGGL(k_dvw_count, dim3(grid), dim3(DVW_NT), 0, s, a);
        hipLaunchKernelGGL(k_dvw_scan, dim3(1), dim3(DVW_NT), 0, s, a);
        hipLaunchKernelGGL(k_dvw_scatter, dim3(grid), dim3(DVW_NT), 0, s, a);
    }
    {
        ProfScope ps(ctx, "dense_views_pairs", s);
        (void)hipMemsetAsync(a.cells, 0, (size_t)a.R * a.tv.n_frames * sizeof(unsigned long long), s);
        if ((long long)a.R * a.tv.n_frames <= DVW_LDS_CELLS) hipLaunchKernelGGL(k_dvw_pairs<true>, dim3(pgrid), dim3(DVW_NT), 0, s, a);
        else hipLaunchKernelGGL(k_dvw_pairs<false>, dim3(pgrid), dim3(DVW_NT), 0, s, a);
    }
    {
        ProfScope ps(ctx, "dense_views_select", s);
        hipLaunchKernelGGL(k_dvw_select, dim3(a.R), dim3(DVW_NT), 0, s, a);
    }
}
