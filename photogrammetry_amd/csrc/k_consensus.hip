// k_consensus.hip -- track consensus: a deterministic two-view RANSAC per track that drops the observations which disagree
// with the track's own best two-view point, and the ordered compaction of the graph (pgx_track_consensus_dev; the rule is
// in include/pgx.h).  Not in the reference, whose tracks span one image pair.
//
// Kernels (eight launches, all on the caller's stream; n_tracks is read on the device):
//   k_cns_frames       one workgroup: per frame M, C = -(M^-1 p4), sign det M, known and M^-1 in one table row, the slot ->
//                      frame inverse, the number of tracks to process (PGX_ST_CNS_CAP) and the zeroed counters
//   k_cns_score<G, C>  persistent, grid-stride over the tracks of one length class, one launch per class (k_tri_tracks'
//                      classes: more than 32 nodes a whole wave, 9..32 nodes 16 lanes, 0..8 nodes 4 lanes; one kernel with
//                      the three phases spilled scalars).  Lanes over OBSERVATIONS: lane l of a group owns the
//                      observations l and l + G, which is every observation of a track of the two short classes, and
//                      holds them in registers (camera rows, centre, pixel, sign).  A long track's lanes read their
//                      observations again from the frame table per predicate (192 B rows, cache resident): holding two
//                      of them as well spilled scalars, and tests/test_consensus_codegen.py pins zero spills.  The group
//                      walks the hypotheses in order; a hypothesis is computed
//                      redundantly in the G lanes from the two rays' 48-byte records (written once per track, read at
//                      group-uniform addresses), and its inliers are counted by a ballot and a population count: no shuffle
//                      and no floating-point reduction, so the key is the same for any lane mapping.  The winner is
//                      recomputed from its pair (the same function on the same bits) for the keep flags and the point.
//   k_cns_scan_reduce  per block of CNS_SCAN_ITEMS tracks the surviving tracks and nodes
//   k_cns_scan_sums    one workgroup: the exclusive scans of the block sums (block_scan_array, tracks then nodes), the totals,
//                      d_summary_out, d_report and the end of the offsets
//   k_cns_scan_apply   per block the exclusive scan of its tracks: d_track_map and the offsets of the surviving tracks
//   k_cns_write        grid-stride over the tracks in the same classes: a kept node goes to its rank inside the track (a
//                      ballot prefix), the track's point and flag to its new index, d_track_of is rewritten
// Counters are integers throughout (LDS, then one atomic per workgroup).  DESIGN.md section 22 has the measurements.
#include "pgx_stage_args.h"

namespace {

constexpr int CNS_NT = 256;             // threads per workgroup of every kernel here
constexpr int CNS_GRID_MAX = 1024;      // workgroups of k_cns_score and k_cns_write (4 per CU), at most
constexpr int CNS_SCAN_PER_THREAD = 4;  // consecutive tracks per thread of a scan block
constexpr int CNS_SCAN_ITEMS = 1024;    // tracks per scan block (CNS_NT * CNS_SCAN_PER_THREAD)
constexpr int CNS_CAM = 24;             // doubles per frame: M (9), C (3), sign det M, known (1 / 0), M^-1 (9), unused
constexpr int CAM_C = 9, CAM_SGN = 12, CAM_KNOWN = 13, CAM_INV = 14;
constexpr int CNS_RAY = 6;              // doubles per known observation of a track: ray (3), centre (3)
// counters (ints) behind meta[0] = tracks to process
constexpr int CT_NODES_IN = 1, CT_OUTLIERS = 2, CT_NOCONS = 3, CT_SHORT = 4, CT_UNDECIDED = 5, CT_LONGEST = 6;

static_assert(CNS_SCAN_ITEMS == CNS_NT * CNS_SCAN_PER_THREAD, "a scan block is CNS_SCAN_PER_THREAD tracks per thread");

// a known observation as its owner lane holds it
struct Obs {
    double m[9], c[3], u, v, sgn;
};

// node o: 0 = invalid, 1 = valid in an unknown frame, 2 = known (x filled)
__device__ __forceinline__ int cns_obs(const CnsArgs &a, long long o, Obs &x, int &f)
{
    f = a.tv.nodes[2 * o];
    const int k = a.tv.nodes[2 * o + 1];
    if (!node_ok(a.tv, f, k)) return 0;
    const double *c = a.cam + (size_t)f * CNS_CAM;
    if (c[CAM_KNOWN] == 0.0) return 1;
    node_keypoint(a.tv, f, k, x.u, x.v);
#pragma unroll
    for (int i = 0; i < 9; i++) x.m[i] = c[i];
#pragma unroll
    for (int i = 0; i < 3; i++) x.c[i] = c[CAM_C + i];
    x.sgn = c[CAM_SGN];
    return 2;
}

__device__ __forceinline__ double dot3(const double *x, const double *y) { return (x[0] * y[0] + x[1] * y[1]) + x[2] * y[2]; }

// the hypothesis of the pair of ray records (ri, rj): false = rejected, else X = the midpoint relative to C_i
__device__ __forceinline__ bool cns_hyp(const double *ri, const double *rj, double cos2, double (&X)[3])
{
    double di[3], dj[3], w0[3];
#pragma unroll
    for (int k = 0; k < 3; k++) {
        di[k] = ri[k];
        dj[k] = rj[k];
        w0[k] = ri[3 + k] - rj[3 + k];
    }
    const double a = dot3(di, di), b = dot3(di, dj), c = dot3(dj, dj), dd = dot3(di, w0), e = dot3(dj, w0);
    const double den = a * c - b * b;
    if (b > 0.0 && b * b >= cos2 * (a * c)) return false;
    if (!(den > 0.0)) return false;
    const double s = (b * e - c * dd) / den, tt = (a * e - b * dd) / den;
    if (!(s > 0.0 && tt > 0.0)) return false;
#pragma unroll
    for (int k = 0; k < 3; k++) X[k] = 0.5 * (s * di[k] + (tt * dj[k] - w0[k]));
    return true;
}

// the predicate: X relative to Ci, seen by observation x
__device__ __forceinline__ bool cns_inlier(const Obs &x, const double (&X)[3], const double *Ci, double px)
{
    const double y0 = X[0] + (Ci[0] - x.c[0]), y1 = X[1] + (Ci[1] - x.c[1]), y2 = X[2] + (Ci[2] - x.c[2]);
    const double h0 = (x.m[0] * y0 + x.m[1] * y1) + x.m[2] * y2;
    const double h1 = (x.m[3] * y0 + x.m[4] * y1) + x.m[5] * y2;
    const double w = (x.m[6] * y0 + x.m[7] * y1) + x.m[8] * y2;
    const double ap = h0 - x.u * w, bp = h1 - x.v * w, ep = px * w;
    return x.sgn * w > 0.0 && ap * ap + bp * bp <= ep * ep;
}

// the G lanes' bits of a wave-wide ballot, lane 0 of the group in bit 0
template <int G> __device__ __forceinline__ unsigned long long group_ballot(bool p)
{
    const unsigned long long b = __ballot(p);
    if (G == 64) return b;
    return (b >> ((threadIdx.x & 63) & ~(G - 1))) & ((1ull << (G & 63)) - 1ull);
}

__device__ __forceinline__ int cns_class(int n) { return n > 32 ? 2 : (n > 8 ? 1 : 0); }

// one round of the staging pass: this lane's observation m (or none), its ray record at the next position among the known
template <int G>
__device__ __forceinline__ int cns_stage(const CnsArgs &a, int o0, int n, int m, int lane, Obs &x, int &nk, int &nvalid)
{
    int f = 0;
    const int kind = m < n ? cns_obs(a, (long long)o0 + m, x, f) : -1;
    if (kind == 0) atomicOr(a.status, (int)PGX_ST_CNS_NODE);
    const unsigned long long kb = group_ballot<G>(kind == 2), vb = group_ballot<G>(kind >= 1);
    if (kind == 2) {
        const int pos = nk + __popcll(kb & ((1ull << lane) - 1ull));
        const double *iv = a.cam + (size_t)f * CNS_CAM + CAM_INV;
        double *r = a.rays + ((size_t)o0 + pos) * CNS_RAY;
#pragma unroll
        for (int k = 0; k < 3; k++) {
            r[k] = x.sgn * ((iv[3 * k] * x.u + iv[3 * k + 1] * x.v) + iv[3 * k + 2]);
            r[3 + k] = x.c[k];
        }
    }
    nk += __popcll(kb);
    nvalid += __popcll(vb);
    return kind;
}

// the inliers of the hypothesis (X, Ci) among the group's observations; in0 / in1: this lane's first two
template <int G, int CLS>
__device__ __forceinline__ int cns_count(const CnsArgs &a, int o0, int n, int lane, const Obs &r0, int k0, const Obs &r1, int k1,
                                         const double (&X)[3], const double *Ci, bool &in0, bool &in1)
{
    int cnt = 0;
    if (CLS != 2) {
        in0 = k0 == 2 && cns_inlier(r0, X, Ci, a.inlier_px);
        in1 = k1 == 2 && cns_inlier(r1, X, Ci, a.inlier_px);
        cnt = __popcll(group_ballot<G>(in0)) + __popcll(group_ballot<G>(in1));
    }
    if (CLS == 2)
        for (int b = 0; b < n; b += G) {
            Obs x;
            int f;
            const bool in = b + lane < n && cns_obs(a, (long long)o0 + b + lane, x, f) == 2 && cns_inlier(x, X, Ci, a.inlier_px);
            cnt += __popcll(group_ballot<G>(in));
        }
    return cnt;
}

// every track of length class CLS, G lanes per track
template <int G, int CLS> __device__ void cns_phase(const CnsArgs &a, long long nt, int (&acc)[8])
{
    const double NaN = __builtin_nan("");
    PGX_TRACK_LOOP(G, nt)
    {
        int o0, n;
        const bool wellformed = track_range(a.tv, t, o0, n);
        if (cns_class(n) != CLS) continue;
        if (!wellformed && lane == 0) atomicOr(a.status, (int)PGX_ST_CNS_NODE);

        // staging: the observations' kinds, the known ones' ray records in d_nodes order
        Obs r0, r1;
        int nk = 0, nvalid = 0;
        const int k0 = CLS != 2 ? cns_stage<G>(a, o0, n, lane, lane, r0, nk, nvalid) : -1;
        const int k1 = CLS != 2 ? cns_stage<G>(a, o0, n, G + lane, lane, r1, nk, nvalid) : -1;
        if (CLS == 2)
            for (int b = 0; b < n; b += G) {
                Obs x;
                cns_stage<G>(a, o0, n, b + lane, lane, x, nk, nvalid);
            }
        __threadfence_block();   // the group's lanes read each other's ray records

        int bits = 0, inl = 0, hwin = -1, kept = nvalid;
        double X[3] = {NaN, NaN, NaN}, W[3] = {NaN, NaN, NaN};   // the winner's point relative to C_i, and in world coordinates
        bool in0 = true, in1 = true;
        unsigned long long best = 0;
        int bi = 0, bj = 1;
        const double *rays = a.rays + (size_t)o0 * CNS_RAY, *ci = rays + 3;
        if (nk < 2) {
            bits = PGX_CNS_FEWVIEWS;
        } else {
            const long long np = (long long)nk * (nk - 1) / 2;
            const bool exhaustive = np <= a.max_hyp;
            const int nh = exhaustive ? (int)np : a.max_hyp;
            int i = 0, j = 0;
            for (int h = 0; h < nh; h++) {
                if (exhaustive) {
                    if (++j >= nk) { i++; j = i + 1; }
                } else {
                    uint64_t st = ransac_stream(a.seed, (int)t, h);
                    int id[2];
                    ransac_draw(st, nk, 2, id);
                    i = id[0] < id[1] ? id[0] : id[1];
                    j = id[0] < id[1] ? id[1] : id[0];
                }
                double Y[3];
                const double *ri = rays + (size_t)i * CNS_RAY;
                if (!cns_hyp(ri, rays + (size_t)j * CNS_RAY, a.cos2, Y)) continue;
                bool p0, p1;
                const unsigned long long key = ransac_key(true, cns_count<G, CLS>(a, o0, n, lane, r0, k0, r1, k1, Y, ri + 3, p0, p1), h);
                if (key > best) { best = key; bi = i; bj = j; }
            }
            if (best == 0) {
                bits = PGX_CNS_LOWPARALLAX;
            } else {
                // the winner again from its pair: the same function on the same bits
                const double *ri = rays + (size_t)bi * CNS_RAY;
                ci = ri + 3;
                cns_hyp(ri, rays + (size_t)bj * CNS_RAY, a.cos2, X);
                inl = cns_count<G, CLS>(a, o0, n, lane, r0, k0, r1, k1, X, ci, in0, in1);
                hwin = ransac_key_index(best);
                kept = nvalid - (nk - inl);
                if (inl < a.min_inliers) bits = PGX_CNS_NOCONSENSUS;
#pragma unroll
                for (int k = 0; k < 3; k++) W[k] = X[k] + ci[k];
            }
        }
        const bool undecided = (bits & (PGX_CNS_FEWVIEWS | PGX_CNS_LOWPARALLAX)) != 0;

        // keep flags: a node in an unknown frame always, a known one unless the winner rejects it
        if (CLS != 2 && lane < n) a.keep[(size_t)o0 + lane] = k0 == 1 || (k0 == 2 && (undecided || in0));
        if (CLS != 2 && G + lane < n) a.keep[(size_t)o0 + G + lane] = k1 == 1 || (k1 == 2 && (undecided || in1));
        if (CLS == 2)
            for (int b = 0; b < n; b += G) {
                if (b + lane >= n) continue;
                Obs x;
                int f;
                const int kd = cns_obs(a, (long long)o0 + b + lane, x, f);
                a.keep[(size_t)o0 + b + lane] = kd == 1 || (kd == 2 && (undecided || cns_inlier(x, X, ci, a.inlier_px)));
            }

        if (lane == 0) {
            const int outliers = bits == 0 ? nk - inl : 0;
            if (bits & PGX_CNS_NOCONSENSUS) {
                kept = 0;
            } else if (kept < a.min_len) {
                bits |= PGX_CNS_SHORT;
                kept = 0;
            }
            a.kept[t] = kept;
            a.stats[4 * t + 0] = nk;
            a.stats[4 * t + 1] = inl;
            a.stats[4 * t + 2] = hwin;
            a.stats[4 * t + 3] = bits;
            const bool point = !undecided;
            a.xyz[3 * t + 0] = point ? W[0] : NaN;
            a.xyz[3 * t + 1] = point ? W[1] : NaN;
            a.xyz[3 * t + 2] = point ? W[2] : NaN;
            acc[CT_NODES_IN] += n;
            acc[CT_OUTLIERS] += outliers;
            acc[CT_NOCONS] += (bits & PGX_CNS_NOCONSENSUS) != 0;
            acc[CT_SHORT] += (bits & PGX_CNS_SHORT) != 0;
            acc[CT_UNDECIDED] += undecided;
            acc[CT_LONGEST] = kept > acc[CT_LONGEST] ? kept : acc[CT_LONGEST];
        }
    }
}

__global__ __launch_bounds__(CNS_NT) void k_cns_frames(CnsArgs a)
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
        const double det = (m00 * k00 + m01 * k01) + m02 * k02;
        double *c = a.cam + (size_t)f * CNS_CAM;
        c[0] = m00; c[1] = m01; c[2] = m02; c[3] = m10; c[4] = m11; c[5] = m12; c[6] = m20; c[7] = m21; c[8] = m22;
        double *iv = c + CAM_INV;
        iv[0] = k00 / det; iv[1] = k10 / det; iv[2] = k20 / det;
        iv[3] = k01 / det; iv[4] = k11 / det; iv[5] = k21 / det;
        iv[6] = k02 / det; iv[7] = k12 / det; iv[8] = k22 / det;
#pragma unroll
        for (int r = 0; r < 3; r++) c[CAM_C + r] = -((iv[3 * r] * p[3] + iv[3 * r + 1] * p[7]) + iv[3 * r + 2] * p[11]);
        c[CAM_SGN] = det > 0.0 ? 1.0 : -1.0;
        c[CAM_KNOWN] = fin && det != 0.0 ? 1.0 : 0.0;
        c[CNS_CAM - 1] = 0.0;
        a.tv.inv[f] = -1;
    }
    if (threadIdx.x == 0) a.meta[0] = clamp_tracks(a.tv, a.status, PGX_ST_CNS_CAP);
    if (threadIdx.x >= 1 && threadIdx.x < 8) a.meta[threadIdx.x] = 0;
    __syncthreads();
    build_slot_inverse(a.tv, a.status, PGX_ST_CNS_DUP);
}

template <int G, int CLS> __global__ __launch_bounds__(CNS_NT) void k_cns_score(CnsArgs a)
{
    __shared__ int s_acc[8];
    if (threadIdx.x < 8) s_acc[threadIdx.x] = 0;
    __syncthreads();
    const long long nt = a.meta[0];
    int acc[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    cns_phase<G, CLS>(a, nt, acc);
#pragma unroll
    for (int k = 1; k < CT_LONGEST; k++)
        if (acc[k]) atomicAdd(&s_acc[k], acc[k]);
    if (acc[CT_LONGEST]) atomicMax(&s_acc[CT_LONGEST], acc[CT_LONGEST]);
    __syncthreads();
    if (threadIdx.x >= 1 && threadIdx.x < CT_LONGEST && s_acc[threadIdx.x]) atomicAdd(&a.meta[threadIdx.x], s_acc[threadIdx.x]);
    if (threadIdx.x == CT_LONGEST && s_acc[CT_LONGEST]) atomicMax(&a.meta[CT_LONGEST], s_acc[CT_LONGEST]);
}

// this thread's CNS_SCAN_PER_THREAD tracks of scan block blockIdx.x: their surviving-track and node counts
__device__ __forceinline__ void scan_items(const CnsArgs &a, long long nt, int (&kp)[CNS_SCAN_PER_THREAD], int &tracks, int &nodes)
{
    const long long t0 = (long long)blockIdx.x * CNS_SCAN_ITEMS + (long long)threadIdx.x * CNS_SCAN_PER_THREAD;
    tracks = 0;
    nodes = 0;
#pragma unroll
    for (int i = 0; i < CNS_SCAN_PER_THREAD; i++) {
        kp[i] = t0 + i < nt ? a.kept[t0 + i] : 0;
        tracks += kp[i] > 0;
        nodes += kp[i];
    }
}

__global__ __launch_bounds__(CNS_NT) void k_cns_scan_reduce(CnsArgs a)
{
    __shared__ int sh[4];
    int kp[CNS_SCAN_PER_THREAD], tracks, nodes;
    scan_items(a, a.meta[0], kp, tracks, nodes);
    tracks = block_sum_i(tracks, sh);
    nodes = block_sum_i(nodes, sh);
    if (threadIdx.x == 0) {
        a.bsum[2 * (size_t)blockIdx.x] = tracks;
        a.bsum[2 * (size_t)blockIdx.x + 1] = nodes;
    }
}

// The surviving tracks and their nodes are scanned one after the other, not packed into one 64-bit value as the track graph's
// are: tracks whose offsets overlap (malformed, reported, but not rejected) can keep more than 2^32 nodes between them, and a
// carry out of the node count must not reach the track index that off_out and map are written at.
__global__ __launch_bounds__(CNS_NT) void k_cns_scan_sums(CnsArgs a, int nblk)
{
    __shared__ int sh[CNS_NT / 64];
    // the block sums are (tracks, nodes) pairs: each half in place, CNS_NT blocks at a time with a carry
    const int cx = block_scan_array<int, CNS_NT>(a.bsum, a.bsum, nblk, sh, 2);
    const int cy = block_scan_array<int, CNS_NT>(a.bsum + 1, a.bsum + 1, nblk, sh, 2);
    if (threadIdx.x == 0) {
        a.off_out[cx] = cy;
        const int32_t *si = a.tv.track_summary;
        a.summary_out[0] = cx;
        a.summary_out[1] = cy;
        a.summary_out[2] = si[2];
        a.summary_out[3] = si[3];
        a.summary_out[4] = si[4];
        a.summary_out[5] = a.meta[CT_LONGEST];
        a.summary_out[6] = si[6];
        a.summary_out[7] = 0;
        a.report[0] = a.meta[0];
        a.report[1] = cx;
        a.report[2] = a.meta[CT_NODES_IN];
        a.report[3] = cy;
        a.report[4] = a.meta[CT_OUTLIERS];
        a.report[5] = a.meta[CT_NOCONS];
        a.report[6] = a.meta[CT_SHORT];
        a.report[7] = a.meta[CT_UNDECIDED];
    }
}

__global__ __launch_bounds__(CNS_NT) void k_cns_scan_apply(CnsArgs a)
{
    __shared__ int sh[CNS_NT / 64];
    const long long nt = a.meta[0];
    int kp[CNS_SCAN_PER_THREAD], x, y, tot;
    scan_items(a, nt, kp, x, y);
    x = a.bsum[2 * (size_t)blockIdx.x] + block_excl_scan<int, CNS_NT>(x, sh, tot);
    y = a.bsum[2 * (size_t)blockIdx.x + 1] + block_excl_scan<int, CNS_NT>(y, sh, tot);
    const long long t0 = (long long)blockIdx.x * CNS_SCAN_ITEMS + (long long)threadIdx.x * CNS_SCAN_PER_THREAD;
#pragma unroll
    for (int i = 0; i < CNS_SCAN_PER_THREAD; i++) {
        if (t0 + i >= nt) break;
        a.map[t0 + i] = kp[i] > 0 ? x : -1;
        if (kp[i] > 0) {
            a.off_out[x] = y;
            x++;
            y += kp[i];
        }
    }
}

template <int G, int CLS> __device__ void cns_write_phase(const CnsArgs &a, long long nt)
{
    PGX_TRACK_LOOP(G, nt)
    {
        int o0, n;
        track_range(a.tv, t, o0, n);
        if (cns_class(n) != CLS) continue;
        const int nw = a.map[t];
        long long at = nw >= 0 ? a.off_out[nw] : 0;
        for (int b = 0; b < n; b += G) {
            const bool act = b + lane < n;
            const long long o = (long long)o0 + b + lane;
            const int f = act ? a.tv.nodes[2 * o] : 0, k = act ? a.tv.nodes[2 * o + 1] : 0;
            const bool kp = act && nw >= 0 && a.keep[o];
            const unsigned long long kb = group_ballot<G>(kp);
            // tracks that overlap (malformed offsets between them, already reported) can keep more nodes than there are
            const unsigned long long pos = (unsigned long long)(at + __popcll(kb & ((1ull << lane) - 1ull)));
            if (kp && pos < (unsigned long long)a.tv.node_cap) {
                a.nodes_out[2 * pos] = f;
                a.nodes_out[2 * pos + 1] = k;
            }
            if (a.track_of && act && node_ok(a.tv, f, k)) a.track_of[(size_t)f * a.tv.stride + k] = nw < 0 ? -1 : (kp ? nw : -3);
            at += __popcll(kb);
        }
        if (lane == 0 && nw >= 0) {
            a.xyz_out[3 * (size_t)nw + 0] = a.xyz[3 * t + 0];
            a.xyz_out[3 * (size_t)nw + 1] = a.xyz[3 * t + 1];
            a.xyz_out[3 * (size_t)nw + 2] = a.xyz[3 * t + 2];
            a.flags_out[nw] = (a.stats[4 * t + 3] & (PGX_CNS_FEWVIEWS | PGX_CNS_LOWPARALLAX)) ? PGX_TRI_FEWVIEWS : 0;
        }
    }
}

__global__ __launch_bounds__(CNS_NT) void k_cns_write(CnsArgs a)
{
    const long long nt = a.meta[0];
    cns_write_phase<64, 2>(a, nt);
    cns_write_phase<16, 1>(a, nt);
    cns_write_phase<4, 0>(a, nt);
}

int cns_grid(int max_tracks)
{
    const long long want = ((long long)max_tracks + 3) / 4;   // a whole wave per track if every track were long
    return (int)(want < 1 ? 1 : (want > CNS_GRID_MAX ? CNS_GRID_MAX : want));
}

int cns_scan_blocks(int max_tracks) { return max_tracks < 1 ? 1 : (int)(((long long)max_tracks + CNS_SCAN_ITEMS - 1) / CNS_SCAN_ITEMS); }

// the workspace, described once: a's workspace pointers (none valid for ws = nullptr) and the bytes
size_t cns_carve(CnsArgs &a, void *ws)
{
    WsCarver w(ws);
    const int n_frames = a.tv.n_frames, max_tracks = a.tv.max_tracks;
    const long long node_cap = a.tv.node_cap;
    const size_t mt = max_tracks < 1 ? 1 : max_tracks, nc = node_cap < 1 ? 1 : (size_t)node_cap;
    a.cam = w.take<double>((size_t)n_frames * CNS_CAM * sizeof(double));
    a.rays = w.take<double>(nc * CNS_RAY * sizeof(double));
    a.xyz = w.take<double>(mt * 3 * sizeof(double));
    a.kept = w.take<int32_t>(mt * sizeof(int32_t));
    a.bsum = w.take<int32_t>((size_t)cns_scan_blocks(max_tracks) * 2 * sizeof(int32_t));
    a.keep = w.take<int8_t>(nc);
    a.tv.inv = w.take<int32_t>((size_t)n_frames * sizeof(int32_t));
    a.meta = w.take<int32_t>(256);
    return w.total();
}

} // namespace

size_t pgx_consensus_ws_bytes(const CnsArgs &a)
{
    CnsArgs b = a;
    return cns_carve(b, nullptr);
}

void pgx_launch_consensus(pgx_ctx *ctx, hipStream_t s, CnsArgs a, void *ws)
{
    a.min_len = a.min_len < 1 ? 1 : a.min_len;
    cns_carve(a, ws);
    const int grid = cns_grid(a.tv.max_tracks), nblk = cns_scan_blocks(a.tv.max_tracks);
    // the profiling groups of the stage's parts (pgx_profile_get; nothing is recorded while profiling is off)
    {
        ProfScope ps(ctx, "consensus_frames", s);
        hipLaunchKernelGGL(k_cns_frames, dim3(1), dim3(CNS_NT), 0, s, a);
    }
    {
        ProfScope ps(ctx, "consensus_score", s);
        hipLaunchKernelGGL((k_cns_score<64, 2>), dim3(grid), dim3(CNS_NT), 0, s, a);   // the longest tracks first
        hipLaunchKernelGGL((k_cns_score<16, 1>), dim3(grid), dim3(CNS_NT), 0, s, a);
        hipLaunchKernelGGL((k_cns_score<4, 0>), dim3(grid), dim3(CNS_NT), 0, s, a);
    }
    {
        ProfScope ps(ctx, "consensus_scan", s);
        hipLaunchKernelGGL(k_cns_scan_reduce, dim3(nblk), dim3(CNS_NT), 0, s, a);
        hipLaunchKernelGGL(k_cns_scan_sums, dim3(1), dim3(CNS_NT), 0, s, a, nblk);
        hipLaunchKernelGGL(k_cns_scan_apply, dim3(nblk), dim3(CNS_NT), 0, s, a);
    }
    {
        ProfScope ps(ctx, "consensus_write", s);
        hipLaunchKernelGGL(k_cns_write, dim3(grid), dim3(CNS_NT), 0, s, a);
    }
}
