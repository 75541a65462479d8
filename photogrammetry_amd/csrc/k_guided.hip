// k_guided.hip -- epipolar-guided exact matching (include/pgx.h: pgx_knn_guided_batch_dev, pgx_match_guided_batch_dev,
// pgx_knn_guided).  Per image pair (a, b) with fundamental matrix F: a row i of frame a may only match the columns j of frame b
// whose keypoint lies within `band` pixels of the row's epipolar line l = F^T h_a(i); the admissibility predicate is the exact
// double expression of include/pgx.h, evaluated with no contraction (-ffp-contract=off and the pragma below).
//
// Three steps per chunk of image pairs:
//   1. k_guided_slots: the frames of the chunk get one workspace slot each (an open-addressing table keyed by frame number),
//      so that a frame shared by many pairs (64 frames against 2016 pairs) is bucketed once;
//   2. k_guided_bucket: one workgroup per slot puts the frame's keypoints into a uniform grid over their bounding box, square
//      cells of 2^s pixels, cell-major (column of cells first), about two keypoints per cell.  Every entry is one 64-bit word:
//      index (20 bits) and both coordinates offset by 2^20 (21 bits each).  A used coordinate outside [-2^20, 2^20) marks the
//      slot bad (every pair that uses it rejects all rows) and sets PGX_ST_BADARG;
//   3. k_guided_walk: one thread per row, rows in frame a's cell order so that the lanes of a wavefront hold nearby lines.  A
//      line closer to horizontal walks the columns of cells: per column the v interval the band can reach over the column's u
//      range is computed in double (approximate reciprocal and root), padded, clamped to the box and cut to INTEGER bounds (keypoints sit on integers), and the
//      cell-major layout makes the cells of that interval one contiguous run of entries.  A steeper line walks the rows of cells
//      with the roles of u and v swapped, cell by cell.  Integer bounds and power-of-two cells make the cell map exact and
//      monotone, so the walk never misses a cell that holds an admissible keypoint and visits every cell at most once.  Each
//      candidate is decided by the exact predicate; admissible ones get the xor + popcount distance and enter the row's top-2
//      as (distance << 20 | column) keys, and the column side as a global atomic min of (distance << 20 | row).
// The NN lists reuse k_knn.hip's selection (pgx_launch_knn_select), so the acceptance rules are those of pgx_match_nn_batch_dev.
#include "pgx_pairlist.h"

#include <climits>
#include <cmath>

namespace {

constexpr int GB = 256;            // threads per workgroup of every kernel here
constexpr int HDR = 16;            // ints of a slot header
constexpr int GUIDED_MAX_CELLS = 8192; // LDS counters of the bucketing pass
constexpr int COORD_LIM = 1 << 20; // used coordinates must lie in [-2^20, 2^20)

// slot header fields
enum { H_BAD = 0, H_N, H_MINX, H_MINY, H_MAXX, H_MAXY, H_SHIFT, H_GX, H_GY };

// the workspace of one chunk (laid out by guided_layout on the host)
struct GuidedWs {
    int *cnt;        // [1] slots in use
    int *tab_key;    // [H] frame number or -1
    int *tab_slot;   // [H] slot of the frame at that table position
    int *side_pos;   // [2M] table position of pairlist entry e
    int *slot_frame; // [2M] frame of slot s
    char *slots;     // [2M] x slot_bytes: header, cell offsets [cells + 1], entries [max_n] (uint64)
    int H, cells_cap;
    size_t head, slot_bytes, off_offsets, off_entries;
};

struct SlotView {
    const int *hdr;
    const int *off;
    const unsigned long long *ent;
};

__device__ __forceinline__ SlotView slot_view(const GuidedWs &w, int s)
{
    const char *base = w.slots + (size_t)s * w.slot_bytes;
    return {reinterpret_cast<const int *>(base), reinterpret_cast<const int *>(base + w.off_offsets),
            reinterpret_cast<const unsigned long long *>(base + w.off_entries)};
}

__device__ __forceinline__ unsigned long long pack_entry(int i, int x, int y)
{
    return (unsigned long long)(uint32_t)i | ((unsigned long long)(uint32_t)(x + COORD_LIM) << 20) |
           ((unsigned long long)(uint32_t)(y + COORD_LIM) << 41);
}

// ---- 1. one slot per distinct frame of the chunk ------------------------------------------------------------------------
__global__ __launch_bounds__(GB) void k_guided_slots(const int32_t *__restrict__ pairlist, int E, GuidedWs w)
{
    const int e = blockIdx.x * GB + threadIdx.x;
    if (e >= E) return;
    const int f = pairlist[e];
    int h = (int)(((uint32_t)f * 2654435761u) & (uint32_t)(w.H - 1));
    for (;;) { // the table holds at least twice as many positions as entries: a free one is always found
        const int old = atomicCAS(&w.tab_key[h], -1, f);
        if (old == -1) {
            const int s = atomicAdd(w.cnt, 1);
            w.tab_slot[h] = s;
            w.slot_frame[s] = f;
            break;
        }
        if (old == f) break;
        h = (h + 1) & (w.H - 1);
    }
    w.side_pos[e] = h;
}

// ---- 2. the grid of one frame --------------------------------------------------------------------------------------------
__global__ __launch_bounds__(GB) void k_guided_bucket(const pgx_keypoint *__restrict__ kp, const int32_t *__restrict__ counts, int S,
                                                      int max_n, GuidedWs w, int *status)
{
    __shared__ int cell_n[GUIDED_MAX_CELLS];
    __shared__ int red[6][GB];
    __shared__ int geo[4]; // shift, gx, gy, cells
    const int s = blockIdx.x, tid = threadIdx.x;
    if (s >= *w.cnt) return;
    const int f = w.slot_frame[s];
    const int n = pgx_clamp_count(counts[f], max_n);
    char *base = w.slots + (size_t)s * w.slot_bytes;
    int *hdr = reinterpret_cast<int *>(base);
    int *off = reinterpret_cast<int *>(base + w.off_offsets);
    unsigned long long *ent = reinterpret_cast<unsigned long long *>(base + w.off_entries);
    const pgx_keypoint *K = kp + (size_t)f * S;

    int mnx = INT_MAX, mny = INT_MAX, mxx = INT_MIN, mxy = INT_MIN, bad = 0;
    for (int i = tid; i < n; i += GB) {
        const int x = K[i].x, y = K[i].y;
        bad |= (x < -COORD_LIM) | (x >= COORD_LIM) | (y < -COORD_LIM) | (y >= COORD_LIM);
        mnx = min(mnx, x); mny = min(mny, y); mxx = max(mxx, x); mxy = max(mxy, y);
    }
    red[0][tid] = mnx; red[1][tid] = mny; red[2][tid] = mxx; red[3][tid] = mxy; red[4][tid] = bad;
    __syncthreads();
    for (int h = GB / 2; h > 0; h >>= 1) {
        if (tid < h) {
            red[0][tid] = min(red[0][tid], red[0][tid + h]);
            red[1][tid] = min(red[1][tid], red[1][tid + h]);
            red[2][tid] = max(red[2][tid], red[2][tid + h]);
            red[3][tid] = max(red[3][tid], red[3][tid + h]);
            red[4][tid] |= red[4][tid + h];
        }
        __syncthreads();
    }
    if (red[4][0]) {
        if (tid == 0) {
            hdr[H_BAD] = 1;
            hdr[H_N] = n;
            atomicOr(status, (int)PGX_ST_BADARG);
        }
        return;
    }
    const int minx = n ? red[0][0] : 0, miny = n ? red[1][0] : 0, maxx = n ? red[2][0] : 0, maxy = n ? red[3][0] : 0;
    if (tid == 0) {
        // the smallest power-of-two cell with at most max(1, n / 2) cells (capped by the workspace): about two keypoints a cell
        const int target = min(max(1, n / 2), w.cells_cap);
        int sh = 0, gx = 1, gy = 1;
        for (; sh <= 21; sh++) {
            gx = ((maxx - minx) >> sh) + 1;
            gy = ((maxy - miny) >> sh) + 1;
            if ((long long)gx * gy <= target) break;
        }
        geo[0] = sh; geo[1] = gx; geo[2] = gy; geo[3] = gx * gy;
        hdr[H_BAD] = 0; hdr[H_N] = n; hdr[H_MINX] = minx; hdr[H_MINY] = miny; hdr[H_MAXX] = maxx; hdr[H_MAXY] = maxy;
        hdr[H_SHIFT] = sh; hdr[H_GX] = gx; hdr[H_GY] = gy;
    }
    for (int c = tid; c < GUIDED_MAX_CELLS; c += GB) cell_n[c] = 0;
    __syncthreads();
    const int sh = geo[0], gy = geo[2], cells = geo[3];
    for (int i = tid; i < n; i += GB) {
        const int x = K[i].x, y = K[i].y;
        atomicAdd(&cell_n[((x - minx) >> sh) * gy + ((y - miny) >> sh)], 1);
    }
    __syncthreads();
    // exclusive scan over the cells: a serial run of `per` cells per thread, then a scan of the 256 run totals
    const int per = (cells + GB - 1) / GB, c0 = tid * per;
    int run = 0;
    for (int c = c0; c < c0 + per && c < cells; c++) run += cell_n[c];
    red[5][tid] = run;
    __syncthreads();
    for (int h = 1; h < GB; h <<= 1) {
        const int v = tid >= h ? red[5][tid - h] : 0;
        __syncthreads();
        red[5][tid] += v;
        __syncthreads();
    }
    int acc = red[5][tid] - run;
    for (int c = c0; c < c0 + per && c < cells; c++) {
        const int v = cell_n[c];
        off[c] = acc;
        cell_n[c] = acc; // from here on: the cell's write cursor
        acc += v;
    }
    if (tid == GB - 1) off[cells] = n;
    __syncthreads();
    // the order inside a cell follows the atomics; no result depends on it (every selection is on a total order of keys)
    for (int i = tid; i < n; i += GB) {
        const int x = K[i].x, y = K[i].y;
        const int pos = atomicAdd(&cell_n[((x - minx) >> sh) * gy + ((y - miny) >> sh)], 1);
        ent[pos] = pack_entry(i, x, y);
    }
}

// ---- 3. the band walk --------------------------------------------------------------------------------------------------

// the integer interval [lo_i, hi_i] of [min(c0, c1) - R, max(c0, c1) + R], padded for rounding and clamped to [bmin, bmax];
// false when empty.  The centres and R come from the hardware's approximate reciprocal and square root (no FMA-based
// refinement, so the kernel has no FMA at all): a relative pad of 2^-12 covers their error, a few cells' worth at most.
__device__ __forceinline__ bool int_span(double c0, double c1, double R, int bmin, int bmax, int &lo_i, int &hi_i)
{
    double lo = fmin(c0, c1) - R, hi = fmax(c0, c1) + R;
    const double pad = 0.000244140625 * (1.0 + fabs(c0) + fabs(c1) + R);
    lo -= pad;
    hi += pad;
    if (!(lo <= hi)) { lo = bmin; hi = bmax; } // NaN: every cell (never expected with finite inputs)
    lo = fmax(lo, (double)bmin);
    hi = fmin(hi, (double)bmax);
    if (lo > hi) return false;
    lo_i = (int)ceil(lo);
    hi_i = (int)floor(hi);
    return lo_i <= hi_i;
}

template <int K, bool COL, int W>
__global__ __launch_bounds__(GB) void k_guided_walk(const uint32_t *__restrict__ desc, const int32_t *__restrict__ counts,
                                                    const int32_t *__restrict__ pairlist, int S, int words, int max_n, int nrb, int M,
                                                    const float *__restrict__ Fm, double band, double T, GuidedWs w,
                                                    int32_t *__restrict__ out_idx, int32_t *__restrict__ out_dist,
                                                    uint32_t *__restrict__ colkey)
{
#pragma clang fp contract(off) // the predicate of include/pgx.h: one rounding per operation, no FMA
    int m, bx;
    pgx_xcd_map(blockIdx.x, nrb, M, m, bx);
    const auto [fa, fb, n1, n2] = pgx_pair_counts(counts, pairlist, m, max_n);
    const int t = bx * GB + threadIdx.x;
    if (t >= n1) return;
    const SlotView A = slot_view(w, w.tab_slot[w.side_pos[2 * m]]);
    const SlotView B = slot_view(w, w.tab_slot[w.side_pos[2 * m + 1]]);
    double f[9];
    bool finite = true;
    for (int q = 0; q < 9; q++) {
        const float v = Fm[9 * (size_t)m + q];
        finite &= isfinite(v);
        f[q] = (double)v;
    }
    int i = t, x = 0, y = 0;
    if (!A.hdr[H_BAD]) {
        const unsigned long long e = A.ent[t];
        i = (int)(e & PGX_IDX_MASK);
        x = (int)((e >> 20) & 0x1FFFFFu) - COORD_LIM;
        y = (int)(e >> 41) - COORD_LIM;
    }
    uint32_t k1 = PGX_KEY_NONE, k2 = PGX_KEY_NONE;
    const double X = (double)x, Y = (double)y;
    // l = F^T (x, y, 1): the products are exact in double
    const double l0 = (f[0] * X + f[3] * Y) + f[6];
    const double l1 = (f[1] * X + f[4] * Y) + f[7];
    const double l2 = (f[2] * X + f[5] * Y) + f[8];
    const double nn = l0 * l0 + l1 * l1;
    if (finite && !A.hdr[H_BAD] && !B.hdr[H_BAD] && n2 > 0 && nn > 0.0) {
        const double thr = T * nn;
        const uint32_t *ra = desc + ((size_t)fa * S + i) * words;
        uint32_t rw[W > 0 ? W : 1];
        if (W > 0)
            for (int q = 0; q < W; q++) rw[q] = ra[q];
        const uint32_t *Bd = desc + (size_t)fb * S * words;
        uint32_t *ck = colkey + (size_t)m * S;
        auto visit = [&](int p0, int p1) __attribute__((always_inline)) {
            for (int p = p0; p < p1; p++) {
                const unsigned long long e = B.ent[p];
                const double u = (double)((int)((e >> 20) & 0x1FFFFFu) - COORD_LIM);
                const double v = (double)((int)(e >> 41) - COORD_LIM);
                const double ev = (l0 * u + l1 * v) + l2;
                if (!(ev * ev <= thr)) continue;
                const int j = (int)(e & PGX_IDX_MASK);
                const uint32_t *rb = Bd + (size_t)j * words;
                int d = 0;
                if (W > 0) {
                    for (int q = 0; q < W; q++) d += __popc(rw[q] ^ rb[q]);
                } else {
                    for (int q = 0; q < words; q++) d += __popc(ra[q] ^ rb[q]);
                }
                const uint32_t key = ((uint32_t)d << PGX_IDX_BITS) | (uint32_t)j;
                if (K == 2) k2 = min(k2, max(k1, key)); // keys are distinct: (k1, k2) stay the two smallest
                k1 = min(k1, key);
                if (COL) {
                    const uint32_t ckey = ((uint32_t)d << PGX_IDX_BITS) | (uint32_t)i;
                    // keys only decrease: a value read earlier bounds the current one from above
                    if (ckey < __hip_atomic_load(ck + j, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMin(ck + j, ckey);
                }
            }
        };
        const int minx = B.hdr[H_MINX], miny = B.hdr[H_MINY], maxx = B.hdr[H_MAXX], maxy = B.hdr[H_MAXY];
        const int sh = B.hdr[H_SHIFT], gx = B.hdr[H_GX], gy = B.hdr[H_GY];
        const int cw = 1 << sh;
        const double rt = __builtin_amdgcn_sqrt(nn);
        if (fabs(l1) >= fabs(l0)) {
            // v as a function of u: centre -(l0 u + l2) / l1, half-width band * |l| / |l1|
            const double r = -__builtin_amdgcn_rcp(l1), R = band * rt * fabs(r);
            for (int cx = 0; cx < gx; cx++) {
                const int u0 = minx + cx * cw, u1 = u0 + cw - 1;
                const double c0 = (l0 * (double)u0 + l2) * r, c1 = (l0 * (double)u1 + l2) * r;
                int vlo, vhi;
                if (!int_span(c0, c1, R, miny, maxy, vlo, vhi)) continue;
                const int base = cx * gy;
                visit(B.off[base + ((vlo - miny) >> sh)], B.off[base + ((vhi - miny) >> sh) + 1]);
            }
        } else {
            const double r = -__builtin_amdgcn_rcp(l0), R = band * rt * fabs(r);
            for (int cy = 0; cy < gy; cy++) {
                const int v0 = miny + cy * cw, v1 = v0 + cw - 1;
                const double c0 = (l1 * (double)v0 + l2) * r, c1 = (l1 * (double)v1 + l2) * r;
                int ulo, uhi;
                if (!int_span(c0, c1, R, minx, maxx, ulo, uhi)) continue;
                const int cx1 = (uhi - minx) >> sh;
                for (int cx = (ulo - minx) >> sh; cx <= cx1; cx++) visit(B.off[cx * gy + cy], B.off[cx * gy + cy + 1]);
            }
        }
    }
    const size_t o = ((size_t)m * S + i) * K;
    pgx_store_keys<K>(k1, k2, out_idx + o, out_dist + o);
}

int table_size(int E)
{
    int H = 16;
    while (H < 2 * E) H <<= 1;
    return H;
}

int cells_cap(int max_n) { return max_n / 2 < 1 ? 1 : (max_n / 2 > GUIDED_MAX_CELLS ? GUIDED_MAX_CELLS : max_n / 2); }

GuidedWs guided_layout(void *ws, int M, int max_n)
{
    GuidedWs w;
    const int E = 2 * M;
    w.H = table_size(E);
    w.cells_cap = cells_cap(max_n);
    w.off_offsets = HDR * sizeof(int);
    w.off_entries = (w.off_offsets + (size_t)(w.cells_cap + 1) * sizeof(int) + 15) & ~(size_t)15;
    w.slot_bytes = (w.off_entries + (size_t)max_n * 8 + 63) & ~(size_t)63;
    int *p = reinterpret_cast<int *>(ws);
    w.cnt = p;
    w.tab_key = p + 16;
    w.tab_slot = w.tab_key + w.H;
    w.side_pos = w.tab_slot + w.H;
    w.slot_frame = w.side_pos + E;
    w.head = ((size_t)(16 + 2 * w.H + 2 * E) * sizeof(int) + 255) & ~(size_t)255;
    w.slots = reinterpret_cast<char *>(ws) + w.head;
    return w;
}

} // namespace

size_t pgx_guided_ws_bytes(int M, int max_n)
{
    const GuidedWs w = guided_layout(nullptr, M, max_n);
    return w.head + (size_t)2 * M * w.slot_bytes;
}

void pgx_launch_guided(pgx_ctx *ctx, hipStream_t s, const uint32_t *d_desc, const pgx_keypoint *d_kp, const int32_t *d_counts,
                       const int32_t *d_pairlist, int M, int S, int words, int max_n, const float *d_F, float band, int k,
                       int32_t *d_idx, int32_t *d_dist, int32_t *d_col, void *ws, int *status)
{
    const GuidedWs w = guided_layout(ws, M, max_n);
    const int E = 2 * M, nb = (max_n + GB - 1) / GB;
    uint32_t *ck = reinterpret_cast<uint32_t *>(d_col);
    {
        ProfScope ps(ctx, "guided_bucket", s);
        (void)hipMemsetAsync(w.cnt, 0, sizeof(int), s);
        (void)hipMemsetAsync(w.tab_key, 0xFF, (size_t)w.H * sizeof(int), s);
        hipLaunchKernelGGL(k_guided_slots, dim3((unsigned)((E + GB - 1) / GB)), dim3(GB), 0, s, d_pairlist, E, w);
        hipLaunchKernelGGL(k_guided_bucket, dim3((unsigned)E), dim3(GB), 0, s, d_kp, d_counts, S, max_n, w, status);
        if (ck) pgx_launch_colkeys(ctx, s, nullptr, false, d_counts, d_pairlist, M, S, max_n, d_col);
    }
    {
        ProfScope ps(ctx, "guided_walk", s);
        const double bd = (double)band, T = bd * bd;
        const unsigned grid = (unsigned)nb * (unsigned)M;
        auto walk = [&](auto K, auto COL, auto W) { // W: the descriptor words a thread keeps in registers (0: any width, from memory)
            hipLaunchKernelGGL((k_guided_walk<decltype(K)::value, decltype(COL)::value, decltype(W)::value>), dim3(grid), dim3(GB), 0, s,
                               d_desc, d_counts, d_pairlist, S, words, max_n, nb, M, d_F, bd, T, w, d_idx, d_dist, ck);
        };
        pgx_dispatch_k_col(k, ck != nullptr, [&](auto K, auto COL) {
            if (words == 8) walk(K, COL, std::integral_constant<int, 8>{});
            else walk(K, COL, std::integral_constant<int, 0>{});
        });
    }
    if (ck) pgx_launch_colkeys(ctx, s, "guided_col", true, d_counts, d_pairlist, M, S, max_n, d_col);
}
