// k_knn.hip -- exact nearest-neighbour matching (include/pgx.h: pgx_knn_batch_dev, pgx_match_nn_batch_dev, pgx_knn).  Per image
// pair: for every row the k <= 2 nearest columns in (distance, column) order, for every column the nearest row in (distance,
// row) order, and the selection (distance gate, ratio test, cross-check) that makes a match list for the track graph of these.
//
// 256-bit descriptors (words == 8) run on the block-scaled FP4 matrix instruction with the arithmetic of k_ham_fp4
// (pgx_fp4.h derives it): acc = F4_BIAS + 8192 * dot + C exactly, dot = 256 - 2 * hamming, and the C input
// carries a 14-bit key so that every selection is an INTEGER maximum of raw accumulator bits.  What differs from k_ham_fp4:
//   * a workgroup owns one row block and walks ALL columns of its image pair, in chunks of at most 4096 (the key's 7-bit tile
//     field): a row's two nearest columns are final inside the workgroup (merged over chunks as distance << 20 | column keys),
//     so there is no merge between workgroups on the row side and no distance matrix anywhere;
//   * row side: per accumulator element a lane keeps b1 >= b2; an element x makes b2 = max(b2, min(b1, x)) -- med3(b1, b2, x)
//     when b1 >= b2 -- and b1 = max(b1, x).  Keys of one lane differ in the tile field, so ties go to the smaller column;
//   * the 32 lanes that share a row are merged by the DPP pattern of half_max_i32 with a top-2 merge at every step (every
//     step combines two disjoint lane sets, so no element is counted twice);
//   * column side: k_ham_fp4's LDS column bests, published once per chunk with a global atomic min of (distance << 20 | row)
//     into the caller's column output, which k_knn_col_finish turns into row indices;
//   * padding: columns past the end of the ragged LAST tile of a chunk are masked on the row side (a duplicate of a real column
//     would come back as a second neighbour); row slots past the end repeat the last row as in k_ham_fp4 (a duplicate ties with
//     its original at a larger row position and never wins a column; its own row results are not written).
// Other widths: plain xor + popcount, one thread per row (top-2) and one per column (nearest row).  Exact; its speed is no target.
#include "pgx_fp4.h"
#include "pgx_pairlist.h"

#include <hip/hip_ext.h>

#include <climits>

namespace {

constexpr int KNN_CHUNK = F4_CHUNK; // columns per pass

// one DPP step of the half-wave merge: (v1 > v2) with the partner lane's pair; lanes of masked-off rows see (INT_MIN, INT_MIN)
template <int CTRL, int ROWMASK>
__device__ __forceinline__ void top2_step(int &v1, int &v2)
{
    const int p1 = __builtin_amdgcn_update_dpp(INT_MIN, v1, CTRL, ROWMASK, 0xF, false);
    const int p2 = __builtin_amdgcn_update_dpp(INT_MIN, v2, CTRL, ROWMASK, 0xF, false);
    v2 = max(min(v1, p1), max(v2, p2));
    v1 = max(v1, p1);
}

// the two largest over each half (32 lanes) of a fully active wavefront: quads, 8, 16 lanes, then row_bcast:15 carries rows 0
// and 2 into rows 1 and 3 (complete in lanes 16..31 and 48..63)
template <int K>
__device__ __forceinline__ void half_top(int &v1, int &v2)
{
    if (K == 1) {
        v1 = max(v1, __builtin_amdgcn_update_dpp(INT_MIN, v1, 0xB1, 0xF, 0xF, false));
        v1 = max(v1, __builtin_amdgcn_update_dpp(INT_MIN, v1, 0x4E, 0xF, 0xF, false));
        v1 = max(v1, __builtin_amdgcn_update_dpp(INT_MIN, v1, 0x141, 0xF, 0xF, false));
        v1 = max(v1, __builtin_amdgcn_update_dpp(INT_MIN, v1, 0x140, 0xF, 0xF, false));
        v1 = max(v1, __builtin_amdgcn_update_dpp(INT_MIN, v1, 0x142, 0xA, 0xF, false));
    } else {
        top2_step<0xB1, 0xF>(v1, v2);  // quad_perm [1,0,3,2]
        top2_step<0x4E, 0xF>(v1, v2);  // quad_perm [2,3,0,1]
        top2_step<0x141, 0xF>(v1, v2); // row_half_mirror
        top2_step<0x140, 0xF>(v1, v2); // row_mirror
        top2_step<0x142, 0xA>(v1, v2); // row_bcast:15 into rows 1, 3
    }
}

// (d, index) keys in min order: merge the pair (n1 <= n2) into (k1 <= k2)
__device__ __forceinline__ void merge_min2(uint32_t &k1, uint32_t &k2, uint32_t n1, uint32_t n2)
{
    k2 = min(max(k1, n1), min(k2, n2));
    k1 = min(k1, n1);
}

// ---- 256-bit descriptors on the FP4 matrix instruction -------------------------------------------------------------------
// idx / dist [M][S][K]; colkey [M][S] (COL): entries j < counts[b] hold PGX_KEY_NONE on entry (k_knn_col_init).
// Held to 240 registers and two waves per SIMD like k_ham_fp4 (tests/test_knn_codegen.py pins it on the code object).
// RT row tiles per wavefront: 4 * RT * 32 rows per workgroup.
template <int K, bool COL, int RT>
__attribute__((amdgpu_num_vgpr(120))) __global__ __launch_bounds__(256, 2) void k_knn_fp4(
    const uint32_t *__restrict__ desc, const int32_t *__restrict__ counts, const int32_t *__restrict__ pairlist, int S, int max_n,
    int nrb, int M, int32_t *__restrict__ out_idx, int32_t *__restrict__ out_dist, uint32_t *__restrict__ colkey)
{
    constexpr int KNN_WROWS = RT * 32, KNN_BM = 4 * KNN_WROWS;
    __shared__ int colbest[COL ? KNN_CHUNK : 1];
    __shared__ uint32_t rowtop[2][KNN_BM]; // running (distance << 20 | column) keys of every row, min order; row owned by one lane
    int m, bx;
    pgx_xcd_map(blockIdx.x, nrb, M, m, bx); // all row blocks of one image pair on one XCD: they stream the same columns
    const auto [fa, fb, n1, n2] = pgx_pair_counts(counts, pairlist, m, max_n);
    const int rb = bx * KNN_BM;
    if (rb >= n1) return;
    const int tid = threadIdx.x;
    int32_t *oidx = out_idx + (size_t)m * S * K, *odist = out_dist + (size_t)m * S * K;
    if (n2 == 0) { // no column: every row's neighbours are missing
        for (int q = tid; q < KNN_BM * K; q += 256)
            if (rb + q / K < n1) { oidx[(size_t)rb * K + q] = -1; odist[(size_t)rb * K + q] = PGX_DIST_NONE; }
        return;
    }
    const int lane = tid & 63, wv = tid >> 6, r = lane & 31, h = lane >> 5;
    int km = (int)0x88888888, kc = 0x22222222;
    asm volatile("" : "+v"(km), "+v"(kc)); // pin the two expansion constants in vector registers

    // row operand: this lane's row of each 32-row tile, its 16-byte quarter-pair (words 4h .. 4h+3) expanded
    const uint32_t *dA = desc + (size_t)fa * S * 8;
    int afr[RT][4][4];
#pragma unroll
    for (int t = 0; t < RT; t++) {
        const int row = rb + wv * KNN_WROWS + t * 32 + r;
        const uint4 w = *reinterpret_cast<const uint4 *>(dA + (size_t)(row < n1 ? row : n1 - 1) * 8 + 4 * h);
        expand_fp4(w.x, km, kc, afr[t][0]);
        expand_fp4(w.y, km, kc, afr[t][1]);
        expand_fp4(w.z, km, kc, afr[t][2]);
        expand_fp4(w.w, km, kc, afr[t][3]);
    }
    const int kwv = (127 - wv) << 7; // column side: the tile field is swapped for the wave's place in the workgroup

    for (int cb = 0; cb < n2; cb += KNN_CHUNK) {
        const int ncol = n2 - cb < KNN_CHUNK ? n2 - cb : KNN_CHUNK, ntile = (ncol + 31) / 32;
        if (COL) {
            for (int c = tid; c < ntile * 32; c += 256) colbest[c] = 0; // below every real value
            __syncthreads();
        }
        const char *dB = reinterpret_cast<const char *>(desc + ((size_t)fb * S + cb) * 8);
        auto fetch = [&](int ct) -> uint4 { // this lane's quarter-pair of column ct * 32 + r, clamped into the chunk
            int c = (ct > 0 ? ct : 0) * 32 + r;
            c = c < ncol ? c : ncol - 1;
            return *reinterpret_cast<const uint4 *>(dB + (uint32_t)c * 32u + 16u * (uint32_t)h);
        };
        // C input of the LAST tile (the loop walks the tiles downwards; a tile step adds 128 on the matrix pipe, see k_ham_fp4):
        // (127 - ct) << 7 | (127 - row position inside the wave's tile)
        f32x16 cc;
        int b1[RT][16], b2[RT][16];
#pragma unroll
        for (int g = 0; g < 16; g++) {
            cc[g] = (float)(F4_BIAS + (((127 - (ntile - 1)) << 7) | (127 - ((g & 3) + 8 * (g >> 2) + 4 * h))));
#pragma unroll
            for (int t = 0; t < RT; t++) b1[t][g] = b2[t][g] = 0; // below every real value (raw bits of a float >= 2^23)
        }
        // one column tile; `slot` holds its raw words (loaded four tiles ago) and is refilled for tile ct - 4
        auto step = [&](int ct, uint4 &slot, bool ragged) {
            int b[4][4];
            expand_fp4(slot.x, km, kc, b[0]);
            expand_fp4(slot.y, km, kc, b[1]);
            expand_fp4(slot.z, km, kc, b[2]);
            expand_fp4(slot.w, km, kc, b[3]);
            slot = fetch(ct - 4);
            const i32x8 onesv = {kc, kc, kc, kc, 0, 0, 0, 0}; // the fp4 code of +1 in every nibble
            const f32x16 ccn = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(onesv, onesv, cc, 4, 4, 0, 128, 0, 127);
            const bool valid = !ragged || ct * 32 + r < ncol;
            int xm[RT];
#pragma unroll
            for (int t = 0; t < RT; t++) {
                f32x16 acc = cc;
#pragma unroll
                for (int s4 = 0; s4 < 4; s4++) {
                    const i32x8 av = {afr[t][s4][0], afr[t][s4][1], afr[t][s4][2], afr[t][s4][3], 0, 0, 0, 0};
                    const i32x8 bv = {b[s4][0], b[s4][1], b[s4][2], b[s4][3], 0, 0, 0, 0};
                    acc = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(av, bv, acc, 4, 4, 0, F4_SCALE_A, 0, 127);
                }
                i32x16 ai;
#pragma unroll
                for (int g = 0; g < 16; g++) ai[g] = __float_as_int(acc[g]);
#pragma unroll
                for (int g = 0; g < 16; g++) {
                    const int x = valid ? ai[g] : 0;
                    if (K == 2) b2[t][g] = max(min(b1[t][g], x), min(max(b1[t][g], x), b2[t][g])); // v_med3_i32
                    b1[t][g] = max(b1[t][g], x);
                }
                if (COL) xm[t] = max16i(ai) - 32 * t; // best of the lane's 16 rows, moved to the tile's place in the wave
            }
            if (COL) {
                int cm = xm[0];
#pragma unroll
                for (int t = 1; t < RT; t++) cm = max(cm, xm[t]);
                atomicMax(&colbest[ct * 32 + r], cm + (kwv - ((127 - ct) << 7)));
            }
            cc = ccn;
        };
        uint4 w0 = fetch(ntile - 1), w1 = fetch(ntile - 2), w2 = fetch(ntile - 3), w3 = fetch(ntile - 4);
        int ct = ntile - 1;
        step(ct, w0, true); // the only tile that can be ragged
        ct--;
        for (; ct >= 3; ct -= 4) {
            step(ct, w1, false);
            step(ct - 1, w2, false);
            step(ct - 2, w3, false);
            step(ct - 3, w0, false);
        }
        if (ct >= 0) { step(ct, w1, false); ct--; }
        if (ct >= 0) { step(ct, w2, false); ct--; }
        if (ct >= 0) { step(ct, w3, false); ct--; }

        // row side: rebuild each value's column position (key = 8191 - position: the smaller column wins a tie), merge the
        // 32 lanes of a row set; value g of a tile ends in lane 16 + g (h = 0) / 48 + g (h = 1)
        int tid2 = threadIdx.x;
        asm volatile("" : "+v"(tid2));
        const int r2 = tid2 & 31;
        uint32_t n1k[RT], n2k[RT];
#pragma unroll
        for (int t = 0; t < RT; t++) {
            int mine1 = INT_MIN, mine2 = INT_MIN;
#pragma unroll
            for (int g = 0; g < 16; g++) {
                auto rekey = [&](int x) {
                    const int raw = x - F4_RAW0;
                    const int cpos = (127 - ((raw >> 7) & 127)) * 32 + r2;
                    return x == 0 ? INT_MIN : (raw & ~0x3FFF) | (8191 - cpos);
                };
                int v1 = rekey(b1[t][g]), v2 = K == 2 ? rekey(b2[t][g]) : INT_MIN;
                half_top<K>(v1, v2);
                if (r2 == 16 + g) { mine1 = v1; mine2 = v2; }
            }
            auto gkey = [&](int v) -> uint32_t { // (hamming << 20 | column) of a merged value
                return v == INT_MIN ? PGX_KEY_NONE
                                    : ((uint32_t)(128 - (v >> 14)) << PGX_IDX_BITS) | (uint32_t)(cb + 8191 - (v & 0x3FFF));
            };
            n1k[t] = gkey(mine1);
            n2k[t] = gkey(mine2);
        }
        if (r2 >= 16) { // the lane owns row value g = r2 - 16 of each of its tiles (in LDS: no registers held across the chunks)
            const int g = r2 - 16, h2 = (tid2 >> 5) & 1, wv2 = tid2 >> 6;
#pragma unroll
            for (int t = 0; t < RT; t++) {
                const int iloc = wv2 * KNN_WROWS + t * 32 + (g & 3) + 8 * (g >> 2) + 4 * h2;
                uint32_t k1 = cb ? rowtop[0][iloc] : PGX_KEY_NONE, k2 = cb ? rowtop[1][iloc] : PGX_KEY_NONE;
                merge_min2(k1, k2, n1k[t], n2k[t]);
                rowtop[0][iloc] = k1;
                rowtop[1][iloc] = k2;
            }
        }
        if (COL) {
            __syncthreads(); // colbest complete
            uint32_t *ck = colkey + (size_t)m * S + cb;
            for (int c = tid; c < ncol; c += 256) {
                const int cbv = colbest[c];
                if (cbv == 0) continue;
                const int v = cbv - F4_RAW0;
                const int key = 16383 - (v & 0x3FFF); // wave << 7 | row position inside the wave
                const int iloc = (key >> 7) * KNN_WROWS + (key & 127);
                atomicMin(&ck[c], ((uint32_t)(128 - (v >> 14)) << PGX_IDX_BITS) | (uint32_t)(rb + iloc));
            }
            __syncthreads(); // before the next chunk clears colbest
        }
    }

    int tid3 = threadIdx.x;
    asm volatile("" : "+v"(tid3));
    const int r3 = tid3 & 31, h3 = (tid3 >> 5) & 1, wv3 = tid3 >> 6;
    if (r3 >= 16) {
        const int g = r3 - 16;
#pragma unroll
        for (int t = 0; t < RT; t++) {
            const int iloc = wv3 * KNN_WROWS + t * 32 + (g & 3) + 8 * (g >> 2) + 4 * h3, i = rb + iloc;
            if (i < n1) pgx_store_keys<K>(rowtop[0][iloc], rowtop[1][iloc], oidx + (size_t)i * K, odist + (size_t)i * K);
        }
    }
}

// column output as keys, (distance << 20 | row) while a producer runs (k_knn_fp4, k_guided_walk): NONE for j < counts[b] of every pair
__global__ __launch_bounds__(256) void k_knn_col_init(const int32_t *__restrict__ counts, const int32_t *__restrict__ pairlist,
                                                      int S, int max_n, int ncb, int M, uint32_t *__restrict__ colkey)
{
    int m, bx;
    pgx_xcd_map(blockIdx.x, ncb, M, m, bx);
    const int j = bx * 256 + threadIdx.x;
    if (j < pgx_clamp_count(counts[pairlist[2 * m + 1]], max_n)) colkey[(size_t)m * S + j] = PGX_KEY_NONE;
}

// keys -> row indices (-1: no row)
__global__ __launch_bounds__(256) void k_knn_col_finish(const int32_t *__restrict__ counts, const int32_t *__restrict__ pairlist,
                                                        int S, int max_n, int ncb, int M, uint32_t *__restrict__ colkey)
{
    int m, bx;
    pgx_xcd_map(blockIdx.x, ncb, M, m, bx);
    const int j = bx * 256 + threadIdx.x;
    if (j < pgx_clamp_count(counts[pairlist[2 * m + 1]], max_n)) {
        const uint32_t k = colkey[(size_t)m * S + j];
        colkey[(size_t)m * S + j] = k == PGX_KEY_NONE ? 0xFFFFFFFFu : (k & PGX_IDX_MASK);
    }
}

// ---- any width: xor + popcount ------------------------------------------------------------------------------------------
template <int K>
__global__ __launch_bounds__(256) void k_knn_rows_valu(const uint32_t *__restrict__ desc, const int32_t *__restrict__ counts,
                                                       const int32_t *__restrict__ pairlist, int S, int words, int max_n, int nrb,
                                                       int M, int32_t *__restrict__ out_idx, int32_t *__restrict__ out_dist)
{
    int m, bx;
    pgx_xcd_map(blockIdx.x, nrb, M, m, bx);
    const auto [fa, fb, n1, n2] = pgx_pair_counts(counts, pairlist, m, max_n);
    const int i = bx * 256 + threadIdx.x;
    if (i >= n1) return;
    const uint32_t *a = desc + ((size_t)fa * S + i) * words, *B = desc + (size_t)fb * S * words;
    int d1 = PGX_DIST_NONE, d2 = PGX_DIST_NONE, j1 = -1, j2 = -1;
    for (int j = 0; j < n2; j++) { // ascending j and strict comparisons: a tie keeps the smaller column
        const uint32_t *b = B + (size_t)j * words;
        int d = 0;
        for (int w = 0; w < words; w++) d += __popc(a[w] ^ b[w]);
        if (d < d1) { d2 = d1; j2 = j1; d1 = d; j1 = j; }
        else if (K == 2 && d < d2) { d2 = d; j2 = j; }
    }
    const size_t o = ((size_t)m * S + i) * K;
    out_idx[o] = j1; out_dist[o] = d1;
    if (K == 2) { out_idx[o + 1] = j2; out_dist[o + 1] = d2; }
}

__global__ __launch_bounds__(256) void k_knn_cols_valu(const uint32_t *__restrict__ desc, const int32_t *__restrict__ counts,
                                                       const int32_t *__restrict__ pairlist, int S, int words, int max_n, int ncb,
                                                       int M, int32_t *__restrict__ col_nn)
{
    int m, bx;
    pgx_xcd_map(blockIdx.x, ncb, M, m, bx);
    const auto [fa, fb, n1, n2] = pgx_pair_counts(counts, pairlist, m, max_n);
    const int j = bx * 256 + threadIdx.x;
    if (j >= n2) return;
    const uint32_t *b = desc + ((size_t)fb * S + j) * words, *A = desc + (size_t)fa * S * words;
    int d1 = PGX_DIST_NONE, i1 = -1;
    for (int i = 0; i < n1; i++) {
        const uint32_t *a = A + (size_t)i * words;
        int d = 0;
        for (int w = 0; w < words; w++) d += __popc(a[w] ^ b[w]);
        if (d < d1) { d1 = d; i1 = i; }
    }
    col_nn[(size_t)m * S + j] = i1;
}

// ---- the NN list: distance gate, ratio test, cross-check ---------------------------------------------------------------
__global__ __launch_bounds__(256) void k_knn_select(const int32_t *__restrict__ counts, const int32_t *__restrict__ pairlist, int S,
                                                    int max_n, int nrb, int M, const int32_t *__restrict__ idx,
                                                    const int32_t *__restrict__ dist, const int32_t *__restrict__ col_nn,
                                                    int max_dist, float ratio, int cross_check, pgx_pair *__restrict__ out)
{
    int m, bx;
    pgx_xcd_map(blockIdx.x, nrb, M, m, bx);
    const int n1 = pgx_clamp_count(counts[pairlist[2 * m]], max_n);
    const int i = bx * 256 + threadIdx.x;
    if (i >= n1) return;
    const size_t o = (size_t)m * S + i;
    const int j1 = idx[2 * o], d1 = dist[2 * o], j2 = idx[2 * o + 1], d2 = dist[2 * o + 1];
    bool ok = j1 >= 0 && d1 <= max_dist;
    // exact: d <= 4064 and a float ratio are exact in double, and so is their product
    if (ok && ratio > 0.f && j2 >= 0) ok = (double)d1 < (double)ratio * (double)d2;
    if (ok && cross_check) ok = col_nn[(size_t)m * S + j1] == i;
    pgx_pair p;
    p.k1 = i;
    p.k2 = ok ? j1 : -1;
    p.dist = ok ? d1 : PGX_DIST_NONE;
    out[o] = p;
}

template <int K, bool COL>
void launch_fp4(pgx_ctx *ctx, hipStream_t s, const uint32_t *d_desc, const int32_t *d_counts, const int32_t *d_pairlist, int M,
                int S, int max_n, int32_t *d_idx, int32_t *d_dist, int32_t *d_col)
{
    // two row tiles per wavefront (the fp4 expansion of a column tile feeds both); the k = 2 form WITHOUT the column side spills
    // there (hipcc 7.2 schedules it into 240 + 36 registers, the form with the column side fits in 238), so it keeps one
    constexpr int RT = (K == 2 && !COL) ? 1 : 2;
    const int nrb = (max_n + 128 * RT - 1) / (128 * RT);
    const dim3 grid((unsigned)nrb * (unsigned)M);
    uint32_t *ck = reinterpret_cast<uint32_t *>(d_col);
    auto *kern = &k_knn_fp4<K, COL, RT>;
    ProfScope ps(ctx, "knn", s, true); // the dispatch's own time stamps
    if (ps.a && ps.b)
        hipExtLaunchKernelGGL(kern, grid, dim3(256), 0, s, ps.a, ps.b, 0, d_desc, d_counts, d_pairlist, S, max_n, nrb, M,
                              d_idx, d_dist, ck);
    else
        hipLaunchKernelGGL(kern, grid, dim3(256), 0, s, d_desc, d_counts, d_pairlist, S, max_n, nrb, M, d_idx, d_dist, ck);
}

} // namespace

void pgx_launch_colkeys(pgx_ctx *ctx, hipStream_t s, const char *scope, bool finish, const int32_t *d_counts,
                        const int32_t *d_pairlist, int M, int S, int max_n, int32_t *d_col)
{
    const int nb = (max_n + 255) / 256;
    ProfScope ps(ctx, scope, s);
    hipLaunchKernelGGL(finish ? k_knn_col_finish : k_knn_col_init, dim3((unsigned)nb * M), dim3(256), 0, s, d_counts, d_pairlist, S, max_n,
                       nb, M, reinterpret_cast<uint32_t *>(d_col));
}

void pgx_launch_knn(pgx_ctx *ctx, hipStream_t s, const uint32_t *d_desc, const int32_t *d_counts, const int32_t *d_pairlist, int M,
                    int S, int words, int max_n, int k, int32_t *d_idx, int32_t *d_dist, int32_t *d_col)
{
    const int nb = (max_n + 255) / 256; // 256-row blocks (KNN_BM) and 256-column blocks per image pair
    if (words == 8) {
        if (d_col) pgx_launch_colkeys(ctx, s, "knn_col", false, d_counts, d_pairlist, M, S, max_n, d_col);
        pgx_dispatch_k_col(k, d_col != nullptr, [&](auto K, auto COL) {
            launch_fp4<decltype(K)::value, decltype(COL)::value>(ctx, s, d_desc, d_counts, d_pairlist, M, S, max_n, d_idx, d_dist, d_col);
        });
        if (d_col) pgx_launch_colkeys(ctx, s, "knn_col", true, d_counts, d_pairlist, M, S, max_n, d_col);
        return;
    }
    ProfScope ps(ctx, "knn", s);
    if (k == 1)
        hipLaunchKernelGGL(k_knn_rows_valu<1>, dim3((unsigned)nb * M), dim3(256), 0, s, d_desc, d_counts, d_pairlist, S, words, max_n,
                           nb, M, d_idx, d_dist);
    else
        hipLaunchKernelGGL(k_knn_rows_valu<2>, dim3((unsigned)nb * M), dim3(256), 0, s, d_desc, d_counts, d_pairlist, S, words, max_n,
                           nb, M, d_idx, d_dist);
    if (d_col)
        hipLaunchKernelGGL(k_knn_cols_valu, dim3((unsigned)nb * M), dim3(256), 0, s, d_desc, d_counts, d_pairlist, S, words, max_n, nb,
                           M, d_col);
}

void pgx_launch_knn_select(pgx_ctx *ctx, hipStream_t s, const int32_t *d_counts, const int32_t *d_pairlist, int M, int S, int max_n,
                           const int32_t *d_idx, const int32_t *d_dist, const int32_t *d_col, int max_dist, float ratio,
                           int cross_check, pgx_pair *d_out)
{
    const int nb = (max_n + 255) / 256;
    ProfScope ps(ctx, "knn_select", s);
    hipLaunchKernelGGL(k_knn_select, dim3((unsigned)nb * M), dim3(256), 0, s, d_counts, d_pairlist, S, max_n, nb, M, d_idx, d_dist,
                       d_col, max_dist, ratio, cross_check, d_out);
}
