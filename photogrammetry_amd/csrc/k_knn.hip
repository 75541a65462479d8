// k_knn.hip -- exact nearest-neighbour matching (include/pgx.h: pgx_knn_batch_dev, pgx_match_nn_batch_dev, pgx_knn).  Per image
// pair: for every row the k <= 2 nearest columns in (distance, column) order, for every column the nearest row in (distance,
// row) order, and the selection (distance gate, ratio test, cross-check) that makes a match list for the track graph of these.
//
// 256-bit descriptors (words == 8) run on the block-scaled FP4 matrix instruction: k_knn_fp4 maps a workgroup to a row block of
// an image pair and hands it to fp4_nn_block (pgx_fp4_nn.h describes the tile walk, the keys, the merges and the padding), which
// the vocabulary quantiser (k_vocab.hip) runs too.  The column side posts (distance << 20 | row) keys with global atomic minima
// into the caller's column output, which k_knn_col_init prepares and k_knn_col_finish turns into row indices.
// Other widths: plain xor + popcount, one thread per row (top-2) and one per column (nearest row).  Exact; its speed is no target.
#include "pgx_fp4_nn.h"

#include <hip/hip_ext.h>

namespace {

// ---- 256-bit descriptors on the FP4 matrix instruction -------------------------------------------------------------------
// idx / dist [M][S][K]; colkey [M][S] (COL): entries j < counts[b] hold PGX_KEY_NONE on entry (k_knn_col_init).
// Held to 240 registers and two waves per SIMD like k_ham_fp4 (tests/test_knn_codegen.py pins it on the code object).
// RT row tiles per wavefront: 4 * RT * 32 rows per workgroup.
template <int K, bool COL, int RT>
__attribute__((amdgpu_num_vgpr(120))) __global__ __launch_bounds__(256, 2) void k_knn_fp4(
    const uint32_t *__restrict__ desc, const int32_t *__restrict__ counts, const int32_t *__restrict__ pairlist, int S, int max_n,
    int nrb, int M, int32_t *__restrict__ out_idx, int32_t *__restrict__ out_dist, uint32_t *__restrict__ colkey)
{
    constexpr int KNN_BM = 4 * RT * 32;
    int m, bx;
    pgx_xcd_map(blockIdx.x, nrb, M, m, bx); // all row blocks of one image pair on one XCD: they stream the same columns
    const auto [fa, fb, n1, n2] = pgx_pair_counts(counts, pairlist, m, max_n);
    const int rb = bx * KNN_BM;
    if (rb >= n1) return;
    int32_t *oidx = out_idx + (size_t)m * S * K, *odist = out_dist + (size_t)m * S * K;
    if (n2 == 0) { // no column: every row's neighbours are missing
        for (int q = threadIdx.x; q < KNN_BM * K; q += 256)
            if (rb + q / K < n1) { oidx[(size_t)rb * K + q] = -1; odist[(size_t)rb * K + q] = PGX_DIST_NONE; }
        return;
    }
    fp4_nn_block<K, COL, RT>(desc + (size_t)fa * S * 8, n1, desc, (size_t)fb * S, n2, rb, oidx, odist, colkey + (size_t)m * S);
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
