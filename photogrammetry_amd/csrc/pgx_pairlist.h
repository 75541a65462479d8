// pgx_pairlist.h -- what the producers of per-pair neighbour lists share (k_knn.hip, k_guided.hip, and through pgx_fp4_nn.h
// the quantiser of k_vocab.hip): the clamped counts of an image pair (the clamp itself, pgx_clamp_count, is pgx_block.h's), the
// write-out of (distance << 20 | index) keys, and the k in {1, 2} x column side on / off dispatch of their launchers.  The
// column-key kernels themselves live in k_knn.hip (pgx_launch_colkeys, pgx_internal.h).
// Internal to libpgx.so; DESIGN.md section 14b.
#pragma once

#include "pgx_internal.h"
#include "pgx_block.h"   // pgx_clamp_count

// calls fn(integral_constant<int, k>, bool_constant<col>) for k in {1, 2}: a launcher names its argument list once
template <class Fn> void pgx_dispatch_k_col(int k, bool col, Fn &&fn)
{
    using K1 = std::integral_constant<int, 1>;
    using K2 = std::integral_constant<int, 2>;
    if (k == 1 && !col) fn(K1{}, std::false_type{});
    else if (k == 1) fn(K1{}, std::true_type{});
    else if (!col) fn(K2{}, std::false_type{});
    else fn(K2{}, std::true_type{});
}

#ifdef __HIPCC__

// image pair m: its two frames and their counts clamped to [0, max_n]
struct PairCounts {
    int fa, fb, n1, n2;
};
__device__ __forceinline__ PairCounts pgx_pair_counts(const int32_t *__restrict__ counts, const int32_t *__restrict__ pairlist, int m,
                                                      int max_n)
{
    const int fa = pairlist[2 * m], fb = pairlist[2 * m + 1];
    return {fa, fb, pgx_clamp_count(counts[fa], max_n), pgx_clamp_count(counts[fb], max_n)};
}

// a row's K smallest keys (k1 <= k2) as its K entries of idx / dist; no neighbour: (-1, PGX_DIST_NONE).  dist may be null
template <int K> __device__ __forceinline__ void pgx_store_keys(uint32_t k1, uint32_t k2, int32_t *idx, int32_t *dist)
{
    const uint32_t k[2] = {k1, k2};
#pragma unroll
    for (int j = 0; j < K; j++) {
        idx[j] = k[j] == PGX_KEY_NONE ? -1 : (int32_t)(k[j] & PGX_IDX_MASK);
        if (dist) dist[j] = k[j] == PGX_KEY_NONE ? PGX_DIST_NONE : (int32_t)(k[j] >> PGX_IDX_BITS);
    }
}

#endif // __HIPCC__
