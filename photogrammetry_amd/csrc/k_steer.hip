// k_steer.hip -- steered BRIEF for gfx950: one wavefront per keypoint, orientation pass and then the descriptor with the pair
// table of the keypoint's direction.  Not in the C# reference; the rule is include/pgx.h's ("steered BRIEF"), every step of
// it in integers, and tests/steered_ref.py restates it in numpy.
//
// Orientation (orient_bin): the disc has radius R <= 31, so its 2R + 1 <= 63 columns fit one wave: lane l owns the column
// dx = l - R and the wave walks the rows dy = -R .. R, each step ONE coalesced load of a row segment of the grey image.  The
// rows go through in groups of ROWS_AHEAD whose loads are all issued before the first value is used.  A lane outside the
// row's half-width (dx^2 + dy^2 > R^2), outside the disc's columns or outside the image takes 0 and loads nothing.  Per lane
// two int32 sums, sum q and sum dy * q; its share of m10 is dx * sum q, formed once at the end.  Two wave sums give
// (m10, m01); lanes k < B form s_k in int64 and ONE wave maximum of ((s_k + 2^46) << 6) | (63 - k) picks the largest s_k and,
// among equals, the smallest k.  Nothing rounds after q: every partial sum is below 2^31 (pgx.h), so any order of the wave
// sums gives the same integers.
//
// Descriptor: brief_256 on plans + bin * PGX_PLAN_WORDS (P == 256), brief_one on pairs_rot + bin * P (every other P); both are
// k_brief.hip's own, unchanged (k_brief_core.inc).  The bin is wave-uniform, so the table's address is scalar.
#include "pgx_internal.h"
#include "pgx_brief_plan.h"

namespace {

#include "k_brief_core.inc"

constexpr int ROWS_AHEAD = 8;

// q(g) of pgx.h: NaN -> 0, clamp to [0, 1], one float32 multiplication by 65535, round to nearest even
__device__ __forceinline__ int steer_q(float v)
{
    v = v >= 0.f ? v : 0.f; // NaN and negatives (the comparison is false for NaN)
    v = v > 1.f ? 1.f : v;  // +inf too
    return (int)__builtin_rintf(v * 65535.0f);
}

__device__ __forceinline__ int wave_sum(int v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// the direction bin of the keypoint (x, y); wave-uniform (an SGPR)
__device__ __forceinline__ int orient_bin(const float *__restrict__ img, int W, int H, int x, int y, const int2 *__restrict__ dirs,
                                          int B, int R)
{
    const int lane = threadIdx.x & 63;
    const int dx = lane - R, R2 = R * R;
    // unsigned arithmetic: a list keypoint may lie anywhere in int32, and a wrapped coordinate is never below W or H
    const uint32_t xs = (uint32_t)x + (uint32_t)dx;
    const int rem = R2 - dx * dx; // the row dy is inside the disc at this column when dy^2 <= rem
    const bool col_in = rem >= 0 && xs < (uint32_t)W;
    int sq = 0, sdy = 0;
    for (int r0 = -R; r0 <= R; r0 += ROWS_AHEAD) {
        float v[ROWS_AHEAD];
#pragma unroll
        for (int j = 0; j < ROWS_AHEAD; j++) {
            const int dy = r0 + j;
            const uint32_t ys = (uint32_t)y + (uint32_t)dy;
            const bool in = col_in && dy * dy <= rem && ys < (uint32_t)H; // rem <= R^2: also false for the rows past R of the last group
            v[j] = in ? img[ys * (uint32_t)W + xs] : 0.f; // exact inside the image: W, H <= 65535 (dims_ok)
        }
#pragma unroll
        for (int j = 0; j < ROWS_AHEAD; j++) {
            const int q = steer_q(v[j]);
            sq += q;
            sdy += (r0 + j) * q;
        }
    }
    const int m10 = wave_sum(dx * sq), m01 = wave_sum(sdy);
    unsigned long long key = 0;
    if (lane < B) {
        const int2 d = dirs[lane];
        const long long s = (long long)m10 * d.x + (long long)m01 * d.y; // |s| < 2^46
        key = ((unsigned long long)(s + (1ll << 46)) << 6) | (unsigned long long)(63 - lane);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const unsigned long long other = __shfl_xor(key, o, 64);
        key = other > key ? other : key;
    }
    return __builtin_amdgcn_readfirstlane(63 - (int)(key & 63u));
}

// k_brief_kept with the orientation pass in front (same block -> frame map, same LDS, no workgroup barrier);
// bins_out [F][out_stride] is optional
template <bool P256>
__global__ __launch_bounds__(256) void k_steer_kept(const float *__restrict__ gray, int W, int H,
                                                    const uint32_t *__restrict__ raw_xy,
                                                    const int32_t *__restrict__ raw_score, int raw_cap,
                                                    const uint32_t *__restrict__ order,
                                                    const int32_t *__restrict__ n_kept, int kp_cap,
                                                    const int4 *__restrict__ pairs_rot, const int32_t *__restrict__ plans,
                                                    const int2 *__restrict__ dirs, int B, int R, int P,
                                                    int words, pgx_keypoint *__restrict__ kp_out, uint32_t *__restrict__ desc_out,
                                                    int32_t *__restrict__ bins_out,
                                                    int32_t *__restrict__ counts_out, int nframes, int out_stride)
{
    __shared__ uint32_t wbuf[4][STRIP_WORDS]; // brief_256: value strip + masks; brief_one: MAX_WORDS + 2 words of it
    int f, kb;
    pgx_xcd_map(blockIdx.x, (kp_cap + 3) / 4, nframes, f, kb); // one frame's reads through ONE XCD's L2, as in k_brief_kept
    const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int k = kb * 4 + wv;
    const int nk = n_kept[f];
    if (kb == 0 && threadIdx.x == 0) counts_out[f] = nk;
    if (k >= nk) return; // wave-uniform
    // the keypoint is the wave's: kept in SGPRs, so that the orientation pass fits into brief_256's vector registers
    const uint32_t ri = __builtin_amdgcn_readfirstlane(order[(size_t)f * kp_cap + k]);
    const uint32_t xy = __builtin_amdgcn_readfirstlane(raw_xy[(size_t)f * raw_cap + ri]);
    const int x = (int)(xy & 0xFFFFu), y = (int)(xy >> 16);
    const float *g = gray + (size_t)f * W * H;
    const int bin = orient_bin(g, W, H, x, y, dirs, B, R);
    if (lane == 0) {
        pgx_keypoint kp;
        kp.x = x; kp.y = y; kp.fast_score = raw_score[(size_t)f * raw_cap + ri];
        kp.value = g[(size_t)y * W + x]; // Keypoint.cs:26
        kp_out[(size_t)f * out_stride + k] = kp;
        if (bins_out) bins_out[(size_t)f * out_stride + k] = bin;
    }
    if (P256) brief_256(g, W, H, x, y, plans + (size_t)bin * PGX_PLAN_WORDS, wbuf[wv], desc_out + ((size_t)f * out_stride + k) * 8);
    else brief_one(g, W, H, x, y, pairs_rot + (size_t)bin * P, P, words, wbuf[wv], desc_out + ((size_t)f * out_stride + k) * words);
}

template <bool P256>
__global__ __launch_bounds__(256) void k_steer_list(const float *__restrict__ gray, int W, int H,
                                                    const pgx_keypoint *__restrict__ kps, int n,
                                                    const int4 *__restrict__ pairs_rot, const int32_t *__restrict__ plans,
                                                    const int2 *__restrict__ dirs, int B, int R, int P,
                                                    int words, uint32_t *__restrict__ desc_out)
{
    __shared__ uint32_t wbuf[4][STRIP_WORDS];
    const int wv = threadIdx.x >> 6;
    const int k = blockIdx.x * 4 + wv;
    if (k >= n) return;
    const int x = __builtin_amdgcn_readfirstlane(kps[k].x), y = __builtin_amdgcn_readfirstlane(kps[k].y); // the wave's keypoint, in SGPRs
    const int bin = orient_bin(gray, W, H, x, y, dirs, B, R);
    if (P256) brief_256(gray, W, H, x, y, plans + (size_t)bin * PGX_PLAN_WORDS, wbuf[wv], desc_out + (size_t)k * 8);
    else brief_one(gray, W, H, x, y, pairs_rot + (size_t)bin * P, P, words, wbuf[wv], desc_out + (size_t)k * words);
}

// bins only (pgx_orient)
__global__ __launch_bounds__(256) void k_orient_list(const float *__restrict__ gray, int W, int H,
                                                     const pgx_keypoint *__restrict__ kps, int n,
                                                     const int2 *__restrict__ dirs, int B, int R, int32_t *__restrict__ bins_out)
{
    const int k = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (k >= n) return;
    const int bin = orient_bin(gray, W, H, kps[k].x, kps[k].y, dirs, B, R);
    if ((threadIdx.x & 63) == 0) bins_out[k] = bin;
}

} // namespace

void pgx_launch_steer(hipStream_t s, const float *gray, int F, int W, int H, const uint32_t *raw_xy,
                      const int32_t *raw_score, int raw_cap, const uint32_t *order, const int32_t *n_kept,
                      int kp_cap, const PgxSteer &st, int P, pgx_keypoint *kp_out, uint32_t *desc_out,
                      int32_t *counts_out, int out_stride)
{
    if (F <= 0 || kp_cap <= 0) return;
    const int words = (P + 31) / 32;
    hipLaunchKernelGGL(P == PGX_PLAN_PAIRS ? k_steer_kept<true> : k_steer_kept<false>, dim3(((kp_cap + 3) / 4) * F), dim3(256), 0, s, gray, W, H,
                       raw_xy, raw_score, raw_cap, order, n_kept, kp_cap, reinterpret_cast<const int4 *>(st.pairs_rot), st.plans,
                       reinterpret_cast<const int2 *>(st.dirs), st.B, st.R, P, words, kp_out, desc_out, st.bins_out, counts_out, F,
                       out_stride);
}

void pgx_launch_steer_list(hipStream_t s, const float *gray, int W, int H, const pgx_keypoint *kps, int n, const PgxSteer &st,
                           int P, uint32_t *desc_out)
{
    if (n <= 0) return;
    const int words = (P + 31) / 32;
    hipLaunchKernelGGL(P == PGX_PLAN_PAIRS ? k_steer_list<true> : k_steer_list<false>, dim3((n + 3) / 4), dim3(256), 0, s, gray, W, H, kps, n,
                       reinterpret_cast<const int4 *>(st.pairs_rot), st.plans, reinterpret_cast<const int2 *>(st.dirs), st.B, st.R, P,
                       words, desc_out);
}

void pgx_launch_orient_list(hipStream_t s, const float *gray, int W, int H, const pgx_keypoint *kps, int n, const PgxSteer &st,
                            int32_t *bins_out)
{
    if (n <= 0) return;
    hipLaunchKernelGGL(k_orient_list, dim3((n + 3) / 4), dim3(256), 0, s, gray, W, H, kps, n,
                       reinterpret_cast<const int2 *>(st.dirs), st.B, st.R, bins_out);
}
