// k_brief.hip -- Keypoint.GetBriefDescriptor for gfx950: one wavefront per keypoint.
//
// Reference: ImageProcessing.Abstractions/Keypoint.cs:29-57.  For test pair p (table order):
// descriptor <<= 1; if either test point is outside [0,W)x[0,H) the bit stays 0; else bit =
// (K[c1] < K[c2]).  So pair p lands on BigInteger bit P-1-p.
//
// Lane l of chunk c evaluates pair 64c+l; a 64-bit ballot, bit-reversed, is the descriptor's
// bits [P-64(c+1), P-64c).  Gathers hit L2 (a 1080p grey image is 8.3 MB); per survivor
// 2*P*4 B of gathers and P/8 B written -- negligible next to the detect stream.
// P == 256 (brief_256) loads the end points in row order from a plan made once per table and hands
// them to the pair lanes through 2 KiB of LDS per wave; every other P (brief_one) gathers in table order.  Both evaluators
// are in k_brief_core.inc, which k_steer.hip (steered BRIEF: the table of the keypoint's direction) shares.
// The reference computes BRIEF for every raw hit and NMS then discards most of them; this
// path computes it for the survivors only, which gives the same descriptors.
#include "pgx_internal.h"
#include "pgx_brief_plan.h"

namespace {

#include "k_brief_core.inc"

// fused path: survivors come as indices (order) into the frame's raw list.  P256 picks brief_256 or brief_one at compile
// time, so that the P == 256 kernel's register count is brief_256's (it runs beside the distance kernel: DESIGN.md section 11).
template <bool P256>
__global__ __launch_bounds__(256) void k_brief_kept(const float *__restrict__ gray, int W, int H,
                                                    const uint32_t *__restrict__ raw_xy,
                                                    const int32_t *__restrict__ raw_score, int raw_cap,
                                                    const uint32_t *__restrict__ order,
                                                    const int32_t *__restrict__ n_kept, int kp_cap,
                                                    const int4 *__restrict__ pairs, const int32_t *__restrict__ plan, int P,
                                                    int words, pgx_keypoint *__restrict__ kp_out, uint32_t *__restrict__ desc_out,
                                                    int32_t *__restrict__ counts_out, int nframes, int out_stride)
{
    __shared__ uint32_t wbuf[4][STRIP_WORDS]; // brief_256: value strip + masks; brief_one: MAX_WORDS + 2 words of it
    // XCD-aware block -> (frame, keypoint block) map: consecutive workgroup ids are dealt round-robin to
    // the 8 XCDs, so id % 8 picks the frame inside a group of 8 frames: all gathers of one frame then go
    // through ONE XCD's L2 instead of eight (speed only; any mapping is correct).
    const int nblk = (kp_cap + 3) / 4;
    const int F8 = (nframes / 8) * 8;
    int f, kb;
    {
        const int Lid = blockIdx.x;
        if (Lid < nblk * F8) {
            const int j = Lid >> 3;
            f = (j / nblk) * 8 + (Lid & 7);
            kb = j % nblk;
        } else {
            const int r = Lid - nblk * F8;
            f = F8 + r / nblk;
            kb = r % nblk;
        }
    }
    const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int k = kb * 4 + wv;
    const int nk = n_kept[f];
    if (kb == 0 && threadIdx.x == 0) counts_out[f] = nk;
    if (k >= nk) return; // wave-uniform
    const uint32_t ri = order[(size_t)f * kp_cap + k];
    const uint32_t xy = raw_xy[(size_t)f * raw_cap + ri];
    const int x = (int)(xy & 0xFFFFu), y = (int)(xy >> 16);
    const float *g = gray + (size_t)f * W * H;
    if (lane == 0) {
        pgx_keypoint kp;
        kp.x = x; kp.y = y; kp.fast_score = raw_score[(size_t)f * raw_cap + ri];
        kp.value = g[(size_t)y * W + x]; // Keypoint.cs:26
        kp_out[(size_t)f * out_stride + k] = kp;
    }
    if (P256) brief_256(g, W, H, x, y, plan, wbuf[wv], desc_out + ((size_t)f * out_stride + k) * 8);
    else brief_one(g, W, H, x, y, pairs, P, words, wbuf[wv], desc_out + ((size_t)f * out_stride + k) * words);
}

template <bool P256>
__global__ __launch_bounds__(256) void k_brief_list(const float *__restrict__ gray, int W, int H,
                                                    const pgx_keypoint *__restrict__ kps, int n,
                                                    const int4 *__restrict__ pairs, const int32_t *__restrict__ plan, int P,
                                                    int words, uint32_t *__restrict__ desc_out)
{
    __shared__ uint32_t wbuf[4][STRIP_WORDS]; // brief_256: value strip + masks; brief_one: MAX_WORDS + 2 words of it
    const int wv = threadIdx.x >> 6;
    const int k = blockIdx.x * 4 + wv;
    if (k >= n) return;
    if (P256) brief_256(gray, W, H, kps[k].x, kps[k].y, plan, wbuf[wv], desc_out + (size_t)k * 8);
    else brief_one(gray, W, H, kps[k].x, kps[k].y, pairs, P, words, wbuf[wv], desc_out + (size_t)k * words);
}

} // namespace

void pgx_launch_brief(hipStream_t s, const float *gray, int F, int W, int H, const uint32_t *raw_xy,
                      const int32_t *raw_score, int raw_cap, const uint32_t *order, const int32_t *n_kept,
                      int kp_cap, const int32_t *pairs, const int32_t *plan, int P, pgx_keypoint *kp_out, uint32_t *desc_out,
                      int32_t *counts_out, int out_stride, const PgxSteer *steer)
{
    if (steer) { // steered mode: k_steer.hip's kernels on the same lists
        pgx_launch_steer(s, gray, F, W, H, raw_xy, raw_score, raw_cap, order, n_kept, kp_cap, *steer, P, kp_out, desc_out, counts_out,
                         out_stride);
        return;
    }
    if (F <= 0 || kp_cap <= 0) return;
    const int words = (P + 31) / 32;
    hipLaunchKernelGGL(P == PGX_PLAN_PAIRS ? k_brief_kept<true> : k_brief_kept<false>, dim3(((kp_cap + 3) / 4) * F), dim3(256), 0, s, gray, W, H, raw_xy, raw_score,
                       raw_cap, order, n_kept, kp_cap, reinterpret_cast<const int4 *>(pairs), plan, P, words, kp_out,
                       desc_out, counts_out, F, out_stride);
}

void pgx_launch_brief_list(hipStream_t s, const float *gray, int W, int H, const pgx_keypoint *kps, int n,
                           const int32_t *pairs, const int32_t *plan, int P, uint32_t *desc_out, const PgxSteer *steer)
{
    if (steer) { pgx_launch_steer_list(s, gray, W, H, kps, n, *steer, P, desc_out); return; }
    if (n <= 0) return;
    const int words = (P + 31) / 32;
    hipLaunchKernelGGL(P == PGX_PLAN_PAIRS ? k_brief_list<true> : k_brief_list<false>, dim3((n + 3) / 4), dim3(256), 0, s, gray, W, H, kps, n,
                       reinterpret_cast<const int4 *>(pairs), plan, P, words, desc_out);
}
