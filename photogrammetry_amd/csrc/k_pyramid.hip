// k_pyramid.hip -- the scale pyramid of the detect chain for gfx950 (pgx_set_pyramid, include/pgx.h; not in the C# reference).
//
// k_pyr_down builds level l of every frame from level l - 1 by rule 3 of the header: a 2-tap bilinear filter per axis at a
// fixed-point source position, nine float32 operations per pixel in the stated order (the library is built with
// -ffp-contract=off, so none is fused).  The kernel is memory-bound: one thread makes four adjacent pixels of one row and
// writes them with ONE 16-byte store where the destination is aligned; a wave is 256 pixels of one row, so the row's y0, y1
// and fy are wave-uniform (scalar registers).  The eight taps per source row of a thread are a span of at most nine
// floats, and the spans of neighbouring lanes and of neighbouring destination rows overlap: L1/L2 serve that, no LDS.
//
// k_pyr_append moves the survivors of levels >= 1 from their per-level lists behind level 0's in the caller's buffers
// (rule 5: coordinates scaled back to level 0), writes every entry's origin and the frame's counts.  An entry's slot is the
// sum of the earlier levels' counts plus its NMS rank: no atomic decides a placement.
#include "pgx_internal.h"

namespace {

// source position of destination index x: q = ((2x + 1) * step - 65536) >> 1 in 16.16
__device__ __forceinline__ void pyr_tap(int x, int step, int n_src, int &i0, int &i1, float &fr)
{
    const long long q = (((long long)(2 * x + 1) * step) - 65536) >> 1;
    i0 = (int)(q >> 16);
    i0 = i0 < n_src - 1 ? i0 : n_src - 1; // never taken for sizes and steps in range (pgx.h); keeps a bad call in bounds
    i1 = i0 + 1 < n_src - 1 ? i0 + 1 : n_src - 1;
    fr = (float)(int)(q & 65535) * 0x1p-16f;
}

__global__ __launch_bounds__(256) void k_pyr_down(const float *__restrict__ src, int Ws, int Hs, float *__restrict__ dst,
                                                  int Wd, int Hd, int step)
{
    const int wv = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int y = (int)blockIdx.y * 4 + wv; // wave-uniform
    const int x4 = ((int)blockIdx.x * 64 + (int)(threadIdx.x & 63)) * 4;
    if (y >= Hd || x4 >= Wd) return;
    int y0, y1;
    float fy;
    pyr_tap(y, step, Hs, y0, y1, fy);
    const float *s = src + (size_t)blockIdx.z * Ws * Hs;
    const float *r0 = s + (size_t)y0 * Ws, *r1 = s + (size_t)y1 * Ws;
    float *o = dst + ((size_t)blockIdx.z * Hd + y) * Wd + x4;
    float v[4];
#pragma unroll
    for (int j = 0; j < 4; j++) {
        const int x = x4 + j < Wd ? x4 + j : Wd - 1; // the row tail repeats its last pixel (not stored)
        int x0, x1;
        float fx;
        pyr_tap(x, step, Ws, x0, x1, fx);
        const float a = r0[x0], b = r0[x1], c = r1[x0], d = r1[x1];
        const float t = a + fx * (b - a);
        const float u = c + fx * (d - c);
        v[j] = t + fy * (u - t);
    }
    if (x4 + 3 < Wd && (reinterpret_cast<uintptr_t>(o) & 15) == 0) {
        *reinterpret_cast<float4 *>(__builtin_assume_aligned(o, 16)) = make_float4(v[0], v[1], v[2], v[3]);
        return;
    }
#pragma unroll 1
    for (int j = 0; j < 4 && x4 + j < Wd; j++) o[j] = v[j]; // the row tail, and rows that start off a 16-byte boundary
}

struct PyrMerge {
    int n_levels, n_run; // levels of the mode; levels that are not empty (the others count 0)
    int W, H;            // level 0
    int scale[8];        // S_l
};

// grid (ceil(tmp_stride / 64), n_run, frames from f0 on); 64 entries of one level of one frame per workgroup
__global__ __launch_bounds__(256) void k_pyr_append(const pgx_keypoint *__restrict__ tmp_kp, const uint32_t *__restrict__ tmp_desc,
                                                    const int32_t *__restrict__ tmp_bins, const int32_t *__restrict__ lvl_counts,
                                                    const int32_t *__restrict__ lvl_nraw, int F, int tmp_stride, int words,
                                                    PyrMerge m, pgx_keypoint *kp, uint32_t *__restrict__ desc,
                                                    int32_t *__restrict__ bins, int32_t *__restrict__ counts,
                                                    int32_t *__restrict__ nraw, int32_t *__restrict__ origin,
                                                    int32_t *__restrict__ stats, int cap, int *status, int f0)
{
    const int f = f0 + (int)blockIdx.z, l = blockIdx.y, k0 = (int)blockIdx.x * 64, tid = threadIdx.x;
    int base = 0;
    for (int j = 0; j < l; j++) base += lvl_counts[j * F + f];
    const int n = lvl_counts[l * F + f];
    if (l == 0 && k0 == 0 && tid == 0) { // the frame's totals
        int total = 0, raw = 0;
        for (int j = 0; j < m.n_levels; j++) {
            const int nj = j < m.n_run ? lvl_counts[j * F + f] : 0, rj = j < m.n_run ? lvl_nraw[j * F + f] : 0;
            if (stats) {
                const int room = cap - total;
                stats[((size_t)f * m.n_levels + j) * 2] = nj < room ? nj : (room > 0 ? room : 0);
                stats[((size_t)f * m.n_levels + j) * 2 + 1] = rj;
            }
            total += nj;
            raw += rj;
        }
        counts[f] = total < cap ? total : cap;
        nraw[f] = raw;
        if (total > cap) atomicOr(status, (int)PGX_ST_KP_CAP);
    }
    int nv = n < cap - base ? n : cap - base; // entries of this level that fit the caller's list
    nv -= k0;                                 // ... from this workgroup's first one
    if (nv <= 0) return;
    if (nv > 64) nv = 64;
    const size_t dst0 = (size_t)f * cap + base + k0;
    if (l == 0) { // level 0 is in place already (the chain wrote it there): only its origin is missing
        if (origin && tid < nv) {
            const pgx_keypoint p = kp[dst0 + tid];
            int32_t *og = origin + (dst0 + tid) * 3;
            og[0] = 0; og[1] = p.x; og[2] = p.y;
        }
        return;
    }
    const size_t src0 = ((size_t)(l - 1) * F + f) * tmp_stride + k0;
    if (tid < nv) {
        pgx_keypoint p = tmp_kp[src0 + tid];
        const int xl = p.x, yl = p.y;
        const long long S = m.scale[l];
        const int x = (int)(((long long)(2 * xl + 1) * S) >> 17), y = (int)(((long long)(2 * yl + 1) * S) >> 17);
        p.x = x < m.W - 1 ? x : m.W - 1;
        p.y = y < m.H - 1 ? y : m.H - 1;
        kp[dst0 + tid] = p;
        if (origin) {
            int32_t *og = origin + (dst0 + tid) * 3;
            og[0] = l; og[1] = xl; og[2] = yl;
        }
        if (bins) bins[dst0 + tid] = tmp_bins[src0 + tid];
    }
    const uint32_t *sd = tmp_desc + src0 * words;
    uint32_t *dd = desc + dst0 * words;
    for (int i = tid; i < nv * words; i += 256) dd[i] = sd[i];
}

} // namespace

void pgx_launch_pyr_down(hipStream_t s, const float *src, int F, int Ws, int Hs, float *dst, int Wd, int Hd, int step_q16)
{
    if (F <= 0 || Wd <= 0 || Hd <= 0) return;
    for (int f0 = 0; f0 < F; f0 += 65535) { // grid.z holds at most 65535 frames
        const int nf = F - f0 < 65535 ? F - f0 : 65535;
        hipLaunchKernelGGL(k_pyr_down, dim3((Wd + 255) / 256, (Hd + 3) / 4, nf), dim3(256), 0, s, src + (size_t)f0 * Ws * Hs, Ws, Hs,
                           dst + (size_t)f0 * Wd * Hd, Wd, Hd, step_q16);
    }
}

void pgx_launch_pyr_append(hipStream_t s, const pgx_keypoint *tmp_kp, const uint32_t *tmp_desc, const int32_t *tmp_bins,
                           const int32_t *lvl_counts, const int32_t *lvl_nraw, int F, int tmp_stride, int words, int n_levels,
                           int n_run, int W, int H, const int32_t *scale, pgx_keypoint *kp, uint32_t *desc, int32_t *bins,
                           int32_t *counts, int32_t *nraw, int32_t *origin, int32_t *stats, int cap, int *status)
{
    if (F <= 0 || tmp_stride <= 0 || n_run <= 0) return;
    PyrMerge m;
    m.n_levels = n_levels; m.n_run = n_run; m.W = W; m.H = H;
    for (int l = 0; l < 8; l++) m.scale[l] = l < n_levels ? scale[l] : 0;
    for (int f0 = 0; f0 < F; f0 += 65535) {
        const int nf = F - f0 < 65535 ? F - f0 : 65535;
        hipLaunchKernelGGL(k_pyr_append, dim3((tmp_stride + 63) / 64, n_run, nf), dim3(256), 0, s, tmp_kp, tmp_desc, tmp_bins,
                           lvl_counts, lvl_nraw, F, tmp_stride, words, m, kp, desc, bins, counts, nraw, origin, stats, cap, status,
                           f0);
    }
}
