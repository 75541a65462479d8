// k_fast.hip -- the reference's FAST-like segment test + raster-order compaction, gfx950.
//
// Reference: ImageProcessing/KeypointDetection.cs:42-138 with its three quirks kept
// (SURVEY D7): ring entry 15 is (-3,+1) again, "different" is |delta| >= T in either
// direction, FastScore = longest circular run of "different" samples (12..16).
//
// Bit formulation (equivalent to the C# state machine, checked against the oracle):
//   S = 16-bit mask of "similar" ring samples.  The pre-test (<= 1 similar among entries
//   0,4,8,12) and the "fifth similar rejects" rule are both implied by "longest run >= 12",
//   so score = longest circular run of zero bits of S if that is >= 12, else none.
//
// k_fast_planes is HBM-bound: 4 B/px grey read (+ 0.5 B/px of ballot planes written).  On the batch path's level 0 the grey
// plane is never read back: k_dewarp_fast gathers the tile's source pixels through the map's gather plan (k_image.hip,
// k_dewarp_plan), greys them into the LDS tile, stores the tile's interior for BRIEF and runs the same two passes
// (fast_tile below: one body for both kernels).  Three launches:
//   k_fast_planes   64x32-pixel tiles staged through LDS (halo 3).  Pass 1, one lane per pixel: the four
//                   compass samples; pixels with at most one similar compass sample are queued in LDS.
//                   Pass 2, one lane per QUEUED pixel (all lanes busy): the rest of the ring and the
//                   run-length rule; score bits are OR-ed into the tile's three ballot planes in LDS.
//                   Per 64-pixel row segment: three 64-bit planes + the count -> seg[F][H][ntx][4]
//   k_seg_scan      one workgroup per frame: exclusive scan (in place) of the dense per-segment counts that
//                   k_fast_planes also writes, in (y, tx) order = raster order; n_raw[f]
//   k_fast_compact  one thread per segment walks its set bits in x order -> raw_xy/raw_score
#include "pgx_internal.h"
#include "pgx_pixel.h"

namespace {

constexpr int TW = 64, TH = 32, HALO = 3;
constexpr int LROWS = TH + 2 * HALO;  // 38
constexpr int LSTRIDE = 72;           // >= 70, keeps rows 16-B aligned
constexpr int NR = (LROWS + 3) / 4;   // 10: tile rows per wave

// The two FAST passes and the write-out of one staged tile (tx, ty) of frame f, for k_fast_planes and k_dewarp_fast alike.
// The caller has cleared planes and *qcount and filled tile; both are ordered before pass 1 by the barrier in here.
__device__ __forceinline__ void fast_tile(const float (*tile)[LSTRIDE], uint16_t *queue, unsigned (*planes)[3][2],
                                          unsigned *qcount, int tx, int ty, int f, int W, int H, float T,
                                          unsigned long long *__restrict__ seg, int ntx, uint32_t *__restrict__ segcnt)
{
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    __syncthreads();

    // Pass 1, every pixel: the four compass samples (:116-133).  A pixel goes on only with at most one of them
    // similar (14 % of the pixels of a textured frame, but almost every 64-pixel row has one: testing the
    // whole ring per wavefront row would run the long path at 14 % lane use).  Survivors are queued in LDS.
    const int x = tx * TW + lane;
    const bool xin = x >= 3 && x < W - 3; // KeypointDetection.cs:45-47
#pragma unroll 1
    for (int k = 0; k < TH / 4; k++) {
        const int ry = wv * (TH / 4) + k;
        const int y = ty * TH + ry;
        if (y >= H) break; // wave-uniform
        bool pass = false;
        unsigned cb = 0;
        if (xin && y >= 3 && y < H - 3) {
            const float c = tile[ry + 3][lane + 3];
            const float lo = __fsub_rn(c, T), hi = __fadd_rn(c, T); // :137, one rounding each
#define PGX_SIM(dx, dy) ((tile[ry + 3 + (dy)][lane + 3 + (dx)] > lo) & (tile[ry + 3 + (dy)][lane + 3 + (dx)] < hi))
            const unsigned s0 = PGX_SIM(-3, 0), s4 = PGX_SIM(0, 3), s8 = PGX_SIM(3, 0), s12 = PGX_SIM(0, -3);
#undef PGX_SIM
            pass = s0 + s4 + s8 + s12 <= 1u;
            cb = s0 | (s4 << 1) | (s8 << 2) | (s12 << 3);
        }
        const unsigned long long pm = __ballot(pass);
        if (pm) {
            unsigned base = 0;
            if (lane == 0) base = atomicAdd(qcount, (unsigned)__popcll(pm));
            base = (unsigned)__shfl((int)base, 0);
            if (pass) queue[base + (unsigned)__popcll(pm & ((1ull << lane) - 1ull))] = (uint16_t)((ry << 10) | (lane << 4) | cb);
        }
    }
    __syncthreads();

    // Pass 2, queued pixels only, all lanes busy: the other ring samples and the run-length rule; the
    // score bits go into the tile's ballot planes with LDS atomics (order-independent, so deterministic).
    const unsigned nq = *qcount;
    for (unsigned e = threadIdx.x; e < nq; e += 256) {
        const unsigned q = queue[e];
        const int ry = (int)(q >> 10), lx = (int)((q >> 4) & 63u);
        const float c = tile[ry + 3][lx + 3];
        const float lo = __fsub_rn(c, T), hi = __fadd_rn(c, T);
#define PGX_SIM(dx, dy) ((unsigned)((tile[ry + 3 + (dy)][lx + 3 + (dx)] > lo) & (tile[ry + 3 + (dy)][lx + 3 + (dx)] < hi)))
        unsigned S = (q & 1u) | ((q & 2u) << 3) | ((q & 4u) << 6) | ((q & 8u) << 9); // ring entries 0, 4, 8, 12
        const unsigned s1 = PGX_SIM(-3, 1);
        S |= s1 << 1;
        S |= PGX_SIM(-2, 2) << 2;
        S |= PGX_SIM(-1, 3) << 3;
        S |= PGX_SIM(1, 3) << 5;
        S |= PGX_SIM(2, 2) << 6;
        S |= PGX_SIM(3, 1) << 7;
        S |= PGX_SIM(3, -1) << 9;
        S |= PGX_SIM(2, -2) << 10;
        S |= PGX_SIM(1, -3) << 11;
        S |= PGX_SIM(-1, -3) << 13;
        S |= PGX_SIM(-2, -2) << 14;
        S |= s1 << 15; // entry 15 = (-3, 1) again (:18)
#undef PGX_SIM
        int score = 0;
        if (S == 0u) {
            score = 16;
        } else { // longest circular run of "different" samples, kept when >= 12 (:65-113)
            const unsigned D = ~S & 0xFFFFu;
            const unsigned dd = D | (D << 16);
            const unsigned x1 = dd & (dd >> 1);
            const unsigned x2 = x1 & (x1 >> 2);
            const unsigned x3 = x2 & (x2 >> 4);
            const unsigned t12 = x3 & (x2 >> 8);
            if (t12) {
                const unsigned t13 = t12 & (dd >> 12);
                const unsigned t14 = t13 & (dd >> 13);
                const unsigned t15 = t14 & (dd >> 14);
                score = 12 + (t13 != 0u) + (t14 != 0u) + (t15 != 0u);
            }
        }
        if (score) {
            const int code = score - 11; // 1..5
            const unsigned bit = 1u << (lx & 31);
            unsigned *pw = &planes[ry][0][lx >> 5];
            if (code & 1) atomicOr(pw, bit);
            if (code & 2) atomicOr(pw + 2, bit);
            if (code & 4) atomicOr(pw + 4, bit);
        }
    }
    __syncthreads();

    if (threadIdx.x < TH) {
        const int ry = threadIdx.x, y = ty * TH + ry;
        if (y < H) {
            const unsigned long long b0 = planes[ry][0][0] | ((unsigned long long)planes[ry][0][1] << 32);
            const unsigned long long b1 = planes[ry][1][0] | ((unsigned long long)planes[ry][1][1] << 32);
            const unsigned long long b2 = planes[ry][2][0] | ((unsigned long long)planes[ry][2][1] << 32);
            unsigned long long *o = seg + (((size_t)f * H + y) * ntx + tx) * 4;
            *reinterpret_cast<ulonglong2 *>(o) = make_ulonglong2(b0, b1);
            const uint32_t cnt = (uint32_t)__popcll(b0 | b1 | b2);
            *reinterpret_cast<ulonglong2 *>(o + 2) = make_ulonglong2(b2, (unsigned long long)cnt);
            segcnt[((size_t)f * H + y) * ntx + tx] = cnt; // dense copy of the counts: k_seg_scan turns it into offsets in place
        }
    }
}

__global__ __launch_bounds__(256) void k_fast_planes(const float *__restrict__ gray, int W, int H, float T,
                                                     unsigned long long *__restrict__ seg, int ntx,
                                                     uint32_t *__restrict__ segcnt)
{
    __shared__ float tile[LROWS][LSTRIDE];
    __shared__ uint16_t queue[TW * TH];  // pixels that passed the compass test: row << 10 | column << 4 | compass bits
    __shared__ unsigned planes[TH][3][2]; // score bit planes of the tile, one 64-bit word per row and plane
    __shared__ unsigned qcount;
    const int tx = blockIdx.x, ty = blockIdx.y, f = blockIdx.z;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const float *g = gray + (size_t)f * W * H;
    const int x0 = tx * TW - HALO, y0 = ty * TH - HALO;
    if (threadIdx.x < TH * 6) (&planes[0][0][0])[threadIdx.x] = 0u;
    if (threadIdx.x == 0) qcount = 0u;

    // each wave owns tile rows wv, wv+4, ...; all global loads are issued before the first LDS store
    // (a load -> store loop serialises six HBM round trips per workgroup)
    {
        float v[NR], hv[NR];
#pragma unroll
        for (int k = 0; k < NR; k++) {
            const int r = wv + 4 * k;
            const int gy = y0 + r;
            const bool rowok = r < LROWS && gy >= 0 && gy < H;
            const float *grow = g + (size_t)(rowok ? gy : 0) * W;
            const int gx = x0 + lane, hx = x0 + 64 + lane;
            v[k] = (rowok && gx >= 0 && gx < W) ? grow[gx] : 0.0f;
            hv[k] = (rowok && lane < 2 * HALO && hx < W) ? grow[hx] : 0.0f;
        }
#pragma unroll
        for (int k = 0; k < NR; k++) {
            const int r = wv + 4 * k;
            if (r < LROWS) {
                tile[r][lane] = v[k];
                if (lane < 2 * HALO) tile[r][64 + lane] = hv[k];
            }
        }
    }
    fast_tile(tile, queue, planes, &qcount, tx, ty, f, W, H, T, seg, ntx, segcnt);
}

// ---- dewarp + grey + FAST in one tile kernel (the batch path's level 0) ---------------------------------------------
// One workgroup owns one 64x32 tile of one frame.  Per wave the tile rows wv, wv + 4, ... (lane = column), and one position
// of the 38 x 6 halo strip on the right per thread.  A position's source offset comes from the map's gather plan, or is the
// pixel's own when no map is set; PGX_GATHER_OOB for a source outside the image and for tile positions outside it, which
// read as grey of (0,0,0,0) = 0.0f: what k_dewarp_gray writes and k_fast_planes pads with.  The rows are gathered GB at a
// time, plan words first and then the pixels (the register budget beside k_ham_fp4 is 32, and ten rows of pixels in flight
// alone are 20), greyed by gray_of into the LDS tile, the tile's interior goes to the grey plane (BRIEF and the pyramid
// read it), and fast_tile does the rest.  The offsets are not kept for a second frame: they would be live across
// fast_tile's 30 registers.
// Workgroup order: the grid is 1-D and the XCD that id % 8 selects (pgx_xcd_map's observation; speed only, any order is
// correct) walks a contiguous run of (frame group, ty, tx, frame in group) with FG frames to the group: a tile's plan
// words serve FG workgroups from one L2, and so do the halo pixels that two neighbouring tiles both gather.
constexpr int FG = 8;  // frames that share a tile's plan words back to back
constexpr int GB = NR / 2; // tile rows per wave gathered at a time
constexpr int HALO_N = LROWS * 2 * HALO; // 228 halo positions, one per thread

template <bool HAS_MAP, bool SRC8>
__attribute__((amdgpu_num_vgpr(16))) // = 32 registers (the attribute counts half on gfx90a and later, as at k_ham_fp4)
__global__ __launch_bounds__(256) void k_dewarp_fast(const typename SrcPix<SRC8>::type *__restrict__ rgba,
                                                     const uint32_t *__restrict__ plan, const uint32_t *__restrict__ plan_oob,
                                                     int W, int H, int F, float T, float *__restrict__ gray,
                                                     unsigned long long *__restrict__ seg, int ntx, int nty,
                                                     uint32_t *__restrict__ segcnt, int *status)
{
    using Px = typename SrcPix<SRC8>::type;
    __shared__ float tile[LROWS][LSTRIDE];
    __shared__ uint16_t queue[TW * TH];
    __shared__ unsigned planes[TH][3][2];
    __shared__ unsigned qcount;
    if (HAS_MAP && blockIdx.x == 0 && threadIdx.x == 0 && *plan_oob) atomicOr(status, (int)PGX_ST_OOB_SOURCE);
    const int nxy = ntx * nty, ntile = nxy * F;
    const int per_xcd = (ntile + 7) >> 3;
    const int id = (int)(blockIdx.x & 7u) * per_xcd + (int)(blockIdx.x >> 3);
    if (id >= ntile) return; // block-uniform: the grid is 8 * per_xcd
    int f, txy;
    {
        const int FF = (F / FG) * FG; // frames in full groups
        if (id < nxy * FF) {
            const int g = id / (nxy * FG), r = id - g * (nxy * FG);
            txy = r / FG;
            f = g * FG + r % FG;
        } else {
            const int r = id - nxy * FF, nl = F - FF;
            txy = r / nl;
            f = FF + r % nl;
        }
    }
    const int ty = txy / ntx, tx = txy - ty * ntx;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int x0 = tx * TW - HALO, y0 = ty * TH - HALO;
    const size_t npix = (size_t)W * H;
    const Px *src = rgba + (size_t)f * npix;
    float *gout = gray + (size_t)f * npix;
    if (threadIdx.x < TH * 6) (&planes[0][0][0])[threadIdx.x] = 0u;
    if (threadIdx.x == 0) qcount = 0u;

    // this thread's positions: column gx of its wave's rows, and (hx, hy) of the halo strip
    const int gx = x0 + lane;
    const int hr = (int)threadIdx.x / (2 * HALO), hc = TW + (int)threadIdx.x % (2 * HALO);
    const int hx = x0 + hc, hy = y0 + hr; // hx >= 0
    const bool hin = threadIdx.x < HALO_N && hy >= 0 && hy < H && hx < W;
    auto offset_of = [&](int k) { // row k of this wave
        const int r = wv + 4 * k, gy = y0 + r;
        uint32_t o = PGX_GATHER_OOB;
        if (r < LROWS && gy >= 0 && gy < H && gx >= 0 && gx < W) {
            o = (uint32_t)gy * (uint32_t)W + (uint32_t)gx;
            if (HAS_MAP) o = plan[o];
        }
        return o;
    };
    auto pixel_at = [&](uint32_t o) { return o != PGX_GATHER_OOB ? load_px<SRC8>(src + o) : make_uint2(0u, 0u); };
    auto put = [&](int k, uint2 p) { // grey into the tile, and into the grey plane when it is an interior pixel of the image
        const int r = wv + 4 * k, gy = y0 + r;
        if (r < LROWS) {
            const float g = gray_of(p);
            tile[r][lane] = g;
            if (lane >= HALO && r >= HALO && r < TH + HALO && gx < W && gy < H) gout[(uint32_t)gy * (uint32_t)W + (uint32_t)gx] = g;
        }
    };
    // four round trips: plan words and pixels of each half of the rows; the halo travels with the first half
#pragma unroll
    for (int k0 = 0; k0 < NR; k0 += GB) {
        uint32_t off[GB], hoff = PGX_GATHER_OOB;
        uint2 px[GB], hpx = make_uint2(0u, 0u);
#pragma unroll
        for (int j = 0; j < GB; j++) off[j] = offset_of(k0 + j);
        if (k0 == 0 && hin) {
            hoff = (uint32_t)hy * (uint32_t)W + (uint32_t)hx;
            if (HAS_MAP) hoff = plan[hoff];
        }
#pragma unroll
        for (int j = 0; j < GB; j++) px[j] = pixel_at(off[j]);
        if (k0 == 0) hpx = pixel_at(hoff);
#pragma unroll
        for (int j = 0; j < GB; j++) put(k0 + j, px[j]);
        if (k0 == 0 && threadIdx.x < HALO_N) {
            const float g = gray_of(hpx);
            tile[hr][hc] = g;
            if (hc < TW + HALO && hr >= HALO && hr < TH + HALO && hin) gout[(uint32_t)hy * (uint32_t)W + (uint32_t)hx] = g;
        }
    }
    fast_tile(tile, queue, planes, &qcount, tx, ty, f, W, H, T, seg, ntx, segcnt);
}

// exclusive scan of per-segment counts, one 1024-thread workgroup per frame
__global__ __launch_bounds__(1024) void k_seg_scan(int nseg, uint32_t *__restrict__ segoff, int32_t *__restrict__ n_raw,
                                                   int raw_cap, int *status)
{
    __shared__ uint32_t wsum[16];
    __shared__ uint32_t carry_s;
    const int f = blockIdx.x;
    uint32_t *so = segoff + (size_t)f * nseg; // in: counts (written by k_fast_planes), out: exclusive offsets
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    if (tid == 0) carry_s = 0;
    __syncthreads();
    for (int base = 0; base < nseg; base += 1024 * 4) {
        // each thread owns 4 consecutive segments
        const int i0 = base + tid * 4;
        uint32_t c[4];
        if (i0 + 3 < nseg && (nseg & 3) == 0) {
            const uint4 v = *reinterpret_cast<const uint4 *>(so + i0);
            c[0] = v.x; c[1] = v.y; c[2] = v.z; c[3] = v.w;
        } else {
#pragma unroll
            for (int k = 0; k < 4; k++) c[k] = (i0 + k < nseg) ? so[i0 + k] : 0u;
        }
        uint32_t tsum = c[0] + c[1] + c[2] + c[3];
        uint32_t incl = tsum;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            uint32_t v = __shfl_up(incl, d);
            if (lane >= d) incl += v;
        }
        if (lane == 63) wsum[wv] = incl;
        __syncthreads();
        uint32_t woff = 0;
        for (int w = 0; w < wv; w++) woff += wsum[w];
        uint32_t run = carry_s + woff + incl - tsum;
#pragma unroll
        for (int k = 0; k < 4; k++) {
            if (i0 + k < nseg) so[i0 + k] = run;
            run += c[k];
        }
        __syncthreads();
        if (tid == 1023) carry_s = run;
        __syncthreads();
    }
    if (tid == 0) {
        n_raw[f] = (int32_t)carry_s;
        if ((int)carry_s > raw_cap) atomicOr(status, (int)PGX_ST_RAW_CAP);
    }
}

// one THREAD per 64-pixel segment (segments hold ~3 hits on average: a wave per segment would be 2M
// nearly empty waves per 64-frame batch); the thread walks the set bits of its segment in x order
__global__ __launch_bounds__(256) void k_fast_compact(const unsigned long long *__restrict__ seg,
                                                      const uint32_t *__restrict__ segoff, int H, int ntx,
                                                      uint32_t *__restrict__ raw_xy, int32_t *__restrict__ raw_score,
                                                      int raw_cap)
{
    const int f = blockIdx.y;
    const int nseg = H * ntx;
    const int s = blockIdx.x * 256 + threadIdx.x;
    if (s >= nseg) return;
    const unsigned long long *sg = seg + ((size_t)f * nseg + s) * 4;
    const ulonglong2 p01 = *reinterpret_cast<const ulonglong2 *>(sg);
    const unsigned long long b0 = p01.x, b1 = p01.y, b2 = sg[2];
    unsigned long long any = b0 | b1 | b2;
    if (!any) return;
    uint32_t pos = segoff[(size_t)f * nseg + s];
    const int y = s / ntx, tx = s - y * ntx;
    while (any) {
        const int l = __builtin_ctzll(any);
        any &= any - 1;
        if (pos >= (uint32_t)raw_cap) break;
        const int code = (int)((b0 >> l) & 1ull) | ((int)((b1 >> l) & 1ull) << 1) | ((int)((b2 >> l) & 1ull) << 2);
        raw_xy[(size_t)f * raw_cap + pos] = ((uint32_t)y << 16) | (uint32_t)(tx * 64 + l);
        raw_score[(size_t)f * raw_cap + pos] = code + 11;
        pos++;
    }
}

} // namespace

size_t pgx_fast_seg_count(int W, int H) { return (size_t)H * ((W + TW - 1) / TW); }

void pgx_launch_fast(hipStream_t s, const float *gray, int F, int W, int H, float T,
                     unsigned long long *seg, uint32_t *segoff, int32_t *n_raw, uint32_t *raw_xy,
                     int32_t *raw_score, int raw_cap, int *status, bool compact, bool planes)
{
    if (F <= 0 || W <= 0 || H <= 0) return;
    const int ntx = (W + TW - 1) / TW, nty = (H + TH - 1) / TH;
    const int nseg = H * ntx;
    if (planes) // not behind pgx_launch_dewarp_fast: seg and the counts in segoff are there already
        hipLaunchKernelGGL(k_fast_planes, dim3(ntx, nty, F), dim3(256), 0, s, gray, W, H, T, seg, ntx, segoff);
    hipLaunchKernelGGL(k_seg_scan, dim3(F), dim3(1024), 0, s, nseg, segoff, n_raw, raw_cap, status);
    // the raster-order raw lists; the fused path's champion NMS bins straight from the planes and writes the
    // list entries of the few points it keeps itself, so it skips this pass
    if (compact)
        hipLaunchKernelGGL(k_fast_compact, dim3((nseg + 255) / 256, F), dim3(256), 0, s, seg, segoff, H, ntx, raw_xy,
                           raw_score, raw_cap);
}

void pgx_launch_dewarp_fast(hipStream_t s, const void *rgba, int src8, const uint32_t *plan, const uint32_t *plan_oob, int F,
                            int W, int H, float T, float *gray, unsigned long long *seg, uint32_t *segoff, int *status)
{
    if (F <= 0 || W <= 0 || H <= 0) return;
    const int ntx = (W + TW - 1) / TW, nty = (H + TH - 1) / TH;
    const int ntile = ntx * nty * F;
    const dim3 grid((unsigned)(8 * ((ntile + 7) / 8))), block(256);
#define PGX_DF(M, S8) hipLaunchKernelGGL((k_dewarp_fast<M, S8>), grid, block, 0, s, reinterpret_cast<const SrcPix<S8>::type *>(rgba), \
                                         plan, plan_oob, W, H, F, T, gray, seg, ntx, nty, segoff, status)
    if (src8) { if (plan) PGX_DF(true, true); else PGX_DF(false, true); }
    else { if (plan) PGX_DF(true, false); else PGX_DF(false, false); }
#undef PGX_DF
}
