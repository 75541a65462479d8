// k_depth.hip -- dense depth maps by a census plane sweep, and the cross-view filter that turns them into a point list
// (pgx_depth_maps_dev, pgx_depth_fuse_dev; include/pgx.h states both rules operation by operation).  Not in the C# reference.
//
// Depth maps, three kernels on the caller's stream:
//   k_dep_census   per frame slot the 9 x 7 census word of every pixel (62 bits as two uint32), from an LDS tile of the grey
//                  image with its clamped halo
//   k_dep_plan     one workgroup per reference: the frame -> slot lookups of its row of d_views, the plane table w_k, and per
//                  source the plane-induced warp A = M_s adj(M_r) / det(M_r), b = p4_s - A p4_r
//   k_dep_sweep<A> one workgroup per 32 x 32 tile of a reference image, four pixels of a column per thread.  Planes go in
//                  chunks of DEP_KC: every pixel of the tile and of its halo of A (coordinates clamped to the image, which is
//                  the rule's clamped box) projects into each source once per plane -- A x is formed once per chunk and
//                  source, the per-plane work is w y + b, two correctly rounded divisions, one 8-byte gather and two
//                  popcounts -- and leaves raw | nvalid << 9 in LDS; after a barrier every thread box-sums the chunk's planes
//                  for its pixels (the row sums shared) and carries in registers each pixel's best key (agg << 8 | k), the
//                  aggregated cost of the plane before and after the best, and nvalid at the best.  There is no cost volume
//                  in memory.  Everything is integer from the census on, and the float64 part is evaluated per pixel in the
//                  rule's order: the bits depend on the inputs only.
// The filter, four kernels:
//   k_fuse_plan    per map the adjugate, det, sign and ||m3|| of its camera, and per source of its row the first row of the call
//                  that has this frame as its reference
//   k_fuse_count   grid-stride over blocks of 256 pixels in (r, v, u) order: back-projection, the agreeing views, the keep flag,
//                  the block's count
//   k_fuse_scan    one workgroup: the exclusive scan of the block counts (block_scan_array: chunks of 256, a running carry)
//   k_fuse_write   the kept pixels of a block at block offset + rank in the block (block_excl_scan): the list is in (r, v, u)
//                  order whatever the grid
// Counters are integer atomics only.  DESIGN.md section 26.
#include "pgx_stage_args.h"
#include "pgx_densecam.h"   // dep_camera, m3_norm, dep_pixel, the filter's camera table and fuse_point: shared with k_cloud.hip

namespace {

constexpr int DEP_NT = 256;            // threads per workgroup of every kernel here
constexpr int DEP_TW = 32, DEP_TH = 32; // the sweep's tile: four pixels per thread, one below the other
constexpr int DEP_KC = 8;              // planes per chunk: one barrier pair and one A x per chunk
constexpr int DEP_DMAX = 256, DEP_SMAX = 8;   // the limits of D and S (pgx.h)
constexpr int DEP_PEN = 31;            // cost of a source that does not see the pixel: half of the 62 bits
constexpr int CEN_TW = 32, CEN_TH = 8; // the census tile
constexpr int FUSE_GRID_MAX = 1024;    // workgroups of k_fuse_count / k_fuse_write, grid-stride beyond

// the lowest slot that holds frame f, -1 if none does or f is no frame number
__device__ __forceinline__ int dep_slot(const DepArgs &a, int f)
{
    if (f < 0 || f >= a.n_frames) return -1;
    if (!a.frame_ids) return f < a.F ? f : -1;
    for (int s = 0; s < a.F; s++)
        if (a.frame_ids[s] == f) return s;
    return -1;
}

__device__ __forceinline__ int clampi(int x, int hi) { return x < 0 ? 0 : (x > hi ? hi : x); }

__global__ __launch_bounds__(DEP_NT) void k_dep_census(const float *__restrict__ gray, int W, int H, uint2 *__restrict__ census)
{
    constexpr int HW = CEN_TW + 8, HH = CEN_TH + 6;
    __shared__ float s_g[HH][HW];
    const int tiles_x = (W + CEN_TW - 1) / CEN_TW;
    const int tx0 = (blockIdx.x % tiles_x) * CEN_TW, ty0 = (blockIdx.x / tiles_x) * CEN_TH;
    const size_t base = (size_t)blockIdx.y * W * H;
    for (int p = threadIdx.x; p < HW * HH; p += DEP_NT) {
        const int hx = p % HW, hy = p / HW;
        s_g[hy][hx] = gray[base + (size_t)clampi(ty0 - 3 + hy, H - 1) * W + clampi(tx0 - 4 + hx, W - 1)];
    }
    __syncthreads();
    const int lx = threadIdx.x % CEN_TW, ly = threadIdx.x / CEN_TW;
    const int u = tx0 + lx, v = ty0 + ly;
    if (u >= W || v >= H) return;
    const float c = s_g[ly + 3][lx + 4];
    unsigned lo = 0, hi = 0;
    int bit = 0;
#pragma unroll
    for (int dy = 0; dy < 7; dy++)
#pragma unroll
        for (int dx = 0; dx < 9; dx++) {
            if (dy == 3 && dx == 4) continue;
            const unsigned b = s_g[ly + dy][lx + dx] < c ? 1u : 0u;
            if (bit < 32) lo |= b << bit; else hi |= b << (bit - 32);
            bit++;
        }
    census[base + (size_t)v * W + u] = make_uint2(lo, hi);
}

__global__ __launch_bounds__(DEP_NT) void k_dep_plan(DepArgs a)
{
    __shared__ double s_adj[9], s_det, s_sn, s_p4[3];
    __shared__ int s_ok;
    const int r = blockIdx.x, t = threadIdx.x;
    const double NaN = __builtin_nan("");
    const int32_t *row = a.views + (size_t)r * (1 + a.S);
    if (t == 0) {
        const int fr = row[0], sl = dep_slot(a, fr);
        double adj[9], det = 0.0;
        bool ok = sl >= 0;
        if (ok) ok = dep_camera(a.P + (size_t)fr * 12, adj, det);
        const double zn = a.range[2 * r], zf = a.range[2 * r + 1];
        ok = ok && zn > 0.0 && zn < zf && isfinite(zf);
        if (ok) {
            const double *p = a.P + (size_t)fr * 12;
#pragma unroll
            for (int k = 0; k < 9; k++) s_adj[k] = adj[k];
            s_det = det;
            s_sn = (det > 0.0 ? 1.0 : -1.0) * m3_norm(p);
            s_p4[0] = p[3]; s_p4[1] = p[7]; s_p4[2] = p[11];
        }
        s_ok = ok;
        a.slot[(size_t)r * (1 + a.S)] = ok ? sl : -1;
        if (r == 0)
            for (int k = 0; k < 8; k++) a.summary[k] = 0;
    }
    __syncthreads();
    const bool ok = s_ok != 0;
    {
        const double izf = 1.0 / a.range[2 * r + 1], izn = 1.0 / a.range[2 * r];
        for (int k = t; k < a.D; k += DEP_NT) {
            double w = NaN;
            if (ok) {
                const double iz = izf + ((double)k / (double)(a.D - 1)) * (izn - izf);
                w = s_sn * (1.0 / iz);
            }
            a.planes[(size_t)r * a.D + k] = w;
            if (a.planes_out) a.planes_out[(size_t)r * a.D + k] = w;
        }
    }
    if (t < a.S) {
        const int fs = row[1 + t];
        int sl = ok ? dep_slot(a, fs) : -1;
        double adj[9], det, wp[12];
        if (sl >= 0 && !dep_camera(a.P + (size_t)fs * 12, adj, det)) sl = -1;
        if (sl >= 0) {
            const double *p = a.P + (size_t)fs * 12;
#pragma unroll
            for (int i = 0; i < 3; i++) {
#pragma unroll
                for (int j = 0; j < 3; j++)
                    wp[3 * i + j] = ((p[4 * i] * s_adj[j] + p[4 * i + 1] * s_adj[3 + j]) + p[4 * i + 2] * s_adj[6 + j]) / s_det;
                wp[9 + i] = p[4 * i + 3] - ((wp[3 * i] * s_p4[0] + wp[3 * i + 1] * s_p4[1]) + wp[3 * i + 2] * s_p4[2]);
            }
        } else {
#pragma unroll
            for (int k = 0; k < 12; k++) wp[k] = NaN;
        }
        a.slot[(size_t)r * (1 + a.S) + 1 + t] = sl;
        const size_t o = ((size_t)r * a.S + t) * 12;
#pragma unroll
        for (int k = 0; k < 12; k++) {
            a.warp[o + k] = wp[k];
            if (a.warp_out) a.warp_out[o + k] = wp[k];
        }
    }
}

template <int A> __global__ __launch_bounds__(DEP_NT) void k_dep_sweep(DepArgs a)
{
    constexpr int HW = DEP_TW + 2 * A, HH = DEP_TH + 2 * A, NP = HW * HH;
    constexpr int PPT = DEP_TH / (DEP_NT / DEP_TW);   // tile pixels per thread, one below the other
    __shared__ unsigned short s_raw[DEP_KC][NP];
    __shared__ double s_pl[DEP_DMAX], s_wp[DEP_SMAX * 12];   // the reference's plane table and warps: held in LDS, not in scalar registers
    __shared__ int s_cnt[8];
    const int W = a.W, H = a.H, D = a.D, S = a.S, r = blockIdx.y, t = threadIdx.x;
    const int tiles_x = (W + DEP_TW - 1) / DEP_TW;
    const int tx0 = (blockIdx.x % tiles_x) * DEP_TW, ty0 = (blockIdx.x / tiles_x) * DEP_TH;
    const int lx = t % DEP_TW, ly0 = (t / DEP_TW) * PPT, u = tx0 + lx, v0 = ty0 + ly0;
    const size_t npix = (size_t)W * H;
    const int32_t *slots = a.slot + (size_t)r * (1 + S);
    const int sr = slots[0];
    const double NaN = __builtin_nan("");
    if (t < 8) s_cnt[t] = 0;
    for (int k = t; k < D; k += DEP_NT) s_pl[k] = a.planes[(size_t)r * D + k];
    if (t < S * 12) s_wp[t] = a.warp[(size_t)r * S * 12 + t];
    __syncthreads();

    unsigned best[PPT];
    int bestk[PPT], prev[PPT], before[PPT], after[PPT], nvb[PPT];
#pragma unroll
    for (int j = 0; j < PPT; j++) { best[j] = 0xFFFFFFFFu; bestk[j] = -2; prev[j] = 0; before[j] = 0; after[j] = 0; nvb[j] = 0; }
    if (sr >= 0) {   // else NOCAMERA for the whole map: workgroup-uniform
        const uint2 *cen_r = a.census + (size_t)sr * npix;
        for (int k0 = 0; k0 < D; k0 += DEP_KC) {
            for (int p = t; p < NP; p += DEP_NT) {
                const int x = clampi(tx0 - A + p % HW, W - 1), y = clampi(ty0 - A + p / HW, H - 1);
                const uint2 cr = cen_r[(size_t)y * W + x];
                const double du = (double)x, dv = (double)y;
                int acc[DEP_KC];
#pragma unroll
                for (int kk = 0; kk < DEP_KC; kk++) acc[kk] = 0;
                for (int s = 0; s < S; s++) {
                    const int ss = slots[1 + s];
                    if (ss < 0) {
#pragma unroll
                        for (int kk = 0; kk < DEP_KC; kk++) acc[kk] += DEP_PEN;
                        continue;
                    }
                    const double *wp = s_wp + s * 12;
                    const double y0 = (wp[0] * du + wp[1] * dv) + wp[2];
                    const double y1 = (wp[3] * du + wp[4] * dv) + wp[5];
                    const double y2 = (wp[6] * du + wp[7] * dv) + wp[8];
                    const double b0 = wp[9], b1 = wp[10], b2 = wp[11];
                    const uint2 *cen_s = a.census + (size_t)ss * npix;
#pragma unroll
                    for (int kk = 0; kk < DEP_KC; kk++) {
                        if (k0 + kk < D) {
                            const double w = s_pl[k0 + kk];
                            int iu, iv, c = DEP_PEN;
                            if (dep_pixel(w * y0 + b0, w * y1 + b1, w * y2 + b2, W, H, iu, iv)) {
                                const uint2 cs = cen_s[(size_t)iv * W + iu];
                                c = __popc(cr.x ^ cs.x) + __popc(cr.y ^ cs.y) + (1 << 9);
                            }
                            acc[kk] += c;
                        }
                    }
                }
#pragma unroll
                for (int kk = 0; kk < DEP_KC; kk++) s_raw[kk][p] = (unsigned short)acc[kk];
            }
            __syncthreads();
#pragma unroll
            for (int kk = 0; kk < DEP_KC; kk++) {
                if (k0 + kk < D) {
                    const int k = k0 + kk;
                    int rs[PPT + 2 * A];   // the row sums that the thread's PPT boxes share
#pragma unroll
                    for (int i = 0; i < PPT + 2 * A; i++) {
                        rs[i] = 0;
#pragma unroll
                        for (int dx = 0; dx <= 2 * A; dx++) rs[i] += s_raw[kk][(ly0 + i) * HW + lx + dx] & 511;
                    }
#pragma unroll
                    for (int j = 0; j < PPT; j++) {
                        int agg = 0;
#pragma unroll
                        for (int dy = 0; dy <= 2 * A; dy++) agg += rs[j + dy];
                        const int nv = s_raw[kk][(ly0 + j + A) * HW + lx + A] >> 9;
                        if (k == bestk[j] + 1) after[j] = agg;
                        const unsigned key = ((unsigned)agg << 8) | (unsigned)k;
                        if (key < best[j]) {   // ties go to the smaller k
                            best[j] = key;
                            bestk[j] = k;
                            before[j] = prev[j];
                            nvb[j] = nv;
                        }
                        prev[j] = agg;
                    }
                }
            }
            __syncthreads();
        }
    }
    int cnt[6] = {0, 0, 0, 0, 0, 0};
#pragma unroll
    for (int j = 0; j < PPT; j++) {
        const int v = v0 + j;
        if (u >= W || v >= H) continue;
        int fl = 0, kq = -1;
        const int ag = (int)(best[j] >> 8);
        double dep = NaN;
        if (sr < 0) {
            fl = PGX_DEP_NOCAMERA;
        } else {
            if (nvb[j] < a.min_views) fl |= PGX_DEP_NOVIEWS;
            if (bestk[j] == 0 || bestk[j] == D - 1) fl |= PGX_DEP_EDGE;
            if (ag > a.max_cost) fl |= PGX_DEP_HIGHCOST;
        }
        if (fl == 0) {
            const int n = before[j] - after[j], den = before[j] - 2 * ag + after[j];
            int off = 0;
            if (den != 0) {
                const int m = ((n < 0 ? -n : n) * 128) / den;
                off = n < 0 ? -m : m;
            }
            kq = 256 * bestk[j] + off;
            const double izf = 1.0 / a.range[2 * r + 1], izn = 1.0 / a.range[2 * r];
            dep = 1.0 / (izf + (((double)kq / 256.0) / (double)(D - 1)) * (izn - izf));
        }
        const size_t o = (size_t)r * npix + (size_t)v * W + u;
        a.kq8[o] = kq;
        a.depth[o] = dep;
        a.flags[o] = fl;
        if (a.cost && sr >= 0) a.cost[o] = ag;
        cnt[0]++;
        cnt[1] += fl == 0;
#pragma unroll
        for (int b = 0; b < 4; b++) cnt[2 + b] += (fl >> b) & 1;
    }
#pragma unroll
    for (int b = 0; b < 6; b++)
        if (cnt[b]) atomicAdd(&s_cnt[b], cnt[b]);
    __syncthreads();
    if (t < 6 && s_cnt[t]) atomicAdd(&a.summary[t], s_cnt[t]);
    if (t == 6 && sr < 0 && blockIdx.x == 0) atomicAdd(&a.summary[6], 1);
}

// ---- the cross-view filter --------------------------------------------------------------------------------------------

__global__ __launch_bounds__(DEP_NT) void k_fuse_plan(FuseArgs a)
{
    const int r = blockIdx.x, t = threadIdx.x;
    if (t == 0) {
        fuse_camera_row(a.P, a.n_frames, a.views[(size_t)r * (1 + a.S)], a.cam + (size_t)r * FUSE_CAM);
        if (r == 0) { a.summary[1] = 0; a.summary[2] = 0; }
    }
    if (t < a.S) {
        const int f = a.views[(size_t)r * (1 + a.S) + 1 + t];
        int rr = -1;
        if (f >= 0 && f < a.n_frames) {
            for (int j = 0; j < a.R; j++)
                if (a.views[(size_t)j * (1 + a.S)] == f) { rr = j; break; }
            double adj[9], det;
            if (rr >= 0 && !dep_camera(a.P + (size_t)f * 12, adj, det)) rr = -1;
        }
        a.rowof[(size_t)r * a.S + t] = rr;
    }
}

__global__ __launch_bounds__(DEP_NT) void k_fuse_count(FuseArgs a)
{
    __shared__ int s_sum[4];
    const int npix = a.W * a.H, N = a.R * npix;
    for (int b = blockIdx.x; b < a.nb; b += gridDim.x) {
        const int i = b * DEP_NT + (int)threadIdx.x;
        int keep = 0, has = 0, any = 0;
        if (i < N) {
            const int r = i / npix, pix = i - r * npix, v = pix / a.W, u = pix - v * a.W;
            const double z = a.depth[i];
            const double *c = a.cam + (size_t)r * FUSE_CAM;
            int ag = -1;
            if (c[12] != 0.0 && isfinite(z)) {
                has = 1;
                ag = 0;
                double X0, X1, X2;
                fuse_point(c, a.P + (size_t)a.views[(size_t)r * (1 + a.S)] * 12, u, v, z, X0, X1, X2);
                for (int s = 0; s < a.S; s++) {
                    const int rr = a.rowof[(size_t)r * a.S + s];
                    if (rr < 0) continue;
                    const double *p = a.P + (size_t)a.views[(size_t)rr * (1 + a.S)] * 12;
                    const double *cj = a.cam + (size_t)rr * FUSE_CAM;
                    const double q0 = ((p[0] * X0 + p[1] * X1) + p[2] * X2) + p[3];
                    const double q1 = ((p[4] * X0 + p[5] * X1) + p[6] * X2) + p[7];
                    const double q2 = ((p[8] * X0 + p[9] * X1) + p[10] * X2) + p[11];
                    int iu, iv;
                    if (!dep_pixel(q0, q1, q2, a.W, a.H, iu, iv)) continue;
                    any = 1;
                    const double zj = a.depth[(size_t)rr * npix + (size_t)iv * a.W + iu];
                    const double d = (cj[10] * q2) / cj[11];
                    if (isfinite(zj) && fabs(d - zj) <= a.rel_tol * zj) ag++;
                }
                keep = ag >= a.min_agree;
            }
            if (a.agree) a.agree[i] = ag;
        }
        a.keep[(size_t)b * DEP_NT + threadIdx.x] = (unsigned char)keep;
        const int nk = block_sum_i(keep, s_sum), nh = block_sum_i(has, s_sum), na = block_sum_i(any, s_sum);
        if (threadIdx.x == 0) {
            a.bsum[b] = nk;
            if (nh) atomicAdd(&a.summary[1], nh);
            if (na) atomicAdd(&a.summary[2], na);
        }
    }
}

__global__ __launch_bounds__(DEP_NT) void k_fuse_scan(FuseArgs a)
{
    __shared__ int s_lds[DEP_NT / 64];
    const int carry = block_scan_array<int, DEP_NT>(a.bsum, a.boff, a.nb, s_lds);
    int skipped = 0;
    for (int r = threadIdx.x; r < a.R; r += DEP_NT) skipped += a.cam[(size_t)r * FUSE_CAM + 12] == 0.0;
    skipped = block_sum_i(skipped, s_lds);
    if (threadIdx.x == 0) {
        a.summary[0] = carry;
        a.summary[3] = skipped;
        if (carry > a.max_points) atomicOr(a.status, (int)PGX_ST_DEP_CAP);
    }
}

__global__ __launch_bounds__(DEP_NT) void k_fuse_write(FuseArgs a)
{
    __shared__ int s_lds[DEP_NT / 64];
    const int npix = a.W * a.H;
    for (int b = blockIdx.x; b < a.nb; b += gridDim.x) {
        const int i = b * DEP_NT + (int)threadIdx.x;
        const int keep = a.keep[(size_t)b * DEP_NT + threadIdx.x];
        int tot;
        const int idx = a.boff[b] + block_excl_scan<int, DEP_NT>(keep, s_lds, tot);
        if (keep && idx < a.max_points) {
            const int r = i / npix, pix = i - r * npix, v = pix / a.W, u = pix - v * a.W;
            double X0, X1, X2;
            fuse_point(a.cam + (size_t)r * FUSE_CAM, a.P + (size_t)a.views[(size_t)r * (1 + a.S)] * 12, u, v, a.depth[i], X0, X1, X2);
            a.xyz[3 * (size_t)idx + 0] = X0;
            a.xyz[3 * (size_t)idx + 1] = X1;
            a.xyz[3 * (size_t)idx + 2] = X2;
            a.src[2 * (size_t)idx + 0] = r;
            a.src[2 * (size_t)idx + 1] = pix;
        }
    }
}

// the workspaces, described once: the arguments' workspace pointers (none valid for ws = nullptr) and the bytes
size_t dep_carve(DepArgs &a, void *ws)
{
    WsCarver w(ws);
    a.census = w.take<uint2>((size_t)a.F * a.W * a.H * sizeof(uint2));
    a.warp = w.take<double>((size_t)a.R * a.S * 12 * sizeof(double));
    a.slot = w.take<int32_t>((size_t)a.R * (1 + a.S) * sizeof(int32_t));
    a.planes = w.take<double>((size_t)a.R * a.D * sizeof(double));
    return w.total();
}

size_t fuse_carve(FuseArgs &a, void *ws)
{
    WsCarver w(ws);
    a.nb = (int)(((long long)a.R * a.W * a.H + DEP_NT - 1) / DEP_NT);
    a.cam = w.take<double>((size_t)a.R * FUSE_CAM * sizeof(double));
    a.rowof = w.take<int32_t>((size_t)a.R * a.S * sizeof(int32_t));
    a.keep = w.take<unsigned char>((size_t)a.nb * DEP_NT);
    a.bsum = w.take<int32_t>((size_t)a.nb * sizeof(int32_t));
    a.boff = w.take<int32_t>((size_t)a.nb * sizeof(int32_t));
    return w.total();
}

} // namespace

size_t pgx_depth_ws_bytes(const DepArgs &a)
{
    DepArgs b = a;
    return dep_carve(b, nullptr);
}

void pgx_launch_depth_maps(pgx_ctx *ctx, hipStream_t s, DepArgs a, int agg_radius, void *ws)
{
    const int W = a.W, H = a.H;
    dep_carve(a, ws);
    {
        ProfScope ps(ctx, "depth_census", s);
        const unsigned tiles = (unsigned)(((W + CEN_TW - 1) / CEN_TW) * ((H + CEN_TH - 1) / CEN_TH));
        hipLaunchKernelGGL(k_dep_census, dim3(tiles, (unsigned)a.F), dim3(DEP_NT), 0, s, a.gray, W, H, a.census);
    }
    {
        ProfScope ps(ctx, "depth_plan", s);
        hipLaunchKernelGGL(k_dep_plan, dim3((unsigned)a.R), dim3(DEP_NT), 0, s, a);
    }
    {
        ProfScope ps(ctx, "depth_sweep", s);
        const dim3 grid((unsigned)(((W + DEP_TW - 1) / DEP_TW) * ((H + DEP_TH - 1) / DEP_TH)), (unsigned)a.R);
        switch (agg_radius) {
        case 0: hipLaunchKernelGGL(k_dep_sweep<0>, grid, dim3(DEP_NT), 0, s, a); break;
        case 1: hipLaunchKernelGGL(k_dep_sweep<1>, grid, dim3(DEP_NT), 0, s, a); break;
        case 2: hipLaunchKernelGGL(k_dep_sweep<2>, grid, dim3(DEP_NT), 0, s, a); break;
        default: hipLaunchKernelGGL(k_dep_sweep<3>, grid, dim3(DEP_NT), 0, s, a); break;
        }
    }
}

size_t pgx_depth_fuse_ws_bytes(const FuseArgs &a)
{
    FuseArgs b = a;
    return fuse_carve(b, nullptr);
}

void pgx_launch_depth_fuse(pgx_ctx *ctx, hipStream_t s, FuseArgs a, void *ws)
{
    fuse_carve(a, ws);
    ProfScope ps(ctx, "depth_fuse", s);
    const unsigned grid = (unsigned)(a.nb < FUSE_GRID_MAX ? a.nb : FUSE_GRID_MAX);
    hipLaunchKernelGGL(k_fuse_plan, dim3((unsigned)a.R), dim3(DEP_NT), 0, s, a);
    hipLaunchKernelGGL(k_fuse_count, dim3(grid), dim3(DEP_NT), 0, s, a);
    hipLaunchKernelGGL(k_fuse_scan, dim3(1), dim3(DEP_NT), 0, s, a);
    hipLaunchKernelGGL(k_fuse_write, dim3(grid), dim3(DEP_NT), 0, s, a);
}
