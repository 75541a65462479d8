// k_cloud.hip -- the fused point list merged into one cloud: one point per occupied cell of a grid, with a normal from the
// point's own depth map and the colour of its reference frame (pgx_cloud_merge_dev; include/pgx.h states the rule operation by
// operation).  Not in the C# reference.
//
// Eight kernels on the caller's stream, none of which needs the count of the list on the host:
//   k_cld_plan    clears the cell table (grid-stride); its first workgroup also fills the filter's camera table per map, the
//                 slot that shows each map's frame, and n = min(d_count[0], max_in)
//   k_cld_normals one thread per point: the normal from the point's own map (the pixel's own back-projection and up to four
//                 neighbours').  A kernel of its own: with the insert in the same kernel the scalar registers spilled.
//   k_cld_points  one thread per point: the used test, the cell key and the position in the cell, the colour, and the insert:
//                 an open-addressing table of
//                 1 << lg_table >= 2 max_in entries, linear probing from cld_hash(key), a 64-bit compare-and-swap on the key
//                 (after a plain load: a key, once written, never changes), atomicMin on the cell's first point and atomicAdd
//                 on its count.  What the accumulate pass needs of the point is kept in 16 bytes.
//   k_cld_count   the owners (the first point of a cell that is kept) per block of 256 points, and the cells
//   k_cld_scan    one workgroup: the exclusive scan of the block counts (block_scan_array), the kept count, the capacity
//                 status, d_report
//   k_cld_rank    the owner's rank in its block (block_excl_scan) plus the block's offset is the cell's output index: the
//                 cells come out in the order of their first points with no sort.  The owner clears its cell's accumulators.
//   k_cld_accum   one thread per point: integer atomics into the accumulators of its cell (64-bit sums of p, q and colour);
//                 consecutive lanes of a wave that name the same cell are summed first and go to memory once
//   k_cld_final   one thread per kept cell: the outputs
// Every sum is an integer: no order of execution changes a bit.  DESIGN.md section 28.
#include "pgx_stage_args.h"
#include "pgx_densecam.h"
#include "pgx_cloudkey.h"   // rule 1 (the used test, the key, the position in the cell), the colour slot, the plan's tail: shared with k_mesh.hip

namespace {

constexpr int CLD_NT = 256;            // threads per workgroup of every kernel here; the block of the owner scan
constexpr int CLD_GRID_MAX = 1024;     // workgroups of the per-point kernels, grid-stride beyond
constexpr int CLD_LG_TMIN = 8;         // the table has at least 1 << 8 entries
constexpr int CLD_ACC = 10;            // 64-bit accumulators per kept cell: sp (3), sn (3), sc (3), nn | nc << 32
constexpr unsigned long long CLD_EMPTY = ~0ull;                    // no key: a key has 63 bits
constexpr unsigned long long CLD_HASH_MUL = 0x9E3779B97F4A7C15ull; // cld_hash: the top lg_table bits of key * this (mod 2^64)

__device__ __forceinline__ unsigned cld_hash(unsigned long long key, int lg) { return (unsigned)((key * CLD_HASH_MUL) >> (64 - lg)); }

__global__ __launch_bounds__(CLD_NT) void k_cld_plan(CloudArgs a)
{
    const size_t T = (size_t)1 << a.lg_table;
    for (size_t i = (size_t)blockIdx.x * CLD_NT + threadIdx.x; i < T; i += (size_t)gridDim.x * CLD_NT) {
        a.keys[i] = CLD_EMPTY;
        a.tfirst[i] = 0x7FFFFFFF;
        a.tcnt[i] = 0;
        a.tout[i] = -1;
    }
    if (blockIdx.x != 0) return;
    cld_plan_rows<CLD_NT>(a);
}

// the point of pixel (u2, v2) of map r if it counts as a neighbour of a pixel at depth z
__device__ __forceinline__ bool cld_neighbour(const CloudArgs &a, const double *c, const double *p, const double *dmap, int u2, int v2,
                                              double z, double &X0, double &X1, double &X2)
{
    X0 = X1 = X2 = 0.0;
    if (u2 < 0 || u2 >= a.W || v2 < 0 || v2 >= a.H) return false;
    const double z2 = dmap[(size_t)v2 * a.W + u2];
    if (!isfinite(z2) || !(fabs(z2 - z) <= a.disc_tol * z)) return false;
    fuse_point(c, p, u2, v2, z2, X0, X1, X2);
    return true;
}

// the difference along (du, dv): central, else forward, else backward; false when neither neighbour counts
__device__ __forceinline__ bool cld_diff(const CloudArgs &a, const double *c, const double *p, const double *dmap, int u, int v, int du,
                                         int dv, double z, double C0, double C1, double C2, double &d0, double &d1, double &d2)
{
    double F0, F1, F2, B0, B1, B2;
    const bool f = cld_neighbour(a, c, p, dmap, u + du, v + dv, z, F0, F1, F2);
    const bool b = cld_neighbour(a, c, p, dmap, u - du, v - dv, z, B0, B1, B2);
    if (f && b) { d0 = F0 - B0; d1 = F1 - B1; d2 = F2 - B2; }
    else if (f) { d0 = F0 - C0; d1 = F1 - C1; d2 = F2 - C2; }
    else if (b) { d0 = C0 - B0; d1 = C1 - B1; d2 = C2 - B2; }
    else { d0 = d1 = d2 = 0.0; }
    return f || b;
}

// rule 2 for every point whose src names a pixel of a map (k_cld_points drops the normal of a point that is not used):
// rec[2 i + 1] = q (3 x 16 bits) | has-normal << 63
__global__ __launch_bounds__(CLD_NT) void k_cld_normals(CloudArgs a)
{
    const int n = a.meta[0], nbn = (n + CLD_NT - 1) / CLD_NT, npix = a.W * a.H;
    for (int b = blockIdx.x; b < nbn; b += gridDim.x) {
        const int i = b * CLD_NT + (int)threadIdx.x;
        if (i >= n) continue;
        const int r = a.src[2 * (size_t)i], pix = a.src[2 * (size_t)i + 1];
        unsigned long long rec = 0;
        if (r >= 0 && r < a.R && pix >= 0 && pix < npix) {
            const double *c = a.cam + (size_t)r * FUSE_CAM;
            const double *dmap = a.depth + (size_t)r * npix;
            const int v = pix / a.W, u = pix - v * a.W;
            const double z = dmap[pix];
            if (c[12] != 0.0 && isfinite(z)) {
                const double *p = a.P + (size_t)a.views[(size_t)r * (1 + a.S)] * 12;
                double C0, C1, C2, du0, du1, du2, dv0, dv1, dv2;
                fuse_point(c, p, u, v, z, C0, C1, C2);
                const bool hu = cld_diff(a, c, p, dmap, u, v, a.normal_step, 0, z, C0, C1, C2, du0, du1, du2);
                const bool hv = cld_diff(a, c, p, dmap, u, v, 0, a.normal_step, z, C0, C1, C2, dv0, dv1, dv2);
                const double n0 = du1 * dv2 - du2 * dv1, n1 = du2 * dv0 - du0 * dv2, n2 = du0 * dv1 - du1 * dv0;
                const double fu = (double)u, fv = (double)v;
                const double e0 = (c[0] * fu + c[1] * fv) + c[2], e1 = (c[3] * fu + c[4] * fv) + c[5], e2 = (c[6] * fu + c[7] * fv) + c[8];
                const double s = (n0 * e0 + n1 * e1) + n2 * e2, L = sqrt((n0 * n0 + n1 * n1) + n2 * n2);
                if (hu && hv && isfinite(L) && L != 0.0 && isfinite(s) && s != 0.0) {
                    const bool flip = s > 0.0;
                    const int q0 = (int)floor(((flip ? -n0 : n0) / L) * 32767.0 + 0.5);
                    const int q1 = (int)floor(((flip ? -n1 : n1) / L) * 32767.0 + 0.5);
                    const int q2 = (int)floor(((flip ? -n2 : n2) / L) * 32767.0 + 0.5);
                    rec = (unsigned long long)(q0 & 0xFFFF) | (unsigned long long)(q1 & 0xFFFF) << 16 |
                          (unsigned long long)(q2 & 0xFFFF) << 32 | 1ull << 63;
                }
            }
        }
        a.rec[2 * (size_t)i + 1] = rec;
    }
}

// rec[2 i] = p (3 x 16 bits) | colour byte 2 << 48 | has-normal << 56 | has-colour << 57; rec[2 i + 1] = q | colour bytes 0, 1 << 48
__global__ __launch_bounds__(CLD_NT) void k_cld_points(CloudArgs a)
{
    __shared__ int s_sum[4];
    const int n = a.meta[0], nbn = (n + CLD_NT - 1) / CLD_NT, npix = a.W * a.H;
    const unsigned mask = (1u << a.lg_table) - 1u;
    for (int b = blockIdx.x; b < nbn; b += gridDim.x) {
        const int i = b * CLD_NT + (int)threadIdx.x;
        int used = 0, hasn = 0, hasc = 0;
        if (i < n) {
            int r, pix;
            unsigned long long key, pk;
            const bool ok = cld_point_key(a.xyz, a.src, (size_t)i, a.R, npix, a.cell, a.ox, a.oy, a.oz, r, pix, key, pk);
            int q0 = 0, q1 = 0, q2 = 0, sl = -1;
            if (ok) {
                used = 1;
                const unsigned long long rq = a.rec[2 * (size_t)i + 1];
                hasn = (int)(rq >> 63);
                if (hasn) { q0 = (short)(rq & 0xFFFFull); q1 = (short)((rq >> 16) & 0xFFFFull); q2 = (short)((rq >> 32) & 0xFFFFull); }
                unsigned long long col = 0;
                const int cs = a.cslot[r];
                if (cs >= 0) {
                    hasc = 1;
                    col = a.rgba8[(size_t)cs * npix + pix] & 0xFFFFFFu;
                }
                // the insert: at most table entries probes (the table is never full: it has 2 max_in entries at the least)
                unsigned h = cld_hash(key, a.lg_table);
                for (unsigned tries = 0; tries <= mask; tries++, h = (h + 1) & mask) {
                    unsigned long long prev = __atomic_load_n(&a.keys[h], __ATOMIC_RELAXED);
                    if (prev == CLD_EMPTY) prev = atomicCAS(&a.keys[h], CLD_EMPTY, key);
                    if (prev == CLD_EMPTY || prev == key) { sl = (int)h; break; }
                }
                if (sl >= 0) {
                    atomicMin(&a.tfirst[sl], i);
                    atomicAdd(&a.tcnt[sl], 1);
                } else {
                    atomicOr(a.status, (int)PGX_ST_INTERNAL);
                }
                a.rec[2 * (size_t)i] = pk | (col >> 16) << 48 | (unsigned long long)hasn << 56 | (unsigned long long)hasc << 57;
                a.rec[2 * (size_t)i + 1] = (rq & 0xFFFFFFFFFFFFull) | (col & 0xFFFFull) << 48;
            }
            a.slot[i] = sl;
            if (a.pt_normal) {
                a.pt_normal[3 * (size_t)i] = q0;
                a.pt_normal[3 * (size_t)i + 1] = q1;
                a.pt_normal[3 * (size_t)i + 2] = q2;
            }
        }
        const int nu = block_sum_i(used, s_sum), nn = block_sum_i(hasn, s_sum), nc = block_sum_i(hasc, s_sum);
        if (threadIdx.x == 0) {
            if (nu) atomicAdd(&a.meta[1], nu);
            if (nn) atomicAdd(&a.meta[2], nn);
            if (nc) atomicAdd(&a.meta[3], nc);
        }
    }
}

// point i is the first of its cell (bit 0) and the owner of a kept cell (bit 1); sl = its table entry
__device__ __forceinline__ int cld_owner(const CloudArgs &a, int i, int n, int &sl)
{
    sl = i < n ? a.slot[i] : -1;
    if (sl < 0 || a.tfirst[sl] != i) return 0;
    return a.tcnt[sl] >= a.min_support ? 3 : 1;
}

__global__ __launch_bounds__(CLD_NT) void k_cld_count(CloudArgs a)
{
    __shared__ int s_sum[4];
    const int n = a.meta[0], nbn = (n + CLD_NT - 1) / CLD_NT;
    for (int b = blockIdx.x; b < nbn; b += gridDim.x) {
        int sl;
        const int own = cld_owner(a, b * CLD_NT + (int)threadIdx.x, n, sl);
        const int nk = block_sum_i(own >> 1, s_sum), ncell = block_sum_i(own & 1, s_sum);
        if (threadIdx.x == 0) {
            a.bsum[b] = nk;
            if (ncell) atomicAdd(&a.meta[4], ncell);
        }
    }
}

__global__ __launch_bounds__(CLD_NT) void k_cld_scan(CloudArgs a)
{
    __shared__ int s_lds[CLD_NT / 64];
    const int n = a.meta[0], nbn = (n + CLD_NT - 1) / CLD_NT;
    const int carry = block_scan_array<int, CLD_NT>(a.bsum, a.boff, nbn, s_lds);
    if (threadIdx.x == 0) {
        a.meta[5] = carry;
        if (carry > a.max_points) atomicOr(a.status, (int)PGX_ST_CLD_CAP);
        a.report[0] = n; a.report[1] = a.meta[1]; a.report[2] = n - a.meta[1]; a.report[3] = a.meta[2]; a.report[4] = a.meta[3];
        a.report[5] = a.meta[4]; a.report[6] = carry; a.report[7] = 0;
    }
}

__global__ __launch_bounds__(CLD_NT) void k_cld_rank(CloudArgs a)
{
    __shared__ int s_lds[CLD_NT / 64];
    const int n = a.meta[0], nbn = (n + CLD_NT - 1) / CLD_NT;
    for (int b = blockIdx.x; b < nbn; b += gridDim.x) {
        int sl, tot;
        const int own = cld_owner(a, b * CLD_NT + (int)threadIdx.x, n, sl);
        const int idx = a.boff[b] + block_excl_scan<int, CLD_NT>(own >> 1, s_lds, tot);
        if (own & 1) a.tout[sl] = (own & 2) ? idx : -2;
        if ((own & 2) && idx < a.max_points) {
            a.oslot[idx] = sl;
#pragma unroll
            for (int k = 0; k < CLD_ACC; k++) a.acc[(size_t)idx * CLD_ACC + k] = 0ull;
        }
    }
}

// The lanes of a wave whose neighbours name the same cell (neighbouring pixels of one map do when the cell is larger than a
// pixel's footprint) sum their records first, by a segmented suffix sum over runs of equal cells, and the run's first lane alone
// goes to memory.  A run has at most 64 points, so the sums of a run fit fields of 32 (p, and q + 32768), 14 (colour) and 7 bits
// (counts) of four words.  The sums are integers: the order changes no bit.  (One atomic per point and sum was measured and is
// slower: tools/experiments/cloud_accum_uncombined.patch)
__global__ __launch_bounds__(CLD_NT) void k_cld_accum(CloudArgs a)
{
    const int n = a.meta[0], nbn = (n + CLD_NT - 1) / CLD_NT, lane = threadIdx.x & 63;
    for (int b = blockIdx.x; b < nbn; b += gridDim.x) {
        const int i = b * CLD_NT + (int)threadIdx.x;
        int o = -1;
        unsigned long long r0 = 0, r1 = 0;
        if (i < n) {
            const int sl = a.slot[i];
            o = sl >= 0 ? a.tout[sl] : -1;
            if (a.cell_of) a.cell_of[i] = o;
            if (o >= a.max_points) o = -1;
            if (o >= 0) { r0 = a.rec[2 * (size_t)i]; r1 = a.rec[2 * (size_t)i + 1]; }
        }
        const unsigned long long hasn = (r0 >> 56) & 1ull, hasc = (r0 >> 57) & 1ull;
        // the sign-extended q, moved to 1 .. 65535 so that a run's sum stays a field of non-negative values
        const long long q0 = (short)(r1 & 0xFFFFull), q1 = (short)((r1 >> 16) & 0xFFFFull), q2 = (short)((r1 >> 32) & 0xFFFFull);
        unsigned long long A = (r0 & 0xFFFFull) | ((r0 >> 16) & 0xFFFFull) << 32;
        unsigned long long B = ((r0 >> 32) & 0xFFFFull) | (hasn ? (unsigned long long)(q0 + 32768) : 0ull) << 32;
        unsigned long long C = (hasn ? (unsigned long long)(q1 + 32768) : 0ull) | (hasn ? (unsigned long long)(q2 + 32768) : 0ull) << 32;
        unsigned long long D = hasc ? (((r1 >> 48) & 0xFFull) | ((r1 >> 56) & 0xFFull) << 14 | ((r0 >> 48) & 0xFFull) << 28) : 0ull;
        D |= hasn << 42 | hasc << 49;
        const int prev = __shfl_up(o, 1, 64);
        const bool head = lane == 0 || prev != o;
        const unsigned long long le = lane == 63 ? ~0ull : (2ull << lane) - 1ull;
        const int rid = __popcll(__ballot(head) & le);   // the number of the lane's run in the wave
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const int rid2 = __shfl_down(rid, d, 64);
            const unsigned long long A2 = __shfl_down(A, d, 64), B2 = __shfl_down(B, d, 64), C2 = __shfl_down(C, d, 64),
                                     D2 = __shfl_down(D, d, 64);
            if (lane + d < 64 && rid2 == rid) { A += A2; B += B2; C += C2; D += D2; }
        }
        if (!head || o < 0) continue;
        unsigned long long *acc = a.acc + (size_t)o * CLD_ACC;
        const unsigned long long nn = (D >> 42) & 0x7Full, nc = (D >> 49) & 0x7Full;
        atomicAdd(&acc[0], A & 0xFFFFFFFFull);
        atomicAdd(&acc[1], A >> 32);
        atomicAdd(&acc[2], B & 0xFFFFFFFFull);
        if (nn) {   // two's complement: the sum of the signed q
            atomicAdd(&acc[3], (B >> 32) - 32768ull * nn);
            atomicAdd(&acc[4], (C & 0xFFFFFFFFull) - 32768ull * nn);
            atomicAdd(&acc[5], (C >> 32) - 32768ull * nn);
        }
        if (nc) {
            atomicAdd(&acc[6], D & 0x3FFFull);
            atomicAdd(&acc[7], (D >> 14) & 0x3FFFull);
            atomicAdd(&acc[8], (D >> 28) & 0x3FFFull);
        }
        if (nn | nc) atomicAdd(&acc[9], nn | nc << 32);
    }
}

__global__ __launch_bounds__(CLD_NT) void k_cld_final(CloudArgs a)
{
    const int kept = a.meta[5] < a.max_points ? a.meta[5] : a.max_points;
    const double org[3] = {a.ox, a.oy, a.oz};
    for (int idx = blockIdx.x * CLD_NT + (int)threadIdx.x; idx < kept; idx += (int)gridDim.x * CLD_NT) {
        const int sl = a.oslot[idx];
        const unsigned long long key = a.keys[sl];
        const int cnt = a.tcnt[sl], first = a.tfirst[sl];
        const unsigned long long *acc = a.acc + (size_t)idx * CLD_ACC;
        const int nn = (int)(acc[9] & 0xFFFFFFFFull), nc = (int)(acc[9] >> 32);
#pragma unroll
        for (int k = 0; k < 3; k++) {
            const long long g = (long long)((key >> (21 * (2 - k))) & 0x1FFFFFull) - CLD_GBIAS;
            const long long sp = (long long)acc[k];
            const double m = (double)(2 * sp + cnt) / (double)(2 * (long long)cnt);
            a.out_xyz[3 * (size_t)idx + k] = org[k] + ((double)g + m / 65536.0) * a.cell;
        }
        const double s0 = (double)(long long)acc[3], s1 = (double)(long long)acc[4], s2 = (double)(long long)acc[5];
        const double L = sqrt((s0 * s0 + s1 * s1) + s2 * s2);
        const bool hn = nn != 0 && L != 0.0;
        a.out_normal[3 * (size_t)idx] = hn ? (float)(s0 / L) : 0.0f;
        a.out_normal[3 * (size_t)idx + 1] = hn ? (float)(s1 / L) : 0.0f;
        a.out_normal[3 * (size_t)idx + 2] = hn ? (float)(s2 / L) : 0.0f;
        unsigned col = 0;
        if (nc != 0) {
            const long long d = 2 * (long long)nc;
            col = (unsigned)((2 * (long long)acc[6] + nc) / d) | (unsigned)((2 * (long long)acc[7] + nc) / d) << 8 |
                  (unsigned)((2 * (long long)acc[8] + nc) / d) << 16 | 255u << 24;
        }
        a.out_rgba8[idx] = col;
        a.out_info[4 * (size_t)idx] = cnt;
        a.out_info[4 * (size_t)idx + 1] = nn;
        a.out_info[4 * (size_t)idx + 2] = nc;
        a.out_info[4 * (size_t)idx + 3] = first;
    }
}

// the workspace, described once: the arguments' workspace pointers (none valid for ws = nullptr) and the bytes
size_t cld_carve(CloudArgs &a, void *ws)
{
    WsCarver w(ws);
    a.lg_table = CLD_LG_TMIN;
    while (((size_t)1 << a.lg_table) < 2 * (size_t)a.max_in) a.lg_table++;
    const size_t T = (size_t)1 << a.lg_table, n = (size_t)a.max_in, m = (size_t)a.max_points;
    a.nb = a.max_in > 0 ? (a.max_in + CLD_NT - 1) / CLD_NT : 1;
    a.keys = w.take<unsigned long long>(T * 8);
    a.tfirst = w.take<int32_t>(T * 4);
    a.tcnt = w.take<int32_t>(T * 4);
    a.tout = w.take<int32_t>(T * 4);
    a.cam = w.take<double>((size_t)a.R * FUSE_CAM * sizeof(double));
    a.cslot = w.take<int32_t>((size_t)a.R * 4);
    a.slot = w.take<int32_t>(n * 4);
    a.rec = w.take<unsigned long long>(n * 16);
    a.bsum = w.take<int32_t>((size_t)a.nb * 4);
    a.boff = w.take<int32_t>((size_t)a.nb * 4);
    a.oslot = w.take<int32_t>(m * 4);
    a.acc = w.take<unsigned long long>(m * CLD_ACC * 8);
    a.meta = w.take<int32_t>(8 * 4);
    return w.total();
}

} // namespace

size_t pgx_cloud_ws_bytes(const CloudArgs &a)
{
    CloudArgs b = a;
    return cld_carve(b, nullptr);
}

void pgx_launch_cloud_merge(pgx_ctx *ctx, hipStream_t s, CloudArgs a, void *ws)
{
    cld_carve(a, ws);
    const unsigned grid = (unsigned)(a.nb < CLD_GRID_MAX ? a.nb : CLD_GRID_MAX);
    {
        ProfScope ps(ctx, "cloud_plan", s);
        const size_t tb = ((size_t)1 << a.lg_table) / CLD_NT;
        hipLaunchKernelGGL(k_cld_plan, dim3((unsigned)(tb < CLD_GRID_MAX ? tb : CLD_GRID_MAX)), dim3(CLD_NT), 0, s, a);
    }
    {
        ProfScope ps(ctx, "cloud_normals", s);
        hipLaunchKernelGGL(k_cld_normals, dim3(grid), dim3(CLD_NT), 0, s, a);
    }
    {
        ProfScope ps(ctx, "cloud_points", s);
        hipLaunchKernelGGL(k_cld_points, dim3(grid), dim3(CLD_NT), 0, s, a);
    }
    {
        ProfScope ps(ctx, "cloud_rank", s);
        hipLaunchKernelGGL(k_cld_count, dim3(grid), dim3(CLD_NT), 0, s, a);
        hipLaunchKernelGGL(k_cld_scan, dim3(1), dim3(CLD_NT), 0, s, a);
        hipLaunchKernelGGL(k_cld_rank, dim3(grid), dim3(CLD_NT), 0, s, a);
    }
    {
        ProfScope ps(ctx, "cloud_accum", s);
        hipLaunchKernelGGL(k_cld_accum, dim3(grid), dim3(CLD_NT), 0, s, a);
    }
    if (a.max_points > 0) {
        ProfScope ps(ctx, "cloud_final", s);
        const int fb = (a.max_points + CLD_NT - 1) / CLD_NT;
        hipLaunchKernelGGL(k_cld_final, dim3((unsigned)(fb < CLD_GRID_MAX ? fb : CLD_GRID_MAX)), dim3(CLD_NT), 0, s, a);
    }
}
