// k_meshclean.hip -- the mesh of pgx_mesh_dev cleaned where it lies: the small connected components dropped, the rest smoothed
// without shrinking (Taubin's lambda | mu on fixed-point positions) and its normals taken from the smoothed triangles
// (pgx_mesh_clean_dev; include/pgx.h states the rule operation by operation).  Not in the C# reference.
//
// Kernels on the caller's stream, none of which needs a count on the host:
//   k_mcl_init     nv and nt from d_counts; per vertex the valid test, the fixed-point position, parent[v] = v, zeroes
//   k_mcl_union    one thread per triangle: the used test, the degrees of its vertices, and the union of its vertices' trees: the
//                  lock-free union-find with hashed priorities of the track graph (pgx_trackgraph.h: trk_find, trk_hook)
//   k_mcl_roots    one thread per vertex: its root, into an array of its own
//   k_mcl_count    one thread per used triangle: the triangles and the smallest vertex per root.  A real mesh is ONE large
//                  component, and a global atomicAdd per triangle on its root serialises (about 10 ns each, k_tracks.hip): the
//                  roots are counted in an LDS table (block_tally_add) that lives across the workgroup's grid-stride passes and is
//                  flushed when it may fill and at the end: one global add and one atomicMin per distinct root and flush.  big: the flush's sums
//                  (old + n; the last add of a root gives its total) through an LDS maximum, one global atomicMax per flush
//   k_mcl_bsum     per block of 256 indices: the kept vertices and kept triangles (one 64-bit value), the row entries of the kept
//                  vertices; the components and the kept ones counted at their names
//   k_mcl_scan     one workgroup: the exclusive scans of the block sums (block_scan_array, twice), the totals, the capacity
//                  status, d_report
//   k_mcl_rank     the block's base plus block_excl_scan: new indices in old-index order with no sort; vertex_map, comp, row starts
//   k_mcl_emit     the kept vertices' copied attributes and the kept triangles with their new indices
//   k_mcl_rows     (iters > 0) one thread per kept triangle: its index into the rows of its three vertices (atomic cursor: no
//                  order, and none is needed: every sum over a row is an integer sum)
//   k_mcl_smooth   (per half-step) one thread per kept vertex: the gather over its row from one q buffer into the other; no atomics.
//                  A row of more than MCL_LONG_ROW entries (a fan) is summed by the whole wave, 64 entries at a time: the
//                  sums are integers, so the split changes no bit
//   k_mcl_tnormal  one thread per kept triangle: m of rule 4 on the final q, three 16-bit components in one word
//   k_mcl_finish   one thread per kept vertex: the sum of m over its row, the normal, the position
// DESIGN.md section 30.
#include "pgx_stage_args.h"
#include "pgx_meshlist.h"   // what every stage does to a mesh list: shared with k_meshdecimate.hip

namespace {

constexpr int MCL_NT = 256;             // threads per workgroup of every kernel here; the block of the scans
constexpr int MCL_GRID_MAX = 1024;      // workgroups of the per-vertex and per-triangle kernels, grid-stride beyond
constexpr int MCL_UNION_GRID = 256;     // ... of k_mcl_union and k_mcl_count: one per CU, as k_trk_union's (fewer flushes, fresher trees)
constexpr int MCL_SLOTS = 512;          // LDS aggregation table of k_mcl_count (>= 2 * MCL_NT)
constexpr int MCL_LONG_ROW = 64;        // a row of more entries is summed by the 64 lanes of its vertex's wave, not by its thread alone
constexpr uint32_t MCL_EMPTY = BLOCK_TALLY_EMPTY;   // hkey: block_tally_add (pgx_block.h) claims such an entry
constexpr unsigned long long MCL_NONRM = ~0ull;   // tnrm: the triangle contributes nothing
constexpr int MCL_NOREP = 0x7FFFFFFF;
constexpr double MCL_STEP_MAX = 4611686018427387904.0;   // 2^62: the clamp of a half-step's increment
enum { MC_NV = 0, MC_NT, MC_USED, MC_COMPS, MC_KEPT, MC_VOUT, MC_TOUT, MC_BIG };   // meta

__device__ __forceinline__ uint32_t mcl_prio(int x) { return (uint32_t)x * 2654435761u; }   // a bijection on 32 bits: no ties

__global__ __launch_bounds__(MCL_NT) void k_mcl_init(MeshCleanArgs a)
{
    int nv, nt;
    mesh_counts(a.counts, a.max_vertices, a.max_tris, nv, nt);
    if (blockIdx.x == 0 && threadIdx.x < 8) a.meta[threadIdx.x] = threadIdx.x == MC_NV ? nv : (threadIdx.x == MC_NT ? nt : 0);
    const double o[3] = {a.ox, a.oy, a.oz};
    for (int v = blockIdx.x * MCL_NT + (int)threadIdx.x; v < nv; v += (int)gridDim.x * MCL_NT) {
        long long q[3];
        const bool ok = mesh_fix_q(a.xyz, (size_t)v, o, a.cell, q);
#pragma unroll
        for (int k = 0; k < 3; k++) a.qa[3 * (size_t)v + k] = ok ? q[k] : 0;
        a.vvalid[v] = ok ? 1 : 0;
        a.parent[v] = v;
        a.rep[v] = MCL_NOREP;
        a.tcnt[v] = 0;
        a.deg[v] = 0;
        a.cursor[v] = 0;
    }
}

__global__ __launch_bounds__(MCL_NT) void k_mcl_union(MeshCleanArgs a)
{
    __shared__ int s_sum[4];
    const int nv = a.meta[MC_NV], nt = a.meta[MC_NT], nbt = (nt + MCL_NT - 1) / MCL_NT;
    int mine = 0;
    for (int b = blockIdx.x; b < nbt; b += gridDim.x) {
        const int k = b * MCL_NT + (int)threadIdx.x;
        if (k >= nt) continue;
        const int i0 = a.tri[3 * (size_t)k], i1 = a.tri[3 * (size_t)k + 1], i2 = a.tri[3 * (size_t)k + 2];
        bool used = (unsigned)i0 < (unsigned)nv && (unsigned)i1 < (unsigned)nv && (unsigned)i2 < (unsigned)nv && i0 != i1 && i0 != i2 &&
                    i1 != i2;
        used = used && a.vvalid[i0] && a.vvalid[i1] && a.vvalid[i2];
        a.tused[k] = used ? 1 : 0;
        if (!used) continue;
        mine++;
        atomicAdd(a.deg + i0, 1);
        atomicAdd(a.deg + i1, 1);
        atomicAdd(a.deg + i2, 1);
        trk_hook(a.parent, i0, i1, [](int x) { return mcl_prio(x); });
        trk_hook(a.parent, i0, i2, [](int x) { return mcl_prio(x); });
    }
    const int nu = block_sum_i(mine, s_sum);
    if (threadIdx.x == 0 && nu) atomicAdd(&a.meta[MC_USED], nu);
}

__global__ __launch_bounds__(MCL_NT) void k_mcl_roots(MeshCleanArgs a)
{
    const int nv = a.meta[MC_NV];
    // into an array of its own: other threads' pointer jumping still stores (older) ancestors into parent[v] while this runs
    for (int v = blockIdx.x * MCL_NT + (int)threadIdx.x; v < nv; v += (int)gridDim.x * MCL_NT)
        a.root[v] = a.deg[v] > 0 ? trk_find(a.parent, v) : -1;
}

// the LDS table into the global sums: one add and one minimum per distinct root, one maximum for the workgroup
__device__ __forceinline__ void mcl_flush(const MeshCleanArgs &a, uint32_t *hkey, int *hcnt, int *hmin, int *s_ctl)
{
    __syncthreads();
    for (int i = threadIdx.x; i < MCL_SLOTS; i += MCL_NT) {
        const uint32_t r = hkey[i];
        if (r == MCL_EMPTY) continue;
        const int n = hcnt[i], old = atomicAdd(a.tcnt + r, n);
        atomicMin(a.rep + r, hmin[i]);
        atomicMax(&s_ctl[1], old + n);
        hkey[i] = MCL_EMPTY; hcnt[i] = 0; hmin[i] = MCL_NOREP;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        if (s_ctl[1] > 0) atomicMax(&a.meta[MC_BIG], s_ctl[1]);
        s_ctl[0] = 0;
        s_ctl[1] = 0;
    }
    __syncthreads();
}

__global__ __launch_bounds__(MCL_NT) void k_mcl_count(MeshCleanArgs a)
{
    __shared__ uint32_t hkey[MCL_SLOTS];
    __shared__ int hcnt[MCL_SLOTS], hmin[MCL_SLOTS], s_ctl[2];   // s_ctl: the slots in use, the largest sum of this flush
    const int nt = a.meta[MC_NT], nbt = (nt + MCL_NT - 1) / MCL_NT;
    for (int i = threadIdx.x; i < MCL_SLOTS; i += MCL_NT) { hkey[i] = MCL_EMPTY; hcnt[i] = 0; hmin[i] = MCL_NOREP; }
    if (threadIdx.x == 0) s_ctl[0] = s_ctl[1] = 0;
    __syncthreads();
    for (int b = blockIdx.x; b < nbt; b += gridDim.x) {   // uniform: every thread of the workgroup takes every pass
        const int in_use = s_ctl[0];
        __syncthreads();   // every thread has read it before the first insert of this pass moves it: the flush is uniform
        if (in_use > MCL_SLOTS - MCL_NT) mcl_flush(a, hkey, hcnt, hmin, s_ctl);   // this pass could fill the table
        const int k = b * MCL_NT + (int)threadIdx.x;
        if (k < nt && a.tused[k]) {
            const int i0 = a.tri[3 * (size_t)k], i1 = a.tri[3 * (size_t)k + 1], i2 = a.tri[3 * (size_t)k + 2];
            if (block_tally_add(hkey, hcnt, hmin, MCL_SLOTS, a.root[i0], min(i0, min(i1, i2)))) atomicAdd(&s_ctl[0], 1);
        }
        __syncthreads();   // s_ctl[0] is read at the head of the next pass
    }
    mcl_flush(a, hkey, hcnt, hmin, s_ctl);
}

// the component of root r is kept
__device__ __forceinline__ bool mcl_kept(const MeshCleanArgs &a, int r, int big)
{
    const int c = a.tcnt[r];
    return c >= a.min_tris && 1000ll * (long long)c >= (long long)a.min_frac_pm * (long long)big;
}

// index i as a vertex and as a triangle: kept or not, the row entries of the vertex
__device__ __forceinline__ void mcl_item(const MeshCleanArgs &a, int i, int nv, int nt, int big, int &vk, int &tk, int &rows, int &vroot)
{
    vk = tk = rows = 0;
    vroot = -1;
    if (i < nv) {
        vroot = a.root[i];
        if (vroot >= 0 && mcl_kept(a, vroot, big)) { vk = 1; rows = a.deg[i]; }
    }
    if (i < nt && a.tused[i]) tk = mcl_kept(a, a.root[a.tri[3 * (size_t)i]], big) ? 1 : 0;
}

__global__ __launch_bounds__(MCL_NT) void k_mcl_bsum(MeshCleanArgs a)
{
    __shared__ int s_sum[4];
    const int nv = a.meta[MC_NV], nt = a.meta[MC_NT], big = a.meta[MC_BIG], n = nv > nt ? nv : nt, nbn = (n + MCL_NT - 1) / MCL_NT;
    for (int b = blockIdx.x; b < nbn; b += gridDim.x) {
        const int i = b * MCL_NT + (int)threadIdx.x;
        int vk, tk, rows, r;
        mcl_item(a, i, nv, nt, big, vk, tk, rows, r);
        const int named = r >= 0 && a.rep[r] == i;   // the component's name stands here
        const int sv = block_sum_i(vk, s_sum), st = block_sum_i(tk, s_sum), sc = block_sum_i(named, s_sum),
                  sk = block_sum_i(named && vk, s_sum);
        // the rows of a block: at most 3 * 2^28 in all, below 2^32; summed as two halves that cannot carry into each other
        const int rl = block_sum_i(rows & 0xFFFF, s_sum), rh = block_sum_i(rows >> 16, s_sum);
        if (threadIdx.x == 0) {
            a.bsum[b] = mesh_pack_kept(sv, st);
            a.rsum[b] = (unsigned long long)(unsigned)rl + ((unsigned long long)(unsigned)rh << 16);
            if (sc) atomicAdd(&a.meta[MC_COMPS], sc);
            if (sk) atomicAdd(&a.meta[MC_KEPT], sk);
        }
    }
}

__global__ __launch_bounds__(MCL_NT) void k_mcl_scan(MeshCleanArgs a)
{
    __shared__ unsigned long long s_lds[MCL_NT / 64];
    const int nv = a.meta[MC_NV], nt = a.meta[MC_NT], n = nv > nt ? nv : nt, nbn = (n + MCL_NT - 1) / MCL_NT;
    const unsigned long long carry = block_scan_array<unsigned long long, MCL_NT>(a.bsum, a.boff, nbn, s_lds);
    block_scan_array<unsigned long long, MCL_NT>(a.rsum, a.rbase, nbn, s_lds);
    if (threadIdx.x == 0) {
        const int vo = mesh_kept_vertices(carry), to = mesh_kept_tris(carry);
        a.meta[MC_VOUT] = vo;
        a.meta[MC_TOUT] = to;
        if (vo > a.max_out_vertices || to > a.max_out_tris) atomicOr(a.status, (int)PGX_ST_MCL_CAP);
        a.report[0] = nv; a.report[1] = nt; a.report[2] = a.meta[MC_USED]; a.report[3] = a.meta[MC_COMPS];
        a.report[4] = a.meta[MC_KEPT]; a.report[5] = vo; a.report[6] = to; a.report[7] = a.meta[MC_BIG];
    }
}

__global__ __launch_bounds__(MCL_NT) void k_mcl_rank(MeshCleanArgs a)
{
    __shared__ unsigned long long s_lds[MCL_NT / 64];
    const int nv = a.meta[MC_NV], nt = a.meta[MC_NT], big = a.meta[MC_BIG], n = nv > nt ? nv : nt, nbn = (n + MCL_NT - 1) / MCL_NT;
    for (int b = blockIdx.x; b < nbn; b += gridDim.x) {
        const int i = b * MCL_NT + (int)threadIdx.x;
        int vk, tk, rows, r;
        mcl_item(a, i, nv, nt, big, vk, tk, rows, r);
        unsigned long long tot;
        const unsigned long long at = a.boff[b] + block_excl_scan<unsigned long long, MCL_NT>(mesh_pack_kept(vk, tk), s_lds, tot);
        const unsigned long long rat = a.rbase[b] + block_excl_scan<unsigned long long, MCL_NT>((unsigned long long)(unsigned)rows, s_lds, tot);
        if (i < nv) {
            const int nw = vk ? mesh_kept_vertices(at) : (r >= 0 ? -2 : -1);
            a.vnew[i] = nw;
            a.roff[i] = (int)rat;
            if (a.vertex_map) a.vertex_map[i] = nw;
            if (a.comp) a.comp[i] = r >= 0 ? a.rep[r] : -1;
        }
        if (i < nt) a.tnew[i] = tk ? mesh_kept_tris(at) : -1;
    }
}

__global__ __launch_bounds__(MCL_NT) void k_mcl_emit(MeshCleanArgs a)
{
    const int nv = a.meta[MC_NV], nt = a.meta[MC_NT], n = nv > nt ? nv : nt;
    for (int i = blockIdx.x * MCL_NT + (int)threadIdx.x; i < n; i += (int)gridDim.x * MCL_NT) {
        const int w = i < nv ? a.vnew[i] : -1;
        if (w >= 0 && w < a.max_out_vertices) {
            a.out_rgba8[w] = a.rgba8[i];
#pragma unroll
            for (int k = 0; k < 4; k++) a.out_info[4 * (size_t)w + k] = a.info[4 * (size_t)i + k];
            if (a.iters == 0) {
#pragma unroll
                for (int k = 0; k < 3; k++) {
                    a.out_xyz[3 * (size_t)w + k] = a.xyz[3 * (size_t)i + k];
                    a.out_normal[3 * (size_t)w + k] = a.normal[3 * (size_t)i + k];
                }
            }
        }
        const int t = i < nt ? a.tnew[i] : -1;
        if (t >= 0 && t < a.max_out_tris) {
#pragma unroll
            for (int k = 0; k < 3; k++) a.out_tri[3 * (size_t)t + k] = a.vnew[a.tri[3 * (size_t)i + k]];
        }
    }
}

__global__ __launch_bounds__(MCL_NT) void k_mcl_rows(MeshCleanArgs a)
{
    const int nt = a.meta[MC_NT];
    for (int k = blockIdx.x * MCL_NT + (int)threadIdx.x; k < nt; k += (int)gridDim.x * MCL_NT) {
        if (a.tnew[k] < 0) continue;
#pragma unroll
        for (int j = 0; j < 3; j++) {
            const int v = a.tri[3 * (size_t)k + j];
            a.rows[(size_t)a.roff[v] + (size_t)atomicAdd(a.cursor + v, 1)] = k;
        }
    }
}

// the sum of x over the 64 lanes of the wave, in every lane (integers: any order gives the same bits)
__device__ __forceinline__ unsigned long long mcl_wave_sum(unsigned long long x)
{
#pragma unroll
    for (int m = 1; m < 64; m <<= 1) x += __shfl_xor(x, m, 64);
    return x;
}

// entries j0, j0 + step, ... below d of a row: the sums of the three positions of their triangles
__device__ __forceinline__ void mcl_row_positions(const MeshCleanArgs &a, const long long *src, const int32_t *row, int j0, int d, int step,
                                                  unsigned long long (&s)[3])
{
    for (int j = j0; j < d; j += step) {
        const int32_t *t = a.tri + 3 * (size_t)row[j];
#pragma unroll
        for (int c = 0; c < 3; c++) {
            const long long *q = src + 3 * (size_t)t[c];
            s[0] += (unsigned long long)q[0]; s[1] += (unsigned long long)q[1]; s[2] += (unsigned long long)q[2];
        }
    }
}

// ... and the sums of their triangles' m of rule 4
__device__ __forceinline__ void mcl_row_normals(const MeshCleanArgs &a, const int32_t *row, int j0, int d, int step, unsigned long long (&s)[3])
{
    for (int j = j0; j < d; j += step) {
        const unsigned long long m = a.tnrm[row[j]];
        if (m == MCL_NONRM) continue;
#pragma unroll
        for (int c = 0; c < 3; c++) s[c] += (unsigned long long)(long long)mesh_unpack_m(m, c);
    }
}

// The row sums of the workgroup's 256 vertices (d entries from ro; d = 0: none): a thread sums its own short row; the long rows
// of a wave are taken one after the other by all its lanes.  Every thread of the workgroup calls this.
template <bool NORMALS>
__device__ __forceinline__ void mcl_row_sums(const MeshCleanArgs &a, const long long *src, int ro, int d, unsigned long long (&s)[3])
{
    const int lane = threadIdx.x & 63;
    s[0] = s[1] = s[2] = 0;
    if (d <= MCL_LONG_ROW) {
        if (NORMALS) mcl_row_normals(a, a.rows + (size_t)ro, 0, d, 1, s);
        else mcl_row_positions(a, src, a.rows + (size_t)ro, 0, d, 1, s);
    }
    unsigned long long longs = __ballot(d > MCL_LONG_ROW);
    while (longs) {   // uniform over the wave
        const int l = __ffsll(longs) - 1;
        longs &= longs - 1;
        const int dl = __shfl(d, l, 64), rl = __shfl(ro, l, 64);
        unsigned long long p[3] = {0, 0, 0};
        if (NORMALS) mcl_row_normals(a, a.rows + (size_t)rl, lane, dl, 64, p);
        else mcl_row_positions(a, src, a.rows + (size_t)rl, lane, dl, 64, p);
#pragma unroll
        for (int c = 0; c < 3; c++) {
            p[c] = mcl_wave_sum(p[c]);
            if (lane == l) s[c] = p[c];
        }
    }
}

// One half-step of rule 3 with factor f from src into dst.  Over a row, the sum of (q[o1] - q[v]) + (q[o2] - q[v]) is the sum of
// the triangles' three positions less 3 d q[v]: the same bits in two's complement, with no search for v in the triangle.
__global__ __launch_bounds__(MCL_NT) void k_mcl_smooth(MeshCleanArgs a, double f, const long long *src, long long *dst)
{
    const int nv = a.meta[MC_NV], nbv = (nv + MCL_NT - 1) / MCL_NT;
    for (int b = blockIdx.x; b < nbv; b += gridDim.x) {
        const int v = b * MCL_NT + (int)threadIdx.x;
        const bool kept = v < nv && a.vnew[v] >= 0;
        const int d = kept ? a.deg[v] : 0;
        unsigned long long s[3];
        mcl_row_sums<false>(a, src, kept ? a.roff[v] : 0, d, s);
        if (!kept) continue;
        const unsigned long long d3 = 3ull * (unsigned long long)d;
        const double den = (double)(2 * (long long)d);
#pragma unroll
        for (int c = 0; c < 3; c++) {
            const long long q = src[3 * (size_t)v + c], D = (long long)(s[c] - d3 * (unsigned long long)q);
            double inc = floor((f * (double)D) / den + 0.5);
            inc = inc > MCL_STEP_MAX ? MCL_STEP_MAX : (inc < -MCL_STEP_MAX ? -MCL_STEP_MAX : inc);
            dst[3 * (size_t)v + c] = (long long)((unsigned long long)q + (unsigned long long)(long long)inc);
        }
    }
}

__global__ __launch_bounds__(MCL_NT) void k_mcl_tnormal(MeshCleanArgs a, const long long *q)
{
    const int nt = a.meta[MC_NT];
    for (int k = blockIdx.x * MCL_NT + (int)threadIdx.x; k < nt; k += (int)gridDim.x * MCL_NT) {
        if (a.tnew[k] < 0) continue;
        const long long *qa = q + 3 * (size_t)a.tri[3 * (size_t)k], *qb = q + 3 * (size_t)a.tri[3 * (size_t)k + 1],
                        *qc = q + 3 * (size_t)a.tri[3 * (size_t)k + 2];
        int m[3];
        a.tnrm[k] = mesh_tri_m(qa, qb, qc, 32767.0, m) ? mesh_pack_m(m) : MCL_NONRM;   // rule 4
    }
}

__global__ __launch_bounds__(MCL_NT) void k_mcl_finish(MeshCleanArgs a, const long long *q)
{
    const int nv = a.meta[MC_NV], nbv = (nv + MCL_NT - 1) / MCL_NT;
    const double o[3] = {a.ox, a.oy, a.oz};
    for (int b = blockIdx.x; b < nbv; b += gridDim.x) {
        const int v = b * MCL_NT + (int)threadIdx.x, w = v < nv ? a.vnew[v] : -1;
        const bool out = w >= 0 && w < a.max_out_vertices;
        unsigned long long s[3];
        mcl_row_sums<true>(a, nullptr, out ? a.roff[v] : 0, out ? a.deg[v] : 0, s);
        if (!out) continue;
        mesh_unit_normal(a.out_normal, w, s[0], s[1], s[2]);
#pragma unroll
        for (int c = 0; c < 3; c++) a.out_xyz[3 * (size_t)w + c] = mesh_q_to_world(o[c], q[3 * (size_t)v + c], a.cell);
    }
}

// the workspace, described once: the arguments' workspace pointers (none valid for ws = nullptr) and the bytes
size_t mcl_carve(MeshCleanArgs &a, void *ws)
{
    WsCarver w(ws);
    const size_t nv = (size_t)a.max_vertices, nt = (size_t)a.max_tris, n = nv > nt ? nv : nt;
    a.nb = n > 0 ? (int)((n + MCL_NT - 1) / MCL_NT) : 1;
    a.parent = w.take<int32_t>(nv * 4);
    a.root = w.take<int32_t>(nv * 4);
    a.rep = w.take<int32_t>(nv * 4);
    a.tcnt = w.take<int32_t>(nv * 4);
    a.deg = w.take<int32_t>(nv * 4);
    a.vnew = w.take<int32_t>(nv * 4);
    a.roff = w.take<int32_t>(nv * 4);
    a.cursor = w.take<int32_t>(nv * 4);
    a.qa = w.take<long long>(nv * 24);
    a.qb = w.take<long long>(nv * 24);
    a.vvalid = w.take<unsigned char>(nv);
    a.tused = w.take<unsigned char>(nt);
    a.tnew = w.take<int32_t>(nt * 4);
    a.rows = w.take<int32_t>(nt * 12);
    a.tnrm = w.take<unsigned long long>(nt * 8);
    a.bsum = w.take<unsigned long long>((size_t)a.nb * 8);
    a.boff = w.take<unsigned long long>((size_t)a.nb * 8);
    a.rsum = w.take<unsigned long long>((size_t)a.nb * 8);
    a.rbase = w.take<unsigned long long>((size_t)a.nb * 8);
    a.meta = w.take<int32_t>(8 * 4);
    return w.total();
}

} // namespace

size_t pgx_mesh_clean_ws_bytes(const MeshCleanArgs &a)
{
    MeshCleanArgs b = a;
    return mcl_carve(b, nullptr);
}

void pgx_launch_mesh_clean(pgx_ctx *ctx, hipStream_t s, MeshCleanArgs a, void *ws)
{
    mcl_carve(a, ws);
    const unsigned bv = (unsigned)(a.max_vertices > 0 ? (a.max_vertices + MCL_NT - 1) / MCL_NT : 1),
                   bt = (unsigned)(a.max_tris > 0 ? (a.max_tris + MCL_NT - 1) / MCL_NT : 1);
    const unsigned vgrid = bv < (unsigned)MCL_GRID_MAX ? bv : (unsigned)MCL_GRID_MAX, tgrid = bt < (unsigned)MCL_GRID_MAX ? bt : (unsigned)MCL_GRID_MAX,
                   ngrid = (unsigned)(a.nb < MCL_GRID_MAX ? a.nb : MCL_GRID_MAX), ugrid = bt < (unsigned)MCL_UNION_GRID ? bt : (unsigned)MCL_UNION_GRID;
    {
        ProfScope ps(ctx, "mclean_init", s);
        hipLaunchKernelGGL(k_mcl_init, dim3(vgrid), dim3(MCL_NT), 0, s, a);
    }
    {
        ProfScope ps(ctx, "mclean_union", s);
        hipLaunchKernelGGL(k_mcl_union, dim3(ugrid), dim3(MCL_NT), 0, s, a);
    }
    {
        ProfScope ps(ctx, "mclean_count", s);
        hipLaunchKernelGGL(k_mcl_roots, dim3(vgrid), dim3(MCL_NT), 0, s, a);
        hipLaunchKernelGGL(k_mcl_count, dim3(ugrid), dim3(MCL_NT), 0, s, a);
    }
    {
        ProfScope ps(ctx, "mclean_rank", s);
        hipLaunchKernelGGL(k_mcl_bsum, dim3(ngrid), dim3(MCL_NT), 0, s, a);
        hipLaunchKernelGGL(k_mcl_scan, dim3(1), dim3(MCL_NT), 0, s, a);
        hipLaunchKernelGGL(k_mcl_rank, dim3(ngrid), dim3(MCL_NT), 0, s, a);
    }
    {
        ProfScope ps(ctx, "mclean_emit", s);
        hipLaunchKernelGGL(k_mcl_emit, dim3(ngrid), dim3(MCL_NT), 0, s, a);
    }
    if (a.iters == 0) return;
    {
        ProfScope ps(ctx, "mclean_rows", s);
        hipLaunchKernelGGL(k_mcl_rows, dim3(tgrid), dim3(MCL_NT), 0, s, a);
    }
    const long long *src = a.qa;
    long long *dst = a.qb;
    {
        ProfScope ps(ctx, "mclean_smooth", s);
        for (int it = 0; it < a.iters; it++)
            for (int half = 0; half < (a.mu == 0.0 ? 1 : 2); half++) {
                hipLaunchKernelGGL(k_mcl_smooth, dim3(vgrid), dim3(MCL_NT), 0, s, a, half ? a.mu : a.lambda, src, dst);
                long long *t = const_cast<long long *>(src);
                src = dst;
                dst = t;
            }
    }
    {
        ProfScope ps(ctx, "mclean_normals", s);
        hipLaunchKernelGGL(k_mcl_tnormal, dim3(tgrid), dim3(MCL_NT), 0, s, a, src);
        hipLaunchKernelGGL(k_mcl_finish, dim3(vgrid), dim3(MCL_NT), 0, s, a, src);
    }
}
