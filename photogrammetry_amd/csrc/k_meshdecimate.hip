// k_meshdecimate.hip -- a mesh in pgx_mesh_dev's layout decimated where it lies by adaptive vertex clustering: the vertices of a
// grid block of 2^l cells merge into one where the triangle normals round the block agree, up to level lmax, and stay apart where
// they do not (pgx_mesh_decimate_dev; include/pgx.h states the rule operation by operation).  Not in the C# reference.
//
// Kernels on the caller's stream, none of which needs a count on the host:
//   k_mdc_plan     one workgroup: nv and nt from d_counts, the sizes of the tables (powers of two >= 2 nv and 2 nt), zeroes
//   k_mdc_init     per vertex the valid test and the fixed-point position; the tables cleared (only the part this call uses)
//   k_mdc_tris     the incidence pass, one thread per triangle: the used test, m of rule 2, the members, and (lmax > lmin) N and S of
//                  the level lmin + 1 blocks of its three corners.  Consecutive triangles of a surface-nets list lie in the same
//                  few blocks: the sums are taken in an LDS table per workgroup that lives across its grid-stride passes, one
//                  corner at a time, flushed when the next corner could fill it and at the end: four global adds per distinct
//                  block and flush, not per incidence
//   k_mdc_vlevel   (per level l) one thread per member still at level l - 1: the flat test of its level-l block
//   k_mdc_up       (per level l < lmax) one thread per entry of level l's table: added into its parent of level l + 1, then cleared
//   k_mdc_clusters one thread per member: its cluster (the key of (L, block)), the minimum for the name and the integer sums, in an
//                  LDS table per workgroup flushed as k_mdc_tris' is: one claim, one atomicMin and eight adds per distinct cluster
//   k_mdc_vslot    one thread per member: the entry of its cluster
//   k_mdc_map      one thread per used triangle: its three clusters, rotated so that the smallest name leads
//   k_mdc_claim    one thread per non-degenerate triangle: the table of triples, claimed by a 32-bit CAS with the triangle's index;
//                  an entry whose owner has the same triple takes the smaller index (atomicMin)
//   k_mdc_mark     one thread per kept triangle (the owner of its entry): its three clusters are in the output
//   k_mdc_bsum / k_mdc_scan / k_mdc_rank   the output vertices (at their names) and the kept triangles numbered in index order
//   k_mdc_emit     vertex_map and level; at a cluster's name Q, the position, the colour, info; the kept triangles' new indices
//   k_mdc_tnormal  one thread per kept triangle: m of rule 7 on Q added to its three clusters; the flipped ones counted
//   k_mdc_finish   at the name of an output cluster: the normal
// Every probe loop is bounded by one round of its table.  DESIGN.md section 31.
#include "pgx_stage_args.h"
#include "pgx_cloudkey.h"
#include "pgx_meshlist.h"   // what every stage does to a mesh list: shared with k_meshclean.hip

namespace {

constexpr int MDC_NT = 256;             // threads per workgroup of every kernel here; the block of the scans
constexpr int MDC_GRID_MAX = 1024;      // workgroups of every kernel, grid-stride beyond
constexpr int MDC_LG_SLOTS = 10;        // lg of MDC_SLOTS
constexpr int MDC_SLOTS = 1024;         // LDS aggregation table of k_mdc_tris
constexpr int MDC_FLUSH_AT = 256;       // ... flushed before a corner when more entries are in use (<= MDC_SLOTS - MDC_NT): at most half full
constexpr int MDC_LG_TMIN = 9;          // the smallest table has 1 << MDC_LG_TMIN entries
constexpr unsigned long long MDC_EMPTY = ~0ull;                    // no key: a key never has all of bits 60 .. 62 set with bit 63
constexpr unsigned long long MDC_HASH_MUL = 0x9E3779B97F4A7C15ull; // mdc_hash: the top lg bits of key * this (mod 2^64)
constexpr unsigned long long MDC_TRI_MUL1 = 0xD6E8FEB86659FD93ull; // mdc_tri_hash: the second and third cluster's factors
constexpr unsigned long long MDC_TRI_MUL2 = 0xC2B2AE3D27D4EB4Full;
constexpr int MDC_NONE = 0x7FFFFFFF;
constexpr long long MDC_Q_MAX = (1ll << 36) - 1;                   // the largest fixed-point position: the last cell's far end
enum { MD_NV = 0, MD_NT, MD_LGV, MD_LGT, MD_USED, MD_CLUSTERS, MD_NONDEG, MD_VOUT, MD_TOUT };   // meta

__device__ __forceinline__ unsigned mdc_hash(unsigned long long key, int lg) { return (unsigned)((key * MDC_HASH_MUL) >> (64 - lg)); }

__device__ __forceinline__ unsigned mdc_tri_hash(int c0, int c1, int c2, int lg)
{
    const unsigned long long x = ((unsigned long long)(unsigned)c0 * MDC_HASH_MUL + (unsigned long long)(unsigned)c1 * MDC_TRI_MUL1) +
                                 (unsigned long long)(unsigned)c2 * MDC_TRI_MUL2;
    return (unsigned)(x >> (64 - lg));
}

// The key of block (b0, b1, b2) of level l.  Level 0: the cloud's 63-bit key of the cell.  Above: a block coordinate has 20 bits
// (b + 2^19), the level stands in bits 60 .. 62 and bit 63 is set, so no two levels share a key and none is MDC_EMPTY (l <= 6).
__device__ __forceinline__ unsigned long long mdc_key(int l, long long b0, long long b1, long long b2)
{
    if (l == 0) return cld_key_of((int)b0, (int)b1, (int)b2);
    return 1ull << 63 | (unsigned long long)l << 60 | (unsigned long long)(b0 + 524288) << 40 | (unsigned long long)(b1 + 524288) << 20 |
           (unsigned long long)(b2 + 524288);
}

// ... of the block of level l that holds position q
__device__ __forceinline__ unsigned long long mdc_key_at(int l, const long long *q) { return mdc_key(l, q[0] >> (16 + l), q[1] >> (16 + l), q[2] >> (16 + l)); }

// ... of the parent of a block of level l >= 1
__device__ __forceinline__ unsigned long long mdc_parent(unsigned long long key)
{
    const int l = (int)((key >> 60) & 7);
    const long long b0 = (long long)((key >> 40) & 0xFFFFF) - 524288, b1 = (long long)((key >> 20) & 0xFFFFF) - 524288,
                    b2 = (long long)(key & 0xFFFFF) - 524288;
    return mdc_key(l + 1, b0 >> 1, b1 >> 1, b2 >> 1);
}

// the entry of `key` in a table of 1 << lg keys, claimed if it has none; -1: the table is full (it cannot be: twice the keys)
__device__ __forceinline__ int mdc_insert(unsigned long long *keys, int lg, unsigned long long key, bool &fresh)
{
    const unsigned mask = (1u << lg) - 1u;
    unsigned h = mdc_hash(key, lg);
    fresh = false;
    for (unsigned i = 0; i <= mask; i++) {
        unsigned long long prev = keys[h];
        if (prev == MDC_EMPTY) {
            prev = atomicCAS(&keys[h], MDC_EMPTY, key);
            fresh = prev == MDC_EMPTY;
        }
        if (prev == MDC_EMPTY || prev == key) return (int)h;
        h = (h + 1) & mask;
    }
    return -1;
}

__device__ __forceinline__ int mdc_find(const unsigned long long *keys, int lg, unsigned long long key)
{
    const unsigned mask = (1u << lg) - 1u;
    unsigned h = mdc_hash(key, lg);
    for (unsigned i = 0; i <= mask; i++) {
        const unsigned long long k = keys[h];
        if (k == key) return (int)h;
        if (k == MDC_EMPTY) return -1;
        h = (h + 1) & mask;
    }
    return -1;
}

// lg of the table for n vertices or triangles: the power of two >= 2 n, at least 1 << MDC_LG_TMIN (the host sizes the workspace by
// the capacity, the device clears and probes what the count needs)
__host__ __device__ inline int mdc_lg(int n)
{
    int lg = MDC_LG_TMIN;
    while (lg < 30 && (1ll << lg) < 2ll * (long long)n) lg++;
    return lg;
}

__global__ __launch_bounds__(MDC_NT) void k_mdc_plan(MeshDecimateArgs a)
{
    if (threadIdx.x >= 16) return;
    int nv, nt;
    mesh_counts(a.counts, a.max_vertices, a.max_tris, nv, nt);
    const int k = threadIdx.x;
    a.meta[k] = k == MD_NV ? nv : (k == MD_NT ? nt : (k == MD_LGV ? mdc_lg(nv) : (k == MD_LGT ? mdc_lg(nt) : 0)));
}

__global__ __launch_bounds__(MDC_NT) void k_mdc_init(MeshDecimateArgs a)
{
    const int nv = a.meta[MD_NV];
    const size_t TV = (size_t)1 << a.meta[MD_LGV], TT = (size_t)1 << a.meta[MD_LGT], stride = (size_t)gridDim.x * MDC_NT,
                 at = (size_t)blockIdx.x * MDC_NT + threadIdx.x;
    const double o[3] = {a.ox, a.oy, a.oz};
    for (size_t v = at; v < (size_t)nv; v += stride) {
        long long q[3];
        const bool ok = mesh_fix_q(a.xyz, v, o, a.cell, q);
#pragma unroll
        for (int k = 0; k < 3; k++)   // t just below 2^20 rounds to 2^36, one past the last cell: rule 1 here clamps it
            a.q[3 * v + k] = ok ? (q[k] > MDC_Q_MAX ? MDC_Q_MAX : q[k]) : 0;
        a.member[v] = ok ? 0 : 2;   // 2: not valid; k_mdc_tris sets 1
        a.lev[v] = (unsigned char)a.lmin;
        a.vslot[v] = -1;
    }
    for (size_t i = at; i < TV; i += stride) {
        a.fkey[0][i] = MDC_EMPTY; a.fkey[1][i] = MDC_EMPTY; a.ckey[i] = MDC_EMPTY;
        a.cname[i] = MDC_NONE; a.cn[i] = 0; a.cnew[i] = -1; a.cused[i] = 0;
#pragma unroll
        for (int k = 0; k < 4; k++) { a.fsum[0][4 * i + k] = 0; a.fsum[1][4 * i + k] = 0; a.csc[4 * i + k] = 0; }
#pragma unroll
        for (int k = 0; k < 3; k++) a.cs[3 * i + k] = 0;
    }
    for (size_t i = at; i < TT; i += stride) a.towner[i] = -1;
}

// the LDS table into the level table: one claim and four adds per distinct block
__device__ __forceinline__ void mdc_flush(const MeshDecimateArgs &a, int lgv, unsigned long long *hkey, unsigned long long *hsum, int *s_ctl)
{
    __syncthreads();
    for (int i = threadIdx.x; i < MDC_SLOTS; i += MDC_NT) {
        const unsigned long long key = hkey[i];
        if (key == MDC_EMPTY) continue;
        bool fresh;
        const int e = mdc_insert(a.fkey[0], lgv, key, fresh);
        if (e < 0) atomicOr(a.status, (int)PGX_ST_INTERNAL);
#pragma unroll
        for (int k = 0; k < 4; k++) {
            if (e >= 0 && hsum[4 * i + k]) atomicAdd(&a.fsum[0][4 * (size_t)e + k], hsum[4 * i + k]);
            hsum[4 * i + k] = 0;
        }
        hkey[i] = MDC_EMPTY;
    }
    __syncthreads();
    if (threadIdx.x == 0) s_ctl[0] = 0;
    __syncthreads();
}

// block `key` counted cnt times more with the triangle's m, in the LDS table; true when it claimed a new entry
__device__ __forceinline__ bool mdc_tally(unsigned long long *hkey, unsigned long long *hsum, unsigned long long key, int cnt, const int (&m)[3])
{
    unsigned h = mdc_hash(key, MDC_LG_SLOTS);
    for (int i = 0; i < MDC_SLOTS; i++) {   // the table is flushed before it can fill: the loop ends at an entry
        const unsigned long long old = atomicCAS(&hkey[h], MDC_EMPTY, key);
        if (old == MDC_EMPTY || old == key) {
#pragma unroll
            for (int k = 0; k < 3; k++)
                if (m[k]) atomicAdd(&hsum[4 * h + k], (unsigned long long)((long long)m[k] * cnt));
            atomicAdd(&hsum[4 * h + 3], (unsigned long long)cnt);
            return old == MDC_EMPTY;
        }
        h = (h + 1) & (MDC_SLOTS - 1);
    }
    return false;
}

__global__ __launch_bounds__(MDC_NT) void k_mdc_tris(MeshDecimateArgs a)
{
    __shared__ unsigned long long hkey[MDC_SLOTS], hsum[4 * MDC_SLOTS];
    __shared__ int s_ctl[1], s_sum[4];
    const int nv = a.meta[MD_NV], nt = a.meta[MD_NT], lgv = a.meta[MD_LGV], nbt = (nt + MDC_NT - 1) / MDC_NT;
    const bool levels = a.lmax > a.lmin;
    for (int i = threadIdx.x; i < MDC_SLOTS; i += MDC_NT) {
        hkey[i] = MDC_EMPTY;
#pragma unroll
        for (int k = 0; k < 4; k++) hsum[4 * i + k] = 0;
    }
    if (threadIdx.x == 0) s_ctl[0] = 0;
    __syncthreads();
    int mine = 0;
    for (int b = blockIdx.x; b < nbt; b += gridDim.x) {   // uniform: every thread of the workgroup takes every pass
        const int k = b * MDC_NT + (int)threadIdx.x;
        bool used = false;
        int m[3] = {0, 0, 0}, cnt[3] = {0, 0, 0};
        unsigned long long key[3] = {0, 0, 0};
        if (k < nt) {
            const int i0 = a.tri[3 * (size_t)k], i1 = a.tri[3 * (size_t)k + 1], i2 = a.tri[3 * (size_t)k + 2];
            used = (unsigned)i0 < (unsigned)nv && (unsigned)i1 < (unsigned)nv && (unsigned)i2 < (unsigned)nv && i0 != i1 && i0 != i2 && i1 != i2;
            used = used && a.member[i0] != 2 && a.member[i1] != 2 && a.member[i2] != 2;
            a.trot[3 * (size_t)k] = used ? 0 : -1;   // k_mdc_map reads the used test here
            if (used) {
                const long long *q0 = a.q + 3 * (size_t)i0, *q1 = a.q + 3 * (size_t)i1, *q2 = a.q + 3 * (size_t)i2;
                mesh_tri_m(q0, q1, q2, 1024.0, m);   // rule 2
                a.tm[k] = mesh_pack_m(m);
                a.member[i0] = 1; a.member[i1] = 1; a.member[i2] = 1;   // the same byte from every writer
                mine++;
                if (levels) {   // the distinct blocks of the three corners, each with its number of corners
                    key[0] = mdc_key_at(a.lmin + 1, q0); key[1] = mdc_key_at(a.lmin + 1, q1); key[2] = mdc_key_at(a.lmin + 1, q2);
                    cnt[0] = 1 + (key[1] == key[0]) + (key[2] == key[0]);
                    cnt[1] = key[1] == key[0] ? 0 : 1 + (key[2] == key[1]);
                    cnt[2] = key[2] == key[0] || key[2] == key[1] ? 0 : 1;
                }
            }
        }
        if (!levels) continue;   // uniform
#pragma unroll
        for (int j = 0; j < 3; j++) {
            const int in_use = s_ctl[0];
            __syncthreads();   // every thread has read it before the first insert of this corner moves it: the flush is uniform
            if (in_use > MDC_FLUSH_AT) mdc_flush(a, lgv, hkey, hsum, s_ctl);   // this corner could fill the table
            if (cnt[j] && mdc_tally(hkey, hsum, key[j], cnt[j], m)) atomicAdd(&s_ctl[0], 1);
            __syncthreads();   // s_ctl[0] is read at the head of the next corner
        }
    }
    if (levels) mdc_flush(a, lgv, hkey, hsum, s_ctl);
    const int nu = block_sum_i(mine, s_sum);
    if (threadIdx.x == 0 && nu) atomicAdd(&a.meta[MD_USED], nu);
}

// level l's table is fkey / fsum [t]
__global__ __launch_bounds__(MDC_NT) void k_mdc_vlevel(MeshDecimateArgs a, int l, int t)
{
    const int nv = a.meta[MD_NV], lgv = a.meta[MD_LGV];
    const double fq2 = (double)(a.flat_q * a.flat_q);
    for (int v = blockIdx.x * MDC_NT + (int)threadIdx.x; v < nv; v += (int)gridDim.x * MDC_NT) {
        if (a.member[v] != 1 || a.lev[v] != l - 1) continue;
        const int e = mdc_find(a.fkey[t], lgv, mdc_key_at(l, a.q + 3 * (size_t)v));
        if (e < 0) continue;   // a member's block has an entry
        const unsigned long long *f = a.fsum[t] + 4 * (size_t)e;
        const unsigned long long S2 = (f[0] * f[0] + f[1] * f[1]) + f[2] * f[2];   // int64, wrapping
        const double N = (double)(long long)f[3];
        if ((double)(long long)S2 >= fq2 * (N * N)) a.lev[v] = (unsigned char)l;
    }
}

// level l's table [t] into level l + 1's [1 - t], and [t] cleared for level l + 2
__global__ __launch_bounds__(MDC_NT) void k_mdc_up(MeshDecimateArgs a, int t)
{
    const int lgv = a.meta[MD_LGV];
    const size_t TV = (size_t)1 << lgv;
    for (size_t i = (size_t)blockIdx.x * MDC_NT + threadIdx.x; i < TV; i += (size_t)gridDim.x * MDC_NT) {
        const unsigned long long key = a.fkey[t][i];
        if (key == MDC_EMPTY) continue;
        bool fresh;
        const int e = mdc_insert(a.fkey[1 - t], lgv, mdc_parent(key), fresh);
        if (e < 0) atomicOr(a.status, (int)PGX_ST_INTERNAL);
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const unsigned long long x = a.fsum[t][4 * i + k];
            if (e >= 0 && x) atomicAdd(&a.fsum[1 - t][4 * (size_t)e + k], x);
            a.fsum[t][4 * i + k] = 0;
        }
        a.fkey[t][i] = MDC_EMPTY;
    }
}

// the LDS table of k_mdc_clusters into the cluster table: one claim, one minimum and eight adds per distinct cluster; the entries
// this thread claimed are counted into fresh
__device__ __forceinline__ void mdc_cflush(const MeshDecimateArgs &a, int lgv, unsigned long long *hkey, unsigned long long *hs, int *hmin, int *hn,
                                           unsigned *hc, int *s_ctl, int &fresh)
{
    __syncthreads();
    for (int i = threadIdx.x; i < MDC_SLOTS; i += MDC_NT) {
        const unsigned long long key = hkey[i];
        if (key == MDC_EMPTY) continue;
        bool fr;
        const int e = mdc_insert(a.ckey, lgv, key, fr);
        if (e < 0) atomicOr(a.status, (int)PGX_ST_INTERNAL);
        else {
            fresh += fr ? 1 : 0;
            atomicMin(&a.cname[e], hmin[i]);
            atomicAdd(&a.cn[e], hn[i]);
#pragma unroll
            for (int k = 0; k < 3; k++) atomicAdd(&a.cs[3 * (size_t)e + k], hs[3 * i + k]);
#pragma unroll
            for (int k = 0; k < 4; k++) atomicAdd(&a.csc[4 * (size_t)e + k], (unsigned long long)hc[4 * i + k]);
        }
        hkey[i] = MDC_EMPTY; hmin[i] = MDC_NONE; hn[i] = 0;
#pragma unroll
        for (int k = 0; k < 3; k++) hs[3 * i + k] = 0;
#pragma unroll
        for (int k = 0; k < 4; k++) hc[4 * i + k] = 0;
    }
    __syncthreads();
    if (threadIdx.x == 0) s_ctl[0] = 0;
    __syncthreads();
}

// On a flat wall a few hundred clusters take every vertex: a global atomic per member and sum serialises on their entries (2.7 ms
// for 2.8 M vertices).  The sums go through an LDS table per workgroup as k_mdc_tris' do: a workgroup's 256 consecutive vertices
// lie in few clusters.  A colour sum in LDS has 32 bits: a workgroup of the capped grid takes at most 2^28 / 1024 vertices, 255 each.
__global__ __launch_bounds__(MDC_NT) void k_mdc_clusters(MeshDecimateArgs a)
{
    __shared__ unsigned long long hkey[MDC_SLOTS], hs[3 * MDC_SLOTS];
    __shared__ int hmin[MDC_SLOTS], hn[MDC_SLOTS], s_ctl[1], s_sum[4];
    __shared__ unsigned hc[4 * MDC_SLOTS];
    const int nv = a.meta[MD_NV], lgv = a.meta[MD_LGV], nbv = (nv + MDC_NT - 1) / MDC_NT;
    for (int i = threadIdx.x; i < MDC_SLOTS; i += MDC_NT) {
        hkey[i] = MDC_EMPTY; hmin[i] = MDC_NONE; hn[i] = 0;
#pragma unroll
        for (int k = 0; k < 3; k++) hs[3 * i + k] = 0;
#pragma unroll
        for (int k = 0; k < 4; k++) hc[4 * i + k] = 0;
    }
    if (threadIdx.x == 0) s_ctl[0] = 0;
    __syncthreads();
    int fresh = 0;
    for (int b = blockIdx.x; b < nbv; b += gridDim.x) {   // uniform: every thread of the workgroup takes every pass
        const int in_use = s_ctl[0];
        __syncthreads();   // every thread has read it before the first insert of this pass moves it: the flush is uniform
        if (in_use > MDC_FLUSH_AT) mdc_cflush(a, lgv, hkey, hs, hmin, hn, hc, s_ctl, fresh);   // this pass could fill the table
        const int v = b * MDC_NT + (int)threadIdx.x;
        if (v < nv && a.member[v] == 1) {
            const int L = a.lev[v];
            const long long *q = a.q + 3 * (size_t)v;
            const unsigned long long key = mdc_key_at(L, q);
            const long long low = (1ll << (16 + L)) - 1;
            const uint32_t c = a.rgba8[v];
            unsigned h = mdc_hash(key, MDC_LG_SLOTS);
            for (int i = 0; i < MDC_SLOTS; i++) {   // the table is flushed before it can fill: the loop ends at an entry
                const unsigned long long old = atomicCAS(&hkey[h], MDC_EMPTY, key);
                if (old == MDC_EMPTY || old == key) {
                    atomicMin(&hmin[h], v);
                    atomicAdd(&hn[h], 1);
#pragma unroll
                    for (int k = 0; k < 3; k++) atomicAdd(&hs[3 * h + k], (unsigned long long)(q[k] & low));   // q - org: the low 16 + L bits
#pragma unroll
                    for (int k = 0; k < 4; k++) atomicAdd(&hc[4 * h + k], (c >> (8 * k)) & 0xFFu);
                    if (old == MDC_EMPTY) atomicAdd(&s_ctl[0], 1);
                    break;
                }
                h = (h + 1) & (MDC_SLOTS - 1);
            }
        }
        __syncthreads();   // s_ctl[0] is read at the head of the next pass
    }
    mdc_cflush(a, lgv, hkey, hs, hmin, hn, hc, s_ctl, fresh);
    const int nc = block_sum_i(fresh, s_sum);
    if (threadIdx.x == 0 && nc) atomicAdd(&a.meta[MD_CLUSTERS], nc);
}

// the entry of every member's cluster, once the table is complete
__global__ __launch_bounds__(MDC_NT) void k_mdc_vslot(MeshDecimateArgs a)
{
    const int nv = a.meta[MD_NV], lgv = a.meta[MD_LGV];
    for (int v = blockIdx.x * MDC_NT + (int)threadIdx.x; v < nv; v += (int)gridDim.x * MDC_NT)
        if (a.member[v] == 1) a.vslot[v] = mdc_find(a.ckey, lgv, mdc_key_at(a.lev[v], a.q + 3 * (size_t)v));
}

__global__ __launch_bounds__(MDC_NT) void k_mdc_map(MeshDecimateArgs a)
{
    __shared__ int s_sum[4];
    const int nt = a.meta[MD_NT], nbt = (nt + MDC_NT - 1) / MDC_NT;
    int mine = 0;
    for (int b = blockIdx.x; b < nbt; b += gridDim.x) {
        const int k = b * MDC_NT + (int)threadIdx.x;
        if (k >= nt || a.trot[3 * (size_t)k] < 0) continue;
        const int c0 = a.vslot[a.tri[3 * (size_t)k]], c1 = a.vslot[a.tri[3 * (size_t)k + 1]], c2 = a.vslot[a.tri[3 * (size_t)k + 2]];
        if (c0 < 0 || c1 < 0 || c2 < 0 || c0 == c1 || c0 == c2 || c1 == c2) { a.trot[3 * (size_t)k] = -1; continue; }   // degenerate
        const int n0 = a.cname[c0], n1 = a.cname[c1], n2 = a.cname[c2];
        const int r = n0 < n1 && n0 < n2 ? 0 : (n1 < n2 ? 1 : 2);   // the names differ as the clusters do
        a.trot[3 * (size_t)k] = r == 0 ? c0 : (r == 1 ? c1 : c2);
        a.trot[3 * (size_t)k + 1] = r == 0 ? c1 : (r == 1 ? c2 : c0);
        a.trot[3 * (size_t)k + 2] = r == 0 ? c2 : (r == 1 ? c0 : c1);
        mine++;
    }
    const int nd = block_sum_i(mine, s_sum);
    if (threadIdx.x == 0 && nd) atomicAdd(&a.meta[MD_NONDEG], nd);
}

__global__ __launch_bounds__(MDC_NT) void k_mdc_claim(MeshDecimateArgs a)
{
    const int nt = a.meta[MD_NT], lgt = a.meta[MD_LGT];
    const unsigned mask = (1u << lgt) - 1u;
    for (int k = blockIdx.x * MDC_NT + (int)threadIdx.x; k < nt; k += (int)gridDim.x * MDC_NT) {
        const int c0 = a.trot[3 * (size_t)k];
        if (c0 < 0) continue;
        const int c1 = a.trot[3 * (size_t)k + 1], c2 = a.trot[3 * (size_t)k + 2];
        unsigned h = mdc_tri_hash(c0, c1, c2, lgt);
        int at = -1;
        for (unsigned i = 0; i <= mask; i++) {
            int own = a.towner[h];
            if (own < 0) own = atomicCAS(&a.towner[h], -1, k);
            if (own < 0) { at = (int)h; break; }   // claimed
            // an entry's owner changes only to a triangle of the same triple: whichever owner was read decides
            if (a.trot[3 * (size_t)own] == c0 && a.trot[3 * (size_t)own + 1] == c1 && a.trot[3 * (size_t)own + 2] == c2) {
                atomicMin(&a.towner[h], k);
                at = (int)h;
                break;
            }
            h = (h + 1) & mask;
        }
        if (at < 0) atomicOr(a.status, (int)PGX_ST_INTERNAL);
        a.tslot[k] = at;
    }
}

// triangle k is kept: used, not degenerate, and the smallest index of its triple
__device__ __forceinline__ bool mdc_tkept(const MeshDecimateArgs &a, int k)
{
    if (a.trot[3 * (size_t)k] < 0) return false;
    const int at = a.tslot[k];
    return at >= 0 && a.towner[at] == k;
}

__global__ __launch_bounds__(MDC_NT) void k_mdc_mark(MeshDecimateArgs a)
{
    const int nt = a.meta[MD_NT];
    for (int k = blockIdx.x * MDC_NT + (int)threadIdx.x; k < nt; k += (int)gridDim.x * MDC_NT) {
        if (!mdc_tkept(a, k)) continue;
#pragma unroll
        for (int j = 0; j < 3; j++) a.cused[a.trot[3 * (size_t)k + j]] = 1;   // the same byte from every writer
    }
}

// index i as a vertex and as a triangle: the name of an output cluster or not (its entry in e), a kept triangle or not
__device__ __forceinline__ void mdc_item(const MeshDecimateArgs &a, int i, int nv, int nt, int &vk, int &tk, int &e)
{
    vk = tk = 0;
    e = -1;
    if (i < nv && a.member[i] == 1) {
        e = a.vslot[i];
        vk = e >= 0 && a.cname[e] == i && a.cused[e] ? 1 : 0;
    }
    if (i < nt) tk = mdc_tkept(a, i) ? 1 : 0;
}

__global__ __launch_bounds__(MDC_NT) void k_mdc_bsum(MeshDecimateArgs a)
{
    __shared__ int s_sum[4];
    const int nv = a.meta[MD_NV], nt = a.meta[MD_NT], n = nv > nt ? nv : nt, nbn = (n + MDC_NT - 1) / MDC_NT;
    for (int b = blockIdx.x; b < nbn; b += gridDim.x) {
        int vk, tk, e;
        mdc_item(a, b * MDC_NT + (int)threadIdx.x, nv, nt, vk, tk, e);
        const int sv = block_sum_i(vk, s_sum), st = block_sum_i(tk, s_sum);
        if (threadIdx.x == 0) a.bsum[b] = mesh_pack_kept(sv, st);
    }
}

__global__ __launch_bounds__(MDC_NT) void k_mdc_scan(MeshDecimateArgs a)
{
    __shared__ unsigned long long s_lds[MDC_NT / 64];
    const int nv = a.meta[MD_NV], nt = a.meta[MD_NT], n = nv > nt ? nv : nt, nbn = (n + MDC_NT - 1) / MDC_NT;
    const unsigned long long carry = block_scan_array<unsigned long long, MDC_NT>(a.bsum, a.boff, nbn, s_lds);
    if (threadIdx.x == 0) {
        const int vo = mesh_kept_vertices(carry), to = mesh_kept_tris(carry);
        a.meta[MD_VOUT] = vo;
        a.meta[MD_TOUT] = to;
        if (vo > a.max_out_vertices || to > a.max_out_tris) atomicOr((unsigned *)a.status, PGX_ST_MDC_CAP);
        a.report[0] = nv; a.report[1] = nt; a.report[2] = a.meta[MD_USED]; a.report[3] = a.meta[MD_CLUSTERS];
        a.report[4] = a.meta[MD_NONDEG] - to; a.report[5] = vo; a.report[6] = to; a.report[7] = 0;   // [7]: k_mdc_tnormal adds
    }
}

__global__ __launch_bounds__(MDC_NT) void k_mdc_rank(MeshDecimateArgs a)
{
    __shared__ unsigned long long s_lds[MDC_NT / 64];
    const int nv = a.meta[MD_NV], nt = a.meta[MD_NT], n = nv > nt ? nv : nt, nbn = (n + MDC_NT - 1) / MDC_NT;
    for (int b = blockIdx.x; b < nbn; b += gridDim.x) {
        const int i = b * MDC_NT + (int)threadIdx.x;
        int vk, tk, e;
        mdc_item(a, i, nv, nt, vk, tk, e);
        unsigned long long tot;
        const unsigned long long at = a.boff[b] + block_excl_scan<unsigned long long, MDC_NT>(mesh_pack_kept(vk, tk), s_lds, tot);
        if (vk) a.cnew[e] = mesh_kept_vertices(at);
        if (i < nt) a.tnew[i] = tk ? mesh_kept_tris(at) : -1;
    }
}

__global__ __launch_bounds__(MDC_NT) void k_mdc_emit(MeshDecimateArgs a)
{
    const int nv = a.meta[MD_NV], nt = a.meta[MD_NT], n = nv > nt ? nv : nt;
    const double o[3] = {a.ox, a.oy, a.oz};
    for (int i = blockIdx.x * MDC_NT + (int)threadIdx.x; i < n; i += (int)gridDim.x * MDC_NT) {
        if (i < nv) {
            const bool mem = a.member[i] == 1;
            const int e = mem ? a.vslot[i] : -1;
            if (a.vertex_map) a.vertex_map[i] = e >= 0 ? (a.cused[e] ? a.cnew[e] : -2) : -1;
            if (a.level) a.level[i] = e >= 0 ? (int)a.lev[i] : -1;
            if (e >= 0 && a.cname[e] == i) {   // the cluster's name: Q in place of the sums, whether it is in the output or not
                const int L = a.lev[i], cn = a.cn[e], w = a.cused[e] ? a.cnew[e] : -1;
                const long long n2 = 2ll * cn;
                const bool out = w >= 0 && w < a.max_out_vertices;
#pragma unroll
                for (int k = 0; k < 3; k++) {
                    const long long q = a.q[3 * (size_t)i + k], org = q - (q & ((1ll << (16 + L)) - 1));   // B << (16 + L)
                    const long long Q = org + (2ll * (long long)a.cs[3 * (size_t)e + k] + cn) / n2;
                    a.cs[3 * (size_t)e + k] = (unsigned long long)Q;
                    if (out) a.out_xyz[3 * (size_t)w + k] = mesh_q_to_world(o[k], Q, a.cell);
                }
                uint32_t c = 0;
#pragma unroll
                for (int k = 0; k < 4; k++) {
                    c |= (uint32_t)((2ll * (long long)a.csc[4 * (size_t)e + k] + cn) / n2) << (8 * k);
                    a.csc[4 * (size_t)e + k] = 0;   // [0..2]: the sums of k_mdc_tnormal from here on
                }
                if (out) {
                    a.out_rgba8[w] = c;
                    a.out_info[4 * (size_t)w] = i; a.out_info[4 * (size_t)w + 1] = L; a.out_info[4 * (size_t)w + 2] = cn; a.out_info[4 * (size_t)w + 3] = 0;
                }
            }
        }
        const int t = i < nt ? a.tnew[i] : -1;
        if (t >= 0 && t < a.max_out_tris) {
#pragma unroll
            for (int k = 0; k < 3; k++) a.out_tri[3 * (size_t)t + k] = a.cnew[a.trot[3 * (size_t)i + k]];
        }
    }
}

__global__ __launch_bounds__(MDC_NT) void k_mdc_tnormal(MeshDecimateArgs a)
{
    __shared__ int s_sum[4];
    const int nt = a.meta[MD_NT], nbt = (nt + MDC_NT - 1) / MDC_NT;
    int flipped = 0;
    for (int b = blockIdx.x; b < nbt; b += gridDim.x) {
        const int k = b * MDC_NT + (int)threadIdx.x;
        if (k >= nt || a.tnew[k] < 0) continue;
        const int c0 = a.trot[3 * (size_t)k], c1 = a.trot[3 * (size_t)k + 1], c2 = a.trot[3 * (size_t)k + 2];
        int m[3];
        mesh_tri_m((const long long *)a.cs + 3 * (size_t)c0, (const long long *)a.cs + 3 * (size_t)c1, (const long long *)a.cs + 3 * (size_t)c2, 32767.0, m);   // rule 7
        const unsigned long long w = a.tm[k];
        const long long dot = ((long long)m[0] * mesh_unpack_m(w, 0) + (long long)m[1] * mesh_unpack_m(w, 1)) + (long long)m[2] * mesh_unpack_m(w, 2);
        flipped += dot < 0 ? 1 : 0;
#pragma unroll
        for (int j = 0; j < 3; j++) {
            const int c = j == 0 ? c0 : (j == 1 ? c1 : c2);
#pragma unroll
            for (int x = 0; x < 3; x++)
                if (m[x]) atomicAdd(&a.csc[4 * (size_t)c + x], (unsigned long long)(long long)m[x]);
        }
    }
    const int nf = block_sum_i(flipped, s_sum);
    if (threadIdx.x == 0 && nf) atomicAdd(&a.report[7], nf);
}

__global__ __launch_bounds__(MDC_NT) void k_mdc_finish(MeshDecimateArgs a)
{
    const int nv = a.meta[MD_NV];
    for (int i = blockIdx.x * MDC_NT + (int)threadIdx.x; i < nv; i += (int)gridDim.x * MDC_NT) {
        if (a.member[i] != 1) continue;
        const int e = a.vslot[i];
        if (e < 0 || a.cname[e] != i || !a.cused[e]) continue;
        const int w = a.cnew[e];
        if (w < 0 || w >= a.max_out_vertices) continue;
        mesh_unit_normal(a.out_normal, w, a.csc[4 * (size_t)e], a.csc[4 * (size_t)e + 1], a.csc[4 * (size_t)e + 2]);
    }
}

// the workspace, described once: the arguments' workspace pointers (none valid for ws = nullptr) and the bytes
size_t mdc_carve(MeshDecimateArgs &a, void *ws)
{
    WsCarver w(ws);
    const size_t nv = (size_t)a.max_vertices, nt = (size_t)a.max_tris, n = nv > nt ? nv : nt;
    a.nb = n > 0 ? (int)((n + MDC_NT - 1) / MDC_NT) : 1;
    a.lg_vcap = mdc_lg(a.max_vertices);
    a.lg_tcap = mdc_lg(a.max_tris);
    const size_t TV = (size_t)1 << a.lg_vcap, TT = (size_t)1 << a.lg_tcap;
    a.q = w.take<long long>(nv * 24);
    a.member = w.take<unsigned char>(nv);
    a.lev = w.take<unsigned char>(nv);
    a.vslot = w.take<int32_t>(nv * 4);
    for (int t = 0; t < 2; t++) {
        a.fkey[t] = w.take<unsigned long long>(TV * 8);
        a.fsum[t] = w.take<unsigned long long>(TV * 32);
    }
    a.ckey = w.take<unsigned long long>(TV * 8);
    a.cname = w.take<int32_t>(TV * 4);
    a.cn = w.take<int32_t>(TV * 4);
    a.cnew = w.take<int32_t>(TV * 4);
    a.cused = w.take<unsigned char>(TV);
    a.cs = w.take<unsigned long long>(TV * 24);
    a.csc = w.take<unsigned long long>(TV * 32);
    a.trot = w.take<int32_t>(nt * 12);
    a.tm = w.take<unsigned long long>(nt * 8);
    a.tslot = w.take<int32_t>(nt * 4);
    a.tnew = w.take<int32_t>(nt * 4);
    a.towner = w.take<int32_t>(TT * 4);
    a.bsum = w.take<unsigned long long>((size_t)a.nb * 8);
    a.boff = w.take<unsigned long long>((size_t)a.nb * 8);
    a.meta = w.take<int32_t>(16 * 4);
    return w.total();
}

} // namespace

size_t pgx_mesh_decimate_ws_bytes(const MeshDecimateArgs &a)
{
    MeshDecimateArgs b = a;
    return mdc_carve(b, nullptr);
}

void pgx_launch_mesh_decimate(pgx_ctx *ctx, hipStream_t s, MeshDecimateArgs a, void *ws)
{
    mdc_carve(a, ws);
    const auto grid = [](size_t items) {
        const size_t b = items > 0 ? (items + MDC_NT - 1) / MDC_NT : 1;
        return dim3((unsigned)(b < (size_t)MDC_GRID_MAX ? b : (size_t)MDC_GRID_MAX));
    };
    const size_t nv = (size_t)a.max_vertices, nt = (size_t)a.max_tris, TV = (size_t)1 << a.lg_vcap, TT = (size_t)1 << a.lg_tcap;
    const dim3 vgrid = grid(nv), tgrid = grid(nt), ngrid = grid(nv > nt ? nv : nt), fgrid = grid(TV),
               igrid = grid(TV > TT ? (TV > nv ? TV : nv) : (TT > nv ? TT : nv));
    {
        ProfScope ps(ctx, "mdec_init", s);
        hipLaunchKernelGGL(k_mdc_plan, dim3(1), dim3(MDC_NT), 0, s, a);
        hipLaunchKernelGGL(k_mdc_init, igrid, dim3(MDC_NT), 0, s, a);
    }
    {
        ProfScope ps(ctx, "mdec_tris", s);
        hipLaunchKernelGGL(k_mdc_tris, tgrid, dim3(MDC_NT), 0, s, a);
    }
    if (a.lmax > a.lmin) {
        ProfScope ps(ctx, "mdec_levels", s);
        int t = 0;
        for (int l = a.lmin + 1; l <= a.lmax; l++) {
            hipLaunchKernelGGL(k_mdc_vlevel, vgrid, dim3(MDC_NT), 0, s, a, l, t);
            if (l < a.lmax) {
                hipLaunchKernelGGL(k_mdc_up, fgrid, dim3(MDC_NT), 0, s, a, t);
                t = 1 - t;
            }
        }
    }
    {
        ProfScope ps(ctx, "mdec_clusters", s);
        hipLaunchKernelGGL(k_mdc_clusters, vgrid, dim3(MDC_NT), 0, s, a);
        hipLaunchKernelGGL(k_mdc_vslot, vgrid, dim3(MDC_NT), 0, s, a);
    }
    {
        ProfScope ps(ctx, "mdec_dedup", s);
        hipLaunchKernelGGL(k_mdc_map, tgrid, dim3(MDC_NT), 0, s, a);
        hipLaunchKernelGGL(k_mdc_claim, tgrid, dim3(MDC_NT), 0, s, a);
        hipLaunchKernelGGL(k_mdc_mark, tgrid, dim3(MDC_NT), 0, s, a);
    }
    {
        ProfScope ps(ctx, "mdec_rank", s);
        hipLaunchKernelGGL(k_mdc_bsum, ngrid, dim3(MDC_NT), 0, s, a);
        hipLaunchKernelGGL(k_mdc_scan, dim3(1), dim3(MDC_NT), 0, s, a);
        hipLaunchKernelGGL(k_mdc_rank, ngrid, dim3(MDC_NT), 0, s, a);
    }
    {
        ProfScope ps(ctx, "mdec_emit", s);
        hipLaunchKernelGGL(k_mdc_emit, ngrid, dim3(MDC_NT), 0, s, a);
    }
    {
        ProfScope ps(ctx, "mdec_normals", s);
        hipLaunchKernelGGL(k_mdc_tnormal, tgrid, dim3(MDC_NT), 0, s, a);
        hipLaunchKernelGGL(k_mdc_finish, vgrid, dim3(MDC_NT), 0, s, a);
    }
}
