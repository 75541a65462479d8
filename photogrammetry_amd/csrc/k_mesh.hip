// k_mesh.hip -- a triangle mesh from the depth maps: a truncated signed distance on a hashed grid of lattice nodes round the
// filter's points, and naive surface nets: one vertex per cube with a sign change, one quad per lattice edge with a sign change
// (pgx_mesh_dev; include/pgx.h states the rule operation by operation).  Not in the C# reference.
//
// Eleven kernels on the caller's stream, none of which needs a count on the host:
//   k_msh_plan     clears the node table (grid-stride); its first workgroup also fills the filter's camera table per map, the
//                  slot that shows each map's frame, and n = min(d_count[0], max_in)
//   k_msh_seed     one thread per point: the used test and the key (pgx_cloudkey.h, the cloud's), and the insert of the node
//                  of the point's own cell: an open-addressing table of 1 << lg_table >= 2 max_voxels entries, linear probing
//                  from msh_hash(key), a 64-bit compare-and-swap on the key after a plain load, atomicMin on the cell's first point
//   k_msh_dilate   the first point of each cell inserts the (2 band)^3 nodes round its cell, atomicMin on ord = 256 i + nb
//   k_msh_tsdf     one thread per table entry: the node projected into every map, w, st and the colour sums in integers
//   k_msh_cubes    one thread per table entry: the eight nodes of the cube whose low node it is: complete, the INSIDE mask, active
//   k_msh_quads    one thread per table entry: per axis, whether the edge from the node has a quad (the four cubes round it)
//   k_msh_count    the vertices and quads owned by each point (ord >> 8) per block of 256 points
//   k_msh_scan     one workgroup: the exclusive scan of the block counts (both in one 64-bit value), the totals, the capacity
//                  status, d_report
//   k_msh_rank     the point's base (block_excl_scan) plus the nodes before it in the point's own nb order is a cube's vertex
//                  index and an edge's quad index: vertices and quads come out in ascending ord with no sort
//   k_msh_vertices one thread per table entry: the vertex of an active cube
//   k_msh_tris     one thread per table entry: the two triangles of each quad
// Every sum over maps and nodes is an integer: no order of execution changes a bit.  A table entry's neighbours are found by
// probing again: the table stores no links.  DESIGN.md section 29.
#include "pgx_stage_args.h"
#include "pgx_densecam.h"
#include "pgx_cloudkey.h"

namespace {

constexpr int MSH_NT = 256;            // threads per workgroup of every kernel here; the block of the owner scan
constexpr int MSH_GRID_MAX = 1024;     // workgroups of the per-point and per-entry kernels, grid-stride beyond
constexpr int MSH_LG_TMIN = 8;         // the table has at least 1 << 8 entries
constexpr int MSH_MARGIN = 4;          // a used point's g lies MSH_MARGIN cells inside the key's range: band <= 3 and one cube more
constexpr unsigned long long MSH_EMPTY = ~0ull;                    // no key: a key has 63 bits
constexpr unsigned long long MSH_NOORD = ~0ull;                    // no ord yet: an ord has 36 bits
constexpr int MSH_NOSEED = 0x7FFFFFFF;
constexpr unsigned long long MSH_HASH_MUL = 0x9E3779B97F4A7C15ull; // msh_hash: the top lg_table bits of key * this (mod 2^64)
enum { MM_N = 0, MM_USED, MM_SEEDS, MM_VOX, MM_VALID, MM_VERT, MM_QUAD };   // meta

__device__ __forceinline__ unsigned msh_hash(unsigned long long key, int lg) { return (unsigned)((key * MSH_HASH_MUL) >> (64 - lg)); }

// the entry of key, claimed if the key is new; -1 when a whole round of the table finds neither the key nor an empty entry
__device__ __forceinline__ int msh_insert(const MeshArgs &a, unsigned long long key)
{
    const unsigned mask = (1u << a.lg_table) - 1u;
    unsigned h = msh_hash(key, a.lg_table);
    for (unsigned tries = 0; tries <= mask; tries++, h = (h + 1) & mask) {
        unsigned long long prev = __atomic_load_n(&a.keys[h], __ATOMIC_RELAXED);
        if (prev == MSH_EMPTY) prev = atomicCAS(&a.keys[h], MSH_EMPTY, key);
        if (prev == MSH_EMPTY || prev == key) return (int)h;
    }
    return -1;
}

// the entry of key in the finished table, -1 if it has none
__device__ __forceinline__ int msh_find(const MeshArgs &a, unsigned long long key)
{
    const unsigned mask = (1u << a.lg_table) - 1u;
    unsigned h = msh_hash(key, a.lg_table);
    for (unsigned tries = 0; tries <= mask; tries++, h = (h + 1) & mask) {
        const unsigned long long k = a.keys[h];
        if (k == key) return (int)h;
        if (k == MSH_EMPTY) return -1;
    }
    return -1;
}

static_assert(MM_N == 0, "cld_plan_rows (pgx_cloudkey.h) leaves n in meta[0]");

// more voxels than max_voxels (a full table has more): nothing behind k_msh_tsdf runs
__device__ __forceinline__ bool msh_overflow(const MeshArgs &a) { return a.meta[MM_VOX] > a.max_voxels; }

__global__ __launch_bounds__(MSH_NT) void k_msh_plan(MeshArgs a)
{
    const size_t T = (size_t)1 << a.lg_table;
    for (size_t i = (size_t)blockIdx.x * MSH_NT + threadIdx.x; i < T; i += (size_t)gridDim.x * MSH_NT) {
        a.keys[i] = MSH_EMPTY;
        a.ord[i] = MSH_NOORD;
        a.sfirst[i] = MSH_NOSEED;
    }
    if (blockIdx.x != 0) return;
    cld_plan_rows<MSH_NT>(a);
}

__global__ __launch_bounds__(MSH_NT) void k_msh_seed(MeshArgs a)
{
    __shared__ int s_sum[4];
    const int n = a.meta[MM_N], nbn = (n + MSH_NT - 1) / MSH_NT, npix = a.W * a.H;
    for (int b = blockIdx.x; b < nbn; b += gridDim.x) {
        const int i = b * MSH_NT + (int)threadIdx.x;
        int used = 0;
        if (i < n) {
            int r, pix, sl = -1;
            unsigned long long key, pk;
            bool ok = cld_point_key(a.xyz, a.src, (size_t)i, a.R, npix, a.cell, a.ox, a.oy, a.oz, r, pix, key, pk);
#pragma unroll
            for (int k = 0; k < 3; k++) {
                const int g = cld_key_g(key, k);
                ok = ok && g >= -CLD_GBIAS + MSH_MARGIN && g < CLD_GBIAS - MSH_MARGIN;
            }
            if (ok) {
                used = 1;
                sl = msh_insert(a, key);
                if (sl >= 0) atomicMin(&a.sfirst[sl], i);
            }
            a.slot[i] = sl;
        }
        const int nu = block_sum_i(used, s_sum);
        if (threadIdx.x == 0 && nu) atomicAdd(&a.meta[MM_USED], nu);
    }
}

// point i is the first of its cell: key = the cell's
__device__ __forceinline__ bool msh_is_seed(const MeshArgs &a, int i, int n, unsigned long long &key)
{
    const int sl = i < n ? a.slot[i] : -1;
    if (sl < 0 || a.sfirst[sl] != i) return false;
    key = a.keys[sl];
    return true;
}

// node nb of the (2 band)^3 round the cell of key
__device__ __forceinline__ unsigned long long msh_band_key(const MeshArgs &a, unsigned long long key, int nb)
{
    const int B2 = 2 * a.band, d0 = nb % B2, d1 = (nb / B2) % B2, d2 = nb / (B2 * B2), lo = a.band - 1;
    return cld_key_of(cld_key_g(key, 0) - lo + d0, cld_key_g(key, 1) - lo + d1, cld_key_g(key, 2) - lo + d2);
}

__global__ __launch_bounds__(MSH_NT) void k_msh_dilate(MeshArgs a)
{
    __shared__ int s_sum[4];
    const int n = a.meta[MM_N], nbn = (n + MSH_NT - 1) / MSH_NT, nnb = 8 * a.band * a.band * a.band;
    for (int b = blockIdx.x; b < nbn; b += gridDim.x) {
        const int i = b * MSH_NT + (int)threadIdx.x;
        unsigned long long key = 0;
        const bool seed = msh_is_seed(a, i, n, key);
        if (seed)
            for (int nb = 0; nb < nnb; nb++) {
                const int e = msh_insert(a, msh_band_key(a, key, nb));
                if (e >= 0) atomicMin(&a.ord[e], 256ull * (unsigned long long)i + (unsigned long long)nb);
            }
        const int ns = block_sum_i(seed ? 1 : 0, s_sum);
        if (threadIdx.x == 0 && ns) atomicAdd(&a.meta[MM_SEEDS], ns);
    }
}

// rule 3 for the node of every occupied entry
__global__ __launch_bounds__(MSH_NT) void k_msh_tsdf(MeshArgs a)
{
    __shared__ int s_sum[4];
    const int T = 1 << a.lg_table, nbt = T / MSH_NT, npix = a.W * a.H;
    const double trunc = (double)a.trunc_cells * a.cell;
    for (int b = blockIdx.x; b < nbt; b += gridDim.x) {
        const int e = b * MSH_NT + (int)threadIdx.x;
        const unsigned long long key = a.keys[e];
        const int occ = key != MSH_EMPTY;
        int valid = 0, inside = 0;
        if (occ) {
            const double X0 = a.ox + (double)cld_key_g(key, 0) * a.cell, X1 = a.oy + (double)cld_key_g(key, 1) * a.cell,
                         X2 = a.oz + (double)cld_key_g(key, 2) * a.cell;
            int w = 0, st = 0, nc = 0, s0 = 0, s1 = 0, s2 = 0;
            for (int r = 0; r < a.R; r++) {
                const double *c = a.cam + (size_t)r * FUSE_CAM;
                if (c[12] == 0.0) continue;
                const double *p = a.P + (size_t)a.views[(size_t)r * (1 + a.S)] * 12;
                const double q0 = ((p[0] * X0 + p[1] * X1) + p[2] * X2) + p[3];
                const double q1 = ((p[4] * X0 + p[5] * X1) + p[6] * X2) + p[7];
                const double q2 = ((p[8] * X0 + p[9] * X1) + p[10] * X2) + p[11];
                int iu, iv;
                if (!dep_pixel(q0, q1, q2, a.W, a.H, iu, iv)) continue;
                const size_t pix = (size_t)iv * a.W + iu;
                const double z = a.depth[(size_t)r * npix + pix];
                if (!isfinite(z)) continue;
                if (a.agree && a.agree[(size_t)r * npix + pix] < a.min_agree) continue;
                const double d = (c[10] * q2) / c[11], s = z - d;
                if (!(s >= -trunc)) continue;   // behind the surface (NaN: passed over)
                const double t = s > trunc ? trunc : s;
                w += 1;
                st += (int)floor((t / trunc) * 32767.0 + 0.5);
                const int cs = a.cslot[r];
                if (s <= trunc && cs >= 0) {
                    const unsigned colr = a.rgba8[(size_t)cs * npix + pix];
                    nc += 1;
                    s0 += (int)(colr & 255u); s1 += (int)((colr >> 8) & 255u); s2 += (int)((colr >> 16) & 255u);
                }
            }
            valid = w >= a.min_weight;
            inside = valid && st < 0;
            a.wst[2 * (size_t)e] = w;
            a.wst[2 * (size_t)e + 1] = st;
            a.col[4 * (size_t)e] = nc; a.col[4 * (size_t)e + 1] = s0; a.col[4 * (size_t)e + 2] = s1; a.col[4 * (size_t)e + 3] = s2;
        }
        a.nflag[e] = (unsigned char)(valid | inside << 1);
        const int no = block_sum_i(occ, s_sum), nv = block_sum_i(valid, s_sum);
        if (threadIdx.x == 0) {
            if (no) atomicAdd(&a.meta[MM_VOX], no);
            if (nv) atomicAdd(&a.meta[MM_VALID], nv);
        }
    }
}

// the key of node j of the cube at key
__device__ __forceinline__ unsigned long long msh_corner(unsigned long long key, int j)
{
    return key + ((unsigned long long)(j & 1) << 42) + ((unsigned long long)((j >> 1) & 1) << 21) + (unsigned long long)((j >> 2) & 1);
}

__global__ __launch_bounds__(MSH_NT) void k_msh_cubes(MeshArgs a)
{
    if (msh_overflow(a)) return;
    const size_t T = (size_t)1 << a.lg_table;
    for (size_t e = (size_t)blockIdx.x * MSH_NT + threadIdx.x; e < T; e += (size_t)gridDim.x * MSH_NT) {
        const unsigned long long key = a.keys[e];
        if (key == MSH_EMPTY) continue;
        const int f0 = a.nflag[e];
        bool complete = f0 & 1;
        int mask = f0 >> 1;
        for (int j = 1; j < 8 && complete; j++) {
            const int ej = msh_find(a, msh_corner(key, j));
            const int f = ej >= 0 ? a.nflag[ej] : 0;
            complete = f & 1;
            mask |= (f >> 1) << j;
        }
        a.cflag[e] = complete ? (mask | 1 << 8 | (mask != 0 && mask != 255 ? 1 << 9 : 0)) : 0;
    }
}

// the key of the node one step back along axis k
__device__ __forceinline__ unsigned long long msh_back(unsigned long long key, int k) { return key - (1ull << (21 * (2 - k))); }

__global__ __launch_bounds__(MSH_NT) void k_msh_quads(MeshArgs a)
{
    if (msh_overflow(a)) return;
    const size_t T = (size_t)1 << a.lg_table;
    for (size_t e = (size_t)blockIdx.x * MSH_NT + threadIdx.x; e < T; e += (size_t)gridDim.x * MSH_NT) {
        const unsigned long long key = a.keys[e];
        if (key == MSH_EMPTY) continue;
        const int cf = a.cflag[e];
        int qb = 0;
        if (cf & 256) {   // Q2 = the node's own cube is complete: the node and its three successors are valid
#pragma unroll
            for (int ax = 0; ax < 3; ax++) {
                if ((cf & 1) == ((cf >> (1 << ax)) & 1)) continue;
                const int b = (ax + 1) % 3, c = (ax + 2) % 3;
                const int e1 = msh_find(a, msh_back(key, c));
                if (e1 < 0 || !(a.cflag[e1] & 256)) continue;
                const int e3 = msh_find(a, msh_back(key, b));
                if (e3 < 0 || !(a.cflag[e3] & 256)) continue;
                const int e0 = msh_find(a, msh_back(msh_back(key, b), c));
                if (e0 < 0 || !(a.cflag[e0] & 256)) continue;
                qb |= 1 << ax;
            }
        }
        a.qflag[e] = (unsigned char)qb;
    }
}

// The nodes that point i owns (ord >> 8 == i), in ascending ord: their vertices and quads counted, and with WRITE the indices
// from vbase and qbase handed out.
template <bool WRITE>
__device__ __forceinline__ void msh_owned(const MeshArgs &a, int i, int n, int vbase, int qbase, int &nv, int &nq)
{
    nv = nq = 0;
    unsigned long long key = 0;
    if (!msh_is_seed(a, i, n, key)) return;
    const int nnb = 8 * a.band * a.band * a.band;
    for (int nb = 0; nb < nnb; nb++) {
        const int e = msh_find(a, msh_band_key(a, key, nb));
        if (e < 0 || a.ord[e] != 256ull * (unsigned long long)i + (unsigned long long)nb) continue;
        if (WRITE) {
            a.vidx[e] = vbase + nv;
            a.qidx[e] = qbase + nq;
        }
        nv += (a.cflag[e] >> 9) & 1;
        nq += __popc((unsigned)a.qflag[e]);
    }
}

__global__ __launch_bounds__(MSH_NT) void k_msh_count(MeshArgs a)
{
    __shared__ int s_sum[4];
    if (msh_overflow(a)) return;
    const int n = a.meta[MM_N], nbn = (n + MSH_NT - 1) / MSH_NT;
    for (int b = blockIdx.x; b < nbn; b += gridDim.x) {
        int nv, nq;
        msh_owned<false>(a, b * MSH_NT + (int)threadIdx.x, n, 0, 0, nv, nq);
        const int tv = block_sum_i(nv, s_sum), tq = block_sum_i(nq, s_sum);
        if (threadIdx.x == 0) a.bsum[b] = (unsigned long long)(unsigned)tv | (unsigned long long)(unsigned)tq << 32;
    }
}

__global__ __launch_bounds__(MSH_NT) void k_msh_scan(MeshArgs a)
{
    __shared__ unsigned long long s_lds[MSH_NT / 64];
    const int n = a.meta[MM_N], nbn = (n + MSH_NT - 1) / MSH_NT;
    const bool over = msh_overflow(a);
    const unsigned long long carry = block_scan_array<unsigned long long, MSH_NT>(a.bsum, a.boff, over ? 0 : nbn, s_lds);
    if (threadIdx.x == 0) {
        const int nv = (int)(carry & 0xFFFFFFFFull), nq = (int)(carry >> 32);
        a.meta[MM_VERT] = nv;
        a.meta[MM_QUAD] = nq;
        if (over || nv > a.max_vertices || 2ll * nq > (long long)a.max_tris) atomicOr(a.status, (int)PGX_ST_MSH_CAP);
        a.report[0] = n; a.report[1] = a.meta[MM_USED]; a.report[2] = a.meta[MM_SEEDS]; a.report[3] = a.meta[MM_VOX];
        a.report[4] = a.meta[MM_VALID]; a.report[5] = nv; a.report[6] = 2 * nq; a.report[7] = 0;
    }
}

__global__ __launch_bounds__(MSH_NT) void k_msh_rank(MeshArgs a)
{
    __shared__ unsigned long long s_lds[MSH_NT / 64];
    if (msh_overflow(a)) return;
    const int n = a.meta[MM_N], nbn = (n + MSH_NT - 1) / MSH_NT;
    for (int b = blockIdx.x; b < nbn; b += gridDim.x) {
        const int i = b * MSH_NT + (int)threadIdx.x;
        int nv, nq;
        msh_owned<false>(a, i, n, 0, 0, nv, nq);
        unsigned long long tot;
        const unsigned long long base =
            a.boff[b] + block_excl_scan<unsigned long long, MSH_NT>((unsigned long long)(unsigned)nv | (unsigned long long)(unsigned)nq << 32, s_lds, tot);
        if (nv | nq) msh_owned<true>(a, i, n, (int)(base & 0xFFFFFFFFull), (int)(base >> 32), nv, nq);
    }
}

// rule 4 for the cube of every entry that has a vertex below the capacity
__global__ __launch_bounds__(MSH_NT) void k_msh_vertices(MeshArgs a)
{
    if (msh_overflow(a)) return;
    const size_t T = (size_t)1 << a.lg_table;
    for (size_t e = (size_t)blockIdx.x * MSH_NT + threadIdx.x; e < T; e += (size_t)gridDim.x * MSH_NT) {
        const unsigned long long key = a.keys[e];
        if (key == MSH_EMPTY) continue;
        const int cf = a.cflag[e];
        if (!(cf & 512)) continue;
        const int v = a.vidx[e];
        if (v >= a.max_vertices) continue;
        double phi[8];
        int nc = 0, sc0 = 0, sc1 = 0, sc2 = 0;
#pragma unroll
        for (int j = 0; j < 8; j++) {
            const int ej = j == 0 ? (int)e : msh_find(a, msh_corner(key, j));   // found: the cube is complete
            phi[j] = (double)a.wst[2 * (size_t)ej + 1] / (double)a.wst[2 * (size_t)ej];
            nc += a.col[4 * (size_t)ej]; sc0 += a.col[4 * (size_t)ej + 1]; sc1 += a.col[4 * (size_t)ej + 2]; sc2 += a.col[4 * (size_t)ej + 3];
        }
        double m0 = 0.0, m1 = 0.0, m2 = 0.0, G[3];
        int k = 0;
#pragma unroll
        for (int ax = 0; ax < 3; ax++) {
            const int lb = ax == 0 ? 1 : 0, hb = ax == 2 ? 1 : 2;   // the two other axes, the lower one first
            double g = 0.0;
#pragma unroll
            for (int t = 0; t < 4; t++) {
                const int lo = (t & 1) << lb | (t >> 1) << hb, hi = lo | 1 << ax;
                g += phi[hi] - phi[lo];
                if (((cf >> lo) & 1) != ((cf >> hi) & 1)) {
                    const double tau = phi[lo] / (phi[lo] - phi[hi]);
                    m0 += ax == 0 ? tau : (double)(lo & 1);
                    m1 += ax == 1 ? tau : (double)((lo >> 1) & 1);
                    m2 += ax == 2 ? tau : (double)((lo >> 2) & 1);
                    k++;
                }
            }
            G[ax] = g;
        }
        const double kd = (double)k;
        a.out_xyz[3 * (size_t)v] = a.ox + ((double)cld_key_g(key, 0) + m0 / kd) * a.cell;
        a.out_xyz[3 * (size_t)v + 1] = a.oy + ((double)cld_key_g(key, 1) + m1 / kd) * a.cell;
        a.out_xyz[3 * (size_t)v + 2] = a.oz + ((double)cld_key_g(key, 2) + m2 / kd) * a.cell;
        const double L = sqrt((G[0] * G[0] + G[1] * G[1]) + G[2] * G[2]);
        const bool hn = L != 0.0 && isfinite(L);
        a.out_normal[3 * (size_t)v] = hn ? (float)(G[0] / L) : 0.0f;
        a.out_normal[3 * (size_t)v + 1] = hn ? (float)(G[1] / L) : 0.0f;
        a.out_normal[3 * (size_t)v + 2] = hn ? (float)(G[2] / L) : 0.0f;
        unsigned colr = 0;
        if (nc != 0) {
            const long long d = 2 * (long long)nc;
            colr = (unsigned)((2 * (long long)sc0 + nc) / d) | (unsigned)((2 * (long long)sc1 + nc) / d) << 8 |
                   (unsigned)((2 * (long long)sc2 + nc) / d) << 16 | 255u << 24;
        }
        a.out_rgba8[v] = colr;
        a.out_info[4 * (size_t)v] = cld_key_g(key, 0);
        a.out_info[4 * (size_t)v + 1] = cld_key_g(key, 1);
        a.out_info[4 * (size_t)v + 2] = cld_key_g(key, 2);
        a.out_info[4 * (size_t)v + 3] = (cf & 255) | k << 8;
    }
}

// rule 5 for every edge that has a quad
__global__ __launch_bounds__(MSH_NT) void k_msh_tris(MeshArgs a)
{
    if (msh_overflow(a)) return;
    const size_t T = (size_t)1 << a.lg_table;
    for (size_t e = (size_t)blockIdx.x * MSH_NT + threadIdx.x; e < T; e += (size_t)gridDim.x * MSH_NT) {
        const unsigned long long key = a.keys[e];
        if (key == MSH_EMPTY) continue;
        const int qb = a.qflag[e];
        if (!qb) continue;
        int q = a.qidx[e];
        const int v2 = a.vidx[e], in = a.cflag[e] & 1;
#pragma unroll
        for (int ax = 0; ax < 3; ax++) {
            if (!((qb >> ax) & 1)) continue;
            const long long t0 = 2ll * q;
            q++;
            if (t0 >= (long long)a.max_tris) continue;
            const int b = (ax + 1) % 3, c = (ax + 2) % 3;
            const int v1 = a.vidx[msh_find(a, msh_back(key, c))], v3 = a.vidx[msh_find(a, msh_back(key, b))],
                      v0 = a.vidx[msh_find(a, msh_back(msh_back(key, b), c))];   // found: k_msh_quads found them
            int32_t *o = a.out_tri + 3 * (size_t)t0;
            o[0] = v0; o[1] = in ? v1 : v2; o[2] = in ? v2 : v1;
            if (t0 + 1 < (long long)a.max_tris) { o[3] = v0; o[4] = in ? v2 : v3; o[5] = in ? v3 : v2; }
        }
    }
}

// the workspace, described once: the arguments' workspace pointers (none valid for ws = nullptr) and the bytes
size_t msh_carve(MeshArgs &a, void *ws)
{
    WsCarver w(ws);
    a.lg_table = MSH_LG_TMIN;
    while (((size_t)1 << a.lg_table) < 2 * (size_t)a.max_voxels) a.lg_table++;
    const size_t T = (size_t)1 << a.lg_table, n = (size_t)a.max_in;
    a.nb = a.max_in > 0 ? (a.max_in + MSH_NT - 1) / MSH_NT : 1;
    a.keys = w.take<unsigned long long>(T * 8);
    a.ord = w.take<unsigned long long>(T * 8);
    a.sfirst = w.take<int32_t>(T * 4);
    a.wst = w.take<int32_t>(T * 8);
    a.col = w.take<int32_t>(T * 16);
    a.cflag = w.take<int32_t>(T * 4);
    a.vidx = w.take<int32_t>(T * 4);
    a.qidx = w.take<int32_t>(T * 4);
    a.nflag = w.take<unsigned char>(T);
    a.qflag = w.take<unsigned char>(T);
    a.cam = w.take<double>((size_t)a.R * FUSE_CAM * sizeof(double));
    a.cslot = w.take<int32_t>((size_t)a.R * 4);
    a.slot = w.take<int32_t>(n * 4);
    a.bsum = w.take<unsigned long long>((size_t)a.nb * 8);
    a.boff = w.take<unsigned long long>((size_t)a.nb * 8);
    a.meta = w.take<int32_t>(8 * 4);
    return w.total();
}

} // namespace

size_t pgx_mesh_ws_bytes(const MeshArgs &a)
{
    MeshArgs b = a;
    return msh_carve(b, nullptr);
}

void pgx_launch_mesh(pgx_ctx *ctx, hipStream_t s, MeshArgs a, void *ws)
{
    msh_carve(a, ws);
    const unsigned pgrid = (unsigned)(a.nb < MSH_GRID_MAX ? a.nb : MSH_GRID_MAX);
    const size_t tb = ((size_t)1 << a.lg_table) / MSH_NT;
    const unsigned tgrid = (unsigned)(tb < MSH_GRID_MAX ? tb : MSH_GRID_MAX);
    {
        ProfScope ps(ctx, "mesh_plan", s);
        hipLaunchKernelGGL(k_msh_plan, dim3(tgrid), dim3(MSH_NT), 0, s, a);
    }
    {
        ProfScope ps(ctx, "mesh_seed", s);
        hipLaunchKernelGGL(k_msh_seed, dim3(pgrid), dim3(MSH_NT), 0, s, a);
    }
    {
        ProfScope ps(ctx, "mesh_dilate", s);
        hipLaunchKernelGGL(k_msh_dilate, dim3(pgrid), dim3(MSH_NT), 0, s, a);
    }
    {
        ProfScope ps(ctx, "mesh_tsdf", s);
        hipLaunchKernelGGL(k_msh_tsdf, dim3(tgrid), dim3(MSH_NT), 0, s, a);
    }
    {
        ProfScope ps(ctx, "mesh_cubes", s);
        hipLaunchKernelGGL(k_msh_cubes, dim3(tgrid), dim3(MSH_NT), 0, s, a);
        hipLaunchKernelGGL(k_msh_quads, dim3(tgrid), dim3(MSH_NT), 0, s, a);
    }
    {
        ProfScope ps(ctx, "mesh_rank", s);
        hipLaunchKernelGGL(k_msh_count, dim3(pgrid), dim3(MSH_NT), 0, s, a);
        hipLaunchKernelGGL(k_msh_scan, dim3(1), dim3(MSH_NT), 0, s, a);
        hipLaunchKernelGGL(k_msh_rank, dim3(pgrid), dim3(MSH_NT), 0, s, a);
    }
    if (a.max_vertices > 0) {
        ProfScope ps(ctx, "mesh_vertices", s);
        hipLaunchKernelGGL(k_msh_vertices, dim3(tgrid), dim3(MSH_NT), 0, s, a);
    }
    if (a.max_tris > 0) {
        ProfScope ps(ctx, "mesh_tris", s);
        hipLaunchKernelGGL(k_msh_tris, dim3(tgrid), dim3(MSH_NT), 0, s, a);
    }
}
