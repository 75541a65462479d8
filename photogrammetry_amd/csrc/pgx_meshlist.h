// pgx_meshlist.h -- what the stages that take a mesh in pgx_mesh_dev's layout (xyz, normal, rgba8, info, tri, counts) and write
// one in the same layout do to every such list (k_meshclean.hip, k_meshdecimate.hip): the counts, the fixed-point position of a
// vertex with its valid test, m of a triangle (16 bits a component), the unit normal from three integer sums, a fixed-point
// position back in the world, and the (vertices, triangles) pair that bsum / scan / rank number the output by.  One copy, so that
// a rule of the layout changes in one place.  Every line is the arithmetic of include/pgx.h in its order (the build is
// -ffp-contract=off and the outputs are compared bit for bit).  Internal to libpgx.so; DESIGN.md section 14j.
#pragma once

#include "pgx_block.h"      // pgx_clamp_count

// nv and nt of the list: counts[5] and counts[6] clamped to the capacities, the capacities themselves without counts
__device__ __forceinline__ void mesh_counts(const int32_t *counts, int max_vertices, int max_tris, int &nv, int &nt)
{
    nv = counts ? pgx_clamp_count(counts[5], max_vertices) : max_vertices;
    nt = counts ? pgx_clamp_count(counts[6], max_tris) : max_tris;
}

// q = floor(t * 65536 + 0.5), t = (X - o) / cell, of vertex v, not clamped; true when the vertex is valid.
// When it is not, q is whatever the conversion of a NaN or of a value out of range gave: the caller must not store it
__device__ __forceinline__ bool mesh_fix_q(const double *xyz, size_t v, const double (&o)[3], double cell, long long (&q)[3])
{
    bool ok = true;
#pragma unroll
    for (int k = 0; k < 3; k++) {
        const double X = xyz[3 * v + k], t = (X - o[k]) / cell;
        ok = ok && isfinite(X) && t >= -1048576.0 && t < 1048576.0;
        q[k] = (long long)floor(t * 65536.0 + 0.5);
    }
    return ok;
}

// coordinate k of a fixed-point position in the world
__device__ __forceinline__ double mesh_q_to_world(double o_k, long long q, double cell) { return o_k + ((double)q / 65536.0) * cell; }

// m = floor((n / L) * scale + 0.5) of the normal n of the triangle (qa, qb, qc); false and zeros when L is 0 or not finite
__device__ __forceinline__ bool mesh_tri_m(const long long *qa, const long long *qb, const long long *qc, double scale, int (&m)[3])
{
    double e1[3], e2[3];
#pragma unroll
    for (int c = 0; c < 3; c++) {
        e1[c] = (double)(long long)((unsigned long long)qb[c] - (unsigned long long)qa[c]);
        e2[c] = (double)(long long)((unsigned long long)qc[c] - (unsigned long long)qa[c]);
    }
    const double n0 = e1[1] * e2[2] - e1[2] * e2[1], n1 = e1[2] * e2[0] - e1[0] * e2[2], n2 = e1[0] * e2[1] - e1[1] * e2[0];
    const double L = sqrt((n0 * n0 + n1 * n1) + n2 * n2);
    const bool ok = L != 0.0 && isfinite(L);
    m[0] = ok ? (int)floor((n0 / L) * scale + 0.5) : 0;
    m[1] = ok ? (int)floor((n1 / L) * scale + 0.5) : 0;
    m[2] = ok ? (int)floor((n2 / L) * scale + 0.5) : 0;
    return ok;
}

// m in one word, 16 bits a component, and component k of such a word
__device__ __forceinline__ unsigned long long mesh_pack_m(const int (&m)[3])
{
    return (unsigned long long)(m[0] & 0xFFFF) | (unsigned long long)(m[1] & 0xFFFF) << 16 | (unsigned long long)(m[2] & 0xFFFF) << 32;
}
__device__ __forceinline__ int mesh_unpack_m(unsigned long long w, int k) { return (int)(short)((w >> (16 * k)) & 0xFFFF); }

// the normal of output vertex w from the int64 sums of its triangles' m: s / L, zeros when L is 0
__device__ __forceinline__ void mesh_unit_normal(float *out_normal, int w, unsigned long long s0, unsigned long long s1, unsigned long long s2)
{
    const double x0 = (double)(long long)s0, x1 = (double)(long long)s1, x2 = (double)(long long)s2, L = sqrt((x0 * x0 + x1 * x1) + x2 * x2);
    const bool hn = L != 0.0;
    out_normal[3 * (size_t)w] = hn ? (float)(x0 / L) : 0.0f;
    out_normal[3 * (size_t)w + 1] = hn ? (float)(x1 / L) : 0.0f;
    out_normal[3 * (size_t)w + 2] = hn ? (float)(x2 / L) : 0.0f;
}

// whether an index is a kept vertex and a kept triangle, as one value that the block sums, the scan and the rank add up
__device__ __forceinline__ unsigned long long mesh_pack_kept(int vk, int tk) { return (unsigned long long)(unsigned)vk | (unsigned long long)(unsigned)tk << 32; }
__device__ __forceinline__ int mesh_kept_vertices(unsigned long long x) { return (int)(x & 0xFFFFFFFFull); }
__device__ __forceinline__ int mesh_kept_tris(unsigned long long x) { return (int)(x >> 32); }
