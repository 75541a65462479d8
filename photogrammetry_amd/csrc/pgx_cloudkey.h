// pgx_cloudkey.h -- what the stages that bin a point list into a grid share (k_cloud.hip: the merged cloud; k_mesh.hip: the
// mesh's seed cells): rule 1 of pgx_cloud_merge_dev (include/pgx.h), i.e. the used test, g = floor((X - o) / cell), the key and
// the position in the cell, and the colour slot of a frame.  One copy, so that a point of the mesh's list lies in the cell the
// cloud puts it in.  Every line is the arithmetic of include/pgx.h in its order.  Besides the rule, the tail that the two plan
// kernels share (cld_plan_rows).  Each file keeps its own table of keys: tests/cloud_ref.py and tests/mesh_ref.py hold the hash
// and the probe to the text of k_cloud.hip and k_mesh.hip.  Internal to libpgx.so; DESIGN.md section 14i.
#pragma once

#include "pgx_block.h"      // pgx_clamp_count
#include "pgx_densecam.h"   // fuse_camera_row

constexpr int CLD_GBIAS = 1 << 20;     // g + CLD_GBIAS is a cell coordinate's 21-bit field of the key

// Point i of the list: its src (r, pix), whether it is USED, its key, and pk = p (3 x 16 bits); key and pk hold zeros in the
// fields of an axis that fails.  npix = W H.
__device__ __forceinline__ bool cld_point_key(const double *xyz, const int32_t *src, size_t i, int R, int npix, double cell, double ox,
                                              double oy, double oz, int &r, int &pix, unsigned long long &key, unsigned long long &pk)
{
    r = src[2 * i];
    pix = src[2 * i + 1];
    bool ok = r >= 0 && r < R && pix >= 0 && pix < npix;
    key = 0;
    pk = 0;
#pragma unroll
    for (int k = 0; k < 3; k++) {
        const double X = xyz[3 * i + k], org = k == 0 ? ox : (k == 1 ? oy : oz);
        const double t = (X - org) / cell, g = floor(t);
        const bool in = isfinite(X) && g >= -1048576.0 && g < 1048576.0;   // NaN fails
        ok = ok && in;
        key = (key << 21) | (unsigned long long)(in ? (long long)g + CLD_GBIAS : 0);
        pk |= (unsigned long long)(in ? (int)floor((t - g) * 65536.0) : 0) << (16 * k);
    }
    return ok;
}

// coordinate k of a key's cell
__device__ __forceinline__ int cld_key_g(unsigned long long key, int k) { return (int)((key >> (21 * (2 - k))) & 0x1FFFFFull) - CLD_GBIAS; }

__device__ __forceinline__ unsigned long long cld_key_of(int g0, int g1, int g2)
{
    return (unsigned long long)(g0 + CLD_GBIAS) << 42 | (unsigned long long)(g1 + CLD_GBIAS) << 21 | (unsigned long long)(g2 + CLD_GBIAS);
}

// the lowest slot that shows frame f, -1 if none does, f is no frame number or there are no colours (A: CloudArgs, MeshArgs)
template <class A> __device__ __forceinline__ int cld_slot(const A &a, int f)
{
    if (!a.rgba8 || f < 0 || f >= a.n_frames) return -1;
    if (!a.frame_ids) return f < a.F ? f : -1;
    for (int s = 0; s < a.F; s++)
        if (a.frame_ids[s] == f) return s;
    return -1;
}

// The tail of a plan kernel, one workgroup of NT threads: per map the filter's camera row and the slot that shows its frame,
// meta[0] = n = min(d_count[0], max_in) (no count: max_in), the other seven counters zero (A: CloudArgs, MeshArgs)
template <int NT, class A> __device__ __forceinline__ void cld_plan_rows(const A &a)
{
    for (int r = threadIdx.x; r < a.R; r += NT) {
        const int fr = a.views[(size_t)r * (1 + a.S)];
        fuse_camera_row(a.P, a.n_frames, fr, a.cam + (size_t)r * FUSE_CAM);
        a.cslot[r] = cld_slot(a, fr);
    }
    if (threadIdx.x == 0) {
        a.meta[0] = a.count ? pgx_clamp_count(a.count[0], a.max_in) : a.max_in;
#pragma unroll
        for (int k = 1; k < 8; k++) a.meta[k] = 0;
    }
}
