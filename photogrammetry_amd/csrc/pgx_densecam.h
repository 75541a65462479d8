// pgx_densecam.h -- the camera algebra that the dense stages share (k_depth.hip: depth maps and the cross-view filter;
// k_cloud.hip: the merged cloud's normals): adjugate and determinant of a 3 x 4 camera, ||m3||, the filter's camera table and
// its back-projection, and the rule's nearest-pixel test.  One copy, so that a pixel's X in the cloud is the X the filter wrote.
// Every line is the arithmetic of include/pgx.h in its order; the library is built without contraction.  Internal to libpgx.so.
#pragma once

#include <hip/hip_runtime.h>

constexpr int FUSE_CAM = 16;           // doubles per map in the filter's camera table: adj (9), det, sign, ||m3||, known, 3 unused

// adj(M) (adj[3 i + j]; M^-1 = adj / det) and det M of a 3 x 4 camera; false if an entry is not finite or det == 0
__device__ __forceinline__ bool dep_camera(const double *p, double (&adj)[9], double &det)
{
    bool fin = true;
#pragma unroll
    for (int k = 0; k < 12; k++) fin = fin && isfinite(p[k]);
    const double m00 = p[0], m01 = p[1], m02 = p[2], m10 = p[4], m11 = p[5], m12 = p[6], m20 = p[8], m21 = p[9], m22 = p[10];
    adj[0] = m11 * m22 - m12 * m21; adj[3] = m12 * m20 - m10 * m22; adj[6] = m10 * m21 - m11 * m20;
    adj[1] = m02 * m21 - m01 * m22; adj[4] = m00 * m22 - m02 * m20; adj[7] = m01 * m20 - m00 * m21;
    adj[2] = m01 * m12 - m02 * m11; adj[5] = m02 * m10 - m00 * m12; adj[8] = m00 * m11 - m01 * m10;
    det = (m00 * adj[0] + m01 * adj[3]) + m02 * adj[6];
    return fin && det != 0.0;
}

__device__ __forceinline__ double m3_norm(const double *p) { return sqrt((p[8] * p[8] + p[9] * p[9]) + p[10] * p[10]); }

// the rule's pixel test: q_2 > 0 and the nearest pixel inside W x H (NaN fails); iu, iv = that pixel
__device__ __forceinline__ bool dep_pixel(double q0, double q1, double q2, int W, int H, int &iu, int &iv)
{
    const double us = q0 / q2 + 0.5, vs = q1 / q2 + 0.5;
    const bool ok = q2 > 0.0 && us >= 0.0 && us < (double)W && vs >= 0.0 && vs < (double)H;
    iu = ok ? (int)us : 0;
    iv = ok ? (int)vs : 0;
    return ok;
}

// row r of the filter's camera table from frame fr's camera: a frame outside [0, n_frames) or an unknown camera is not known
__device__ __forceinline__ void fuse_camera_row(const double *P, int n_frames, int fr, double *c)
{
    double adj[9], det = 0.0, sg = 0.0, n3 = 0.0;
#pragma unroll
    for (int k = 0; k < 9; k++) adj[k] = 0.0;
    bool ok = fr >= 0 && fr < n_frames;
    if (ok) {
        const double *p = P + (size_t)fr * 12;
        ok = dep_camera(p, adj, det);
        sg = det > 0.0 ? 1.0 : -1.0;
        n3 = m3_norm(p);
    }
#pragma unroll
    for (int k = 0; k < 9; k++) c[k] = adj[k];
    c[9] = det; c[10] = sg; c[11] = n3; c[12] = ok ? 1.0 : 0.0; c[13] = 0.0; c[14] = 0.0; c[15] = 0.0;
}

// X of pixel (u, v) of a map at depth z; c = the map's row of the camera table, p = its camera
__device__ __forceinline__ void fuse_point(const double *c, const double *p, int u, int v, double z, double &X0, double &X1, double &X2)
{
    const double w = (c[10] * c[11]) * z;
    const double t0 = w * (double)u - p[3], t1 = w * (double)v - p[7], t2 = w - p[11];
    X0 = ((c[0] * t0 + c[1] * t1) + c[2] * t2) / c[9];
    X1 = ((c[3] * t0 + c[4] * t1) + c[5] * t2) / c[9];
    X2 = ((c[6] * t0 + c[7] * t1) + c[8] * t2) / c[9];
}
