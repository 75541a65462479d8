// pgx_trackgraph.h -- what every consumer of the track graph shares (k_triangulate.hip, k_bundle.hip, k_register.hip, k_consensus.hip,
// k_denseviews.hip): the read-only view of the graph and the keypoints, its validation and walking on the device, the lock-free
// union-find (k_tracks.hip, k_meshclean.hip), the cameras, and the workspace carver of the launchers.  The lane-group and
// workgroup reductions and the workgroup scans that stood here are pgx_block.h's, which this header brings along with
// pgx_hoststage.h and pgx_ransac.h (the sampler and the keys of the RANSAC stages among its consumers): a file that wants the
// primitives alone includes pgx_block.h.  Internal to libpgx.so; DESIGN.md sections 14a and 14i.
#pragma once

#include "pgx_internal.h"
#include "pgx_block.h"      // gsum, block_sums, block_excl_scan, block_scan_array, block_tally_add, pgx_clamp_count
#include "pgx_hoststage.h"   // WsCarver, the workspace carver of the launchers
#include "pgx_ransac.h"

#include <cmath>

// The shared inputs of a stage, embedded in its kernel-argument struct.
struct TrackView {
    const pgx_keypoint *kp;       // [F][stride] by slot
    const int32_t *frame_ids;     // [F] slot -> frame, nullptr = identity
    const int32_t *offsets;       // [n_tracks + 1]
    const int32_t *nodes;         // [node_cap][2] = (frame, keypoint)
    const int32_t *track_summary; // [0] = n_tracks
    int F, stride, n_frames, max_tracks;
    long long node_cap;           // entries of nodes (and of a per-node output) an offset may reach
    int32_t *inv;                 // workspace [n_frames] frame -> slot, -1 = none (build_slot_inverse)
};

#ifdef __HIPCC__

// ---- the graph --------------------------------------------------------------------------------------------------------

// nodes [o0, o0 + n) of track t; false (and n = 0) for malformed offsets
__device__ __forceinline__ bool track_range(const TrackView &tv, long long t, int &o0, int &n)
{
    o0 = tv.offsets[t];
    const int o1 = tv.offsets[t + 1];
    const bool bad = o0 < 0 || o1 < o0 || (long long)o1 > tv.node_cap;
    n = bad ? 0 : o1 - o0;
    return !bad;
}

// node (f, k) names a frame that a slot holds and a keypoint slot of it
__device__ __forceinline__ bool node_ok(const TrackView &tv, int f, int k)
{
    return !(f < 0 || f >= tv.n_frames || k < 0 || k >= tv.stride || tv.inv[f] < 0);
}

// keypoint of a node that is node_ok
__device__ __forceinline__ void node_keypoint(const TrackView &tv, int f, int k, double &u, double &v)
{
    const pgx_keypoint p = tv.kp[(size_t)tv.inv[f] * tv.stride + k];
    u = (double)p.x;
    v = (double)p.y;
}

// One workgroup, after inv[] = -1 and a barrier: the inverse of the slot -> frame map; a second slot naming a frame
// raises dup_bit.  The caller places the barrier behind it.
__device__ __forceinline__ void build_slot_inverse(const TrackView &tv, int *status, unsigned dup_bit)
{
    for (int s = threadIdx.x; s < tv.F; s += blockDim.x) {
        const int f = tv.frame_ids ? tv.frame_ids[s] : s;
        if (f < 0 || f >= tv.n_frames) continue;
        if (atomicCAS(&tv.inv[f], -1, s) != -1) atomicOr(status, (int)dup_bit);
    }
}

// tracks to process = clamp(n_tracks, 0, max_tracks); more than max_tracks raises cap_bit (one thread calls this)
__device__ __forceinline__ int clamp_tracks(const TrackView &tv, int *status, unsigned cap_bit)
{
    int nt = tv.track_summary[0];
    nt = nt < 0 ? 0 : nt;
    if (nt > tv.max_tracks) {
        atomicOr(status, (int)cap_bit);
        nt = tv.max_tracks;
    }
    return nt;
}

// Grid-stride loop over the tracks t < nt with G lanes per track (G a power of two <= 64): declares gid, ngroups, lane.
#define PGX_TRACK_LOOP(G, nt)                                                                \
    const long long gid = ((long long)blockIdx.x * blockDim.x + threadIdx.x) / (G);         \
    const long long ngroups = (long long)gridDim.x * blockDim.x / (G);                       \
    const int lane = threadIdx.x & ((G) - 1);                                                \
    for (long long t = gid; t < (nt); t += ngroups)

// ---- lock-free union-find with hashed priorities (k_tracks.hip: keypoints joined by matches; k_meshclean.hip: vertices joined
// by triangles).  The priority prio(x), a bijection on the ids so that there are no ties, is the graph's own (trk_prio, mcl_prio) --

__device__ __forceinline__ int trk_ld(const int32_t *p)
{
    // a plain load the compiler may not cache in a register across the loops below (no cache-bypass bits at this scope)
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT);
}
__device__ __forceinline__ void trk_st(int32_t *p, int v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT); }

// Root of x with intermediate pointer jumping.  Invariant: prio(parent[v]) < prio(v) unless v is a root (parent[v] == v), and
// parent[v] only ever moves to an ancestor of v.  A value read here may be STALE (another XCD's L2, this CU's L1): every
// earlier value of parent[v] is v itself or an ancestor, so a walk over stale values still descends in priority (it ends), and
// a stale read can only name a node that is no longer a root -- the caller's atomicCAS then fails and returns the truth.
__device__ __forceinline__ int trk_find(int32_t *parent, int x)
{
    int curr = trk_ld(parent + x);
    if (curr != x) {
        int prev = x, next;
        while (curr != (next = trk_ld(parent + curr))) {
            trk_st(parent + prev, next);
            prev = curr;
            curr = next;
        }
    }
    return curr;
}

// The trees of u and v become one: RANDOM linking -- of two roots the one with the larger hashed id hooks under the other, by an
// atomicCAS on a root only.  A CAS that fails returns the root's true parent: the walk goes on from the root above it.
template <class Prio> __device__ __forceinline__ void trk_hook(int32_t *parent, int u, int v, Prio prio)
{
    int ru = trk_find(parent, u), rv = trk_find(parent, v);
    while (ru != rv) {
        if (prio(ru) < prio(rv)) { const int t = ru; ru = rv; rv = t; }   // ru hooks under rv
        const int old = atomicCAS(parent + ru, ru, rv);
        if (old == ru) break;
        ru = trk_find(parent, old);   // ru was no root any more: go on from the root above its true parent
    }
}

// ---- cameras ----------------------------------------------------------------------------------------------------------

// R' = Exp(omega) R (Rodrigues); R, Ro row-major 3x3
__device__ __forceinline__ void rotate_left(const double *om, const double *R, double *Ro)
{
    const double th2 = om[0] * om[0] + om[1] * om[1] + om[2] * om[2];
    double A, B;
    if (th2 < 1e-8) {
        A = 1.0 - th2 / 6.0;
        B = 0.5 - th2 / 24.0;
    } else {
        const double th = sqrt(th2);
        A = sin(th) / th;
        B = (1.0 - cos(th)) / th2;
    }
    const double wx = om[0], wy = om[1], wz = om[2];
    // E = I + A [w]x + B [w]x^2, [w]x^2 = w w^T - th2 I
    double E[9];
    E[0] = 1.0 + B * (wx * wx - th2);
    E[1] = -A * wz + B * (wx * wy);
    E[2] = A * wy + B * (wx * wz);
    E[3] = A * wz + B * (wy * wx);
    E[4] = 1.0 + B * (wy * wy - th2);
    E[5] = -A * wx + B * (wy * wz);
    E[6] = -A * wy + B * (wz * wx);
    E[7] = A * wx + B * (wz * wy);
    E[8] = 1.0 + B * (wz * wz - th2);
#pragma unroll
    for (int r = 0; r < 3; r++)
#pragma unroll
        for (int c = 0; c < 3; c++) Ro[3 * r + c] = (E[3 * r] * R[c] + E[3 * r + 1] * R[3 + c]) + E[3 * r + 2] * R[6 + c];
}

// P = K [R | t] of r = (R row-major, t), K = (fx, fy, cx, cy); NaN rows when the camera is not known
__device__ __forceinline__ void camera_matrix(const double *K, const double (&r)[12], bool known, double *P)
{
    const double NaN = __builtin_nan("");
    // column j of [R | t]: (r[j], r[3 + j], r[6 + j]) for j < 3, (t0, t1, t2) for j = 3
    for (int j = 0; j < 4; j++) {
        const double c0 = j < 3 ? r[j] : r[9], c1 = j < 3 ? r[3 + j] : r[10], c2 = j < 3 ? r[6 + j] : r[11];
        P[j] = known ? K[0] * c0 + K[2] * c2 : NaN;
        P[4 + j] = known ? K[1] * c1 + K[3] * c2 : NaN;
        P[8 + j] = known ? c2 : NaN;
    }
}

#endif // __HIPCC__
