// pgx_stage_args.h -- the arguments of the stages behind the matchers, each as the struct its kernels take by value:
// triangulation, bundle adjustment, registration, consensus, verification, initial pair, depth maps, depth fuse, dense views, cloud merge, mesh, mesh clean.  The C ABI's
// two forms of a stage (pgx_api.hip) fill "the caller fills" by name and hand the struct to run_X; the launcher carves the
// workspace into the rest and launches.  The layout IS the kernarg layout: fields, order and types are the kernels' (the
// capitals in the shapes are constants of the stage's .hip file).  Internal to libpgx.so; DESIGN.md section 14h.
#pragma once

#include "pgx_trackgraph.h"

// ---- k_triangulate.hip (multi-view triangulation of tracks; pgx_triangulate_tracks_dev semantics, include/pgx.h) ----------
struct TriArgs {
    // the caller fills
    TrackView tv;                 // node_cap also bounds node_err
    const double *P;              // [n_frames][12]
    int refine_iters;
    double min_par, max_reproj;   // min_parallax_deg, max_reproj_px
    double *xyz, *quality;        // [max_tracks][3] each
    int32_t *flags;               // [max_tracks]
    double *node_err;             // [node_cap] or nullptr
    int32_t *summary;             // [8]
    // the launcher fills (workspace)
    double *cam;                  // [n_frames][CAM_STRIDE]
    int32_t *meta;                // [0] tracks to process
    int32_t *part;                // [grid][8] per-workgroup counters
    // the caller fills
    int *status;                  // PGX_ST_TRI_* bits
};
size_t pgx_triangulate_ws_bytes(const TriArgs &a);   // of a's caller-filled part
void pgx_launch_triangulate(hipStream_t s, TriArgs a, void *ws);

// ---- k_bundle.hip (bundle adjustment of cameras and track points; pgx_bundle_adjust_dev semantics, include/pgx.h) ---------
struct BaCtrl;   // k_bundle.hip's control block
struct BaArgs {
    // the caller fills
    TrackView tv;                // node_cap also bounds node_err
    const double *K, *Rt_in;     // [n_frames][4], [n_frames][12]
    const int32_t *fixed;        // [n_frames]
    const double *xyz_in;        // [max_tracks][3]
    const int32_t *track_flags;  // [max_tracks] or nullptr
    int max_iters;
    double huber, lambda0;       // huber_px
    double *Rt_out, *P_out, *xyz_out, *node_err, *trace;   // [n_frames][12] x2, [max_tracks][3], [node_cap] or nullptr, [max_iters + 1][2]
    int32_t *report;             // [8]
    int *status;                 // PGX_ST_BA_* bits
    // the launcher fills (workspace)
    BaCtrl *ctrl;
    int32_t *fstate, *free_frame, *cam_cnt, *csr_off; // [n_frames], [128] x3
    double *cams;                // [2][n_frames][12] ping-pong by ctrl->sel
    double *S, *rhs, *dc;        // [BA_LD][BA_LD], [BA_LD], [BA_LD]
    double *X;                   // [2][max_tracks][3]
    double *V, *g, *Vi;          // [max_tracks][6], [3], [6]
    double *tcost, *tdx, *tx;    // [max_tracks] each
    int32_t *part;               // [max_tracks]: used observations of a track that takes part, else 0
    double *nd;                  // [node_cap][BA_ND]
    int32_t *ncf;                // [node_cap]: free number, -1 used in a fixed frame, -2 unused
    int32_t *csr_node, *csr_track;  // [node_cap]
};
size_t pgx_bundle_ws_bytes(const BaArgs &a);
void pgx_launch_bundle(hipStream_t s, BaArgs a, void *ws);

// ---- k_register.hip (frame registration by P3P RANSAC; pgx_register_frames_dev semantics, include/pgx.h) ------------------
struct RegArgs {
    // the caller fills (nblk: the launcher, derived from n_samples)
    TrackView tv;                // node_cap also bounds node_inlier
    const double *K, *Rt_in;     // [n_frames][4], [n_frames][12]
    const int32_t *reg;          // [n_frames]
    const double *xyz;           // [max_tracks][3]
    const int32_t *track_flags;  // [max_tracks] or nullptr
    int n_samples, min_inliers, refine_iters, nblk;
    double inlier_px;
    uint64_t seed;
    double *Rt_out, *P_out, *frame_err;          // [n_frames][12] x2, [n_frames][2]
    int32_t *frame_stats, *node_inlier, *report; // [n_frames][4], [node_cap] or nullptr, [8]
    int *status;                 // PGX_ST_REG_* bits
    // the launcher fills (workspace)
    int32_t *ctrl;               // [0] tracks to process, [1] targets
    int32_t *tnum, *tframe, *cnt, *coff, *nlist;  // [n_frames] each
    int32_t *cf;                 // [node_cap]: target number of a correspondence node, else -1
    int32_t *corr_node;          // [node_cap]
    double *cx, *cy, *cz, *cu, *cv;  // [node_cap] each, by position coff[target] + j
    double *S;                   // [n_frames][4]
    double *win;                 // [n_frames][16]: the winner's R, t_S
    int32_t *winfo;              // [n_frames][2]: winning sample or -1, flags
    double *hyp;                 // [n_frames][chunk][4][REG_HD]
    unsigned long long *best;    // [n_frames][nblk]
};
size_t pgx_register_ws_bytes(const RegArgs &a);
void pgx_launch_register(hipStream_t s, RegArgs a, void *ws);

// ---- k_consensus.hip (track consensus; pgx_track_consensus_dev semantics, include/pgx.h) ----------------------------------
struct CnsArgs {
    // the caller fills (min_len: the launcher clamps it to >= 1)
    TrackView tv;                 // node_cap also bounds nodes_out
    const double *P;              // [n_frames][12]
    double inlier_px, cos2;       // cos2 = the square of the cosine of min_parallax_deg
    int min_inliers, min_len, max_hyp;
    uint64_t seed;
    // [max_tracks + 1], [node_cap][2], [8], [max_tracks] x2, [max_tracks][4], [F][stride] or nullptr, [8]
    int32_t *off_out, *nodes_out, *summary_out, *map, *flags_out, *stats, *track_of, *report;
    double *xyz_out;              // [max_tracks][3]
    // the launcher fills (workspace)
    double *cam;                  // [n_frames][CNS_CAM]
    double *rays;                 // [node_cap][CNS_RAY]: track t's known observations from its first node on
    double *xyz;                  // [max_tracks][3] by old index
    int32_t *kept;                // [max_tracks] nodes the track keeps, 0 = the track is removed
    int32_t *bsum;                // [scan blocks][2] tracks and nodes, exclusive after k_cns_scan_sums
    int8_t *keep;                 // [node_cap]
    int32_t *meta;                // [0] tracks to process, [CT_*] counters
    // the caller fills
    int *status;                  // PGX_ST_CNS_* bits
};
size_t pgx_consensus_ws_bytes(const CnsArgs &a);
// ctx: the profiling groups consensus_frames / _score / _scan / _write
void pgx_launch_consensus(pgx_ctx *ctx, hipStream_t s, CnsArgs a, void *ws);

// ---- k_verify.hip (two-view verification by epipolar RANSAC; pgx_verify_pairs_dev semantics, include/pgx.h) ---------------
struct VerArgs {
    // the caller fills, every pointer the first of the launch's pairs' rows (nblk: the launcher, derived from n_samples)
    const pgx_keypoint *kp;      // [F][stride] by slot
    const pgx_pair *matches;     // [M][stride]
    const int32_t *counts, *pairlist;   // [F], [M][2]
    int stride, max_dist, n_samples, min_inliers, refit_iters, nblk;
    double inlier_px;
    uint64_t seed;
    pgx_pair *out;               // [M][stride]
    double *F;                   // [M][9]
    float *F32;                  // [M][9] or nullptr
    int32_t *stats, *inlier;     // [M][8], [M][stride] or nullptr
    double *sample_F;            // [M][n_samples][9] or nullptr
    int32_t *sample_count;       // [M][n_samples] or nullptr
    // the launcher fills (workspace, per pair of the chunk)
    int32_t *ncand;              // [M]
    int32_t *cpos;               // [M][stride]: candidate position of an entry, -1 = not a candidate
    double *x, *y, *u, *v;       // [M][stride] by candidate position
    double *hyp;                 // [M][chunk][9]
    unsigned long long *best;    // [M][nblk]: the scoring workgroups' keys of one chunk
    int32_t *nvalid;             // [M][nblk]: their valid samples
    unsigned long long *run;     // [M]: best key so far
    int32_t *run_valid;          // [M]: valid samples so far
    double *win;                 // [M][9]: the F of run
    int32_t *winfo;              // [M][8]: d_stats' row
};
// samples per chunk for a workspace of M pairs (a multiple of 256), and the bytes of that workspace: not less for more pairs
int pgx_verify_chunk(int M, int n_samples);
size_t pgx_verify_ws_bytes(int M, int stride, int n_samples, int chunk);
// M <= 65535 pairs that share the workspace.  chunk: the workspace's
void pgx_launch_verify(hipStream_t s, VerArgs a, int M, int chunk, void *ws);
// d_report from the d_stats rows of all M pairs of a call
void pgx_launch_verify_summary(hipStream_t s, const int32_t *d_stats, int M, int32_t *d_report);

// ---- k_initpair.hip (relative pose per image pair and the choice of the initial pair; pgx_init_pair_dev semantics) --------
struct InitArgs {
    // the caller fills, all M pairs of a call (split: the launcher, derived from stride)
    const pgx_keypoint *kp;      // [nslots][stride] by slot
    const pgx_pair *matches;     // [M][stride]
    const int32_t *counts, *pairlist, *frame_ids;   // [nslots], [M][2], [nslots] or nullptr
    const double *F, *K;         // [M][9], [n_frames][4]
    int M, nslots, stride, n_frames, max_dist, min_points, split;
    double cos2, min_front_frac; // cos2 = the square of the cosine of min_angle_deg
    double *Rt_pair, *sigma, *cand_Rt, *Rt_out, *P_out;   // [M][12], [M] or nullptr, [M][48] or nullptr, [n_frames][12] x2
    int32_t *pair_stats, *fixed_out, *register_out, *report;   // [M][8], [n_frames] x2, [8]
    // the launcher fills (workspace)
    double *wd;    // [M][INIT_WS_D]
    int32_t *wi;   // [M][INIT_WS_I]
};
size_t pgx_init_pair_ws_bytes(const InitArgs &a);
void pgx_launch_init_pair(hipStream_t s, InitArgs a, void *ws);

// ---- k_depth.hip (census plane-sweep depth maps and the cross-view filter; pgx_depth_maps_dev and pgx_depth_fuse_dev ------
// semantics, include/pgx.h).  ctx: the profiling groups depth_census / depth_plan / depth_sweep / depth_fuse
struct DepArgs {
    // the caller fills
    const float *gray;            // [F][H][W]
    int F, W, H;
    const int32_t *frame_ids;     // [F] or nullptr
    int n_frames;
    const double *P;              // [n_frames][12]
    const int32_t *views;         // [R][1 + S]
    int R, S;
    const double *range;          // [R][2]
    int D, min_views, max_cost;
    int32_t *kq8;                 // [R][H][W], as depth and flags
    double *depth;
    int32_t *cost;                // [R][H][W] or nullptr
    int32_t *flags;
    double *warp_out, *planes_out; // [R][S][12], [R][D], or nullptr
    int32_t *summary;             // [8]
    // the launcher fills (workspace)
    uint2 *census;                // [F][H][W]
    double *warp;                 // [R][S][12]: A row-major, then b
    int32_t *slot;                // [R][1 + S]: the slot of the reference (-1: NOCAMERA) and of every valid source (-1: none)
    double *planes;               // [R][D]: w_k
};
size_t pgx_depth_ws_bytes(const DepArgs &a);
void pgx_launch_depth_maps(pgx_ctx *ctx, hipStream_t s, DepArgs a, int agg_radius, void *ws);

struct FuseArgs {
    // the caller fills
    const double *depth;          // [R][H][W]
    const int32_t *views;         // [R][1 + S]
    int R, S, W, H, n_frames;
    const double *P;              // [n_frames][12]
    double rel_tol;
    int min_agree, max_points;
    double *xyz;                  // [max_points][3]
    int32_t *src;                 // [max_points][2]
    int32_t *agree;               // [R][H][W] or nullptr
    int32_t *summary;             // [4]
    // the launcher fills (workspace, derived)
    double *cam;                  // [R][FUSE_CAM]
    int32_t *rowof;               // [R][S]: the map a source is compared with, -1 = none
    unsigned char *keep;          // [nb * 256]
    int32_t *bsum, *boff;         // [nb]: kept pixels per block, their exclusive scan
    int nb;                       // blocks of 256 pixels
    // the caller fills
    int *status;                  // more than max_points kept pixels: PGX_ST_DEP_CAP
};
size_t pgx_depth_fuse_ws_bytes(const FuseArgs &a);
void pgx_launch_depth_fuse(pgx_ctx *ctx, hipStream_t s, FuseArgs a, void *ws);

// ---- k_denseviews.hip (sources and depth range per reference from the sparse model; pgx_dense_views_dev semantics) ---------
// ctx: the profiling groups dense_views_nodes / _pairs / _select
struct DvwArgs {
    // the caller fills
    TrackView tv;                 // the graph alone: no keypoints, no slots; node_cap = max_nodes
    const double *xyz;            // [max_tracks][3]
    const int32_t *track_flags;   // [max_tracks] or nullptr
    const double *P;              // [n_frames][12]
    const int32_t *refs;          // [R] or nullptr
    int R, S, min_shared, min_points, q_near_pm, q_far_pm;
    double cmin2, cmax2, grow;    // the squares of the cosines of min_angle_deg and max_angle_deg
    int32_t *views;               // [R][1 + S]
    double *range;                // [R][2]
    int32_t *pair_counts, *ref_stats, *report;   // [R][n_frames][2] or nullptr, [R][4], [8]
    // the launcher fills (workspace)
    unsigned long long *cells;    // [R][n_frames]: shared | good << 32, counted in the first row that names a frame
    double *cam;                  // [n_frames][DVW_CAM]
    double *zb;                   // [node_cap]: the depths of the used nodes, frame f's at fbase[f] .. fbase[f + 1]
    int32_t *rowof;               // [n_frames]: the first row of refs that names the frame, or DVW_NOROW
    int32_t *fcnt, *fbase, *fcur; // [n_frames], [n_frames + 1], [n_frames]: used nodes, bucket starts, scatter cursors
    int32_t *meta;                // [0] tracks to process
    // the caller fills
    int *status;                  // PGX_ST_DVW_* bits
};
size_t pgx_dense_views_ws_bytes(const DvwArgs &a);
void pgx_launch_dense_views(pgx_ctx *ctx, hipStream_t s, DvwArgs a, void *ws);

// ---- k_cloud.hip (the fused point list merged into one cloud with normals and colour; pgx_cloud_merge_dev semantics) -------
// ctx: the profiling groups cloud_plan / cloud_normals / cloud_points / cloud_rank / cloud_accum / cloud_final
struct CloudArgs {
    // the caller fills
    const double *xyz;            // [max_in][3]
    const int32_t *src;           // [max_in][2] = (r, v W + u)
    const int32_t *count;         // [0] = the entries of the list, or nullptr: max_in
    int max_in;
    const double *depth;          // [R][H][W]
    const int32_t *views;         // [R][1 + S]: column 0 alone is read
    int R, S, W, H, n_frames;
    const double *P;              // [n_frames][12]
    const uint32_t *rgba8;        // [F][H][W] or nullptr
    int F;
    const int32_t *frame_ids;     // [F] or nullptr
    double cell, ox, oy, oz, disc_tol;
    int normal_step, min_support, max_points;
    double *out_xyz;              // [max_points][3]
    float *out_normal;            // [max_points][3]
    uint32_t *out_rgba8;          // [max_points]
    int32_t *out_info;            // [max_points][4] = (cnt, nn, nc, first)
    int32_t *pt_normal;           // [max_in][3] or nullptr
    int32_t *cell_of;             // [max_in] or nullptr
    int32_t *report;              // [8]
    // the launcher fills (workspace, derived)
    int lg_table;                 // the table has 1 << lg_table entries
    unsigned long long *keys;     // [table]: the cell's key, CLD_EMPTY = none
    int32_t *tfirst, *tcnt, *tout; // [table]: the smallest point of the cell, its points, its output index (-2: dropped)
    double *cam;                  // [R][FUSE_CAM]: the filter's camera table
    int32_t *cslot;               // [R]: the slot that shows the map's frame, -1 = none
    int32_t *slot;                // [max_in]: the point's table entry, -1 = not used
    unsigned long long *rec;      // [max_in][2]: p (3 x 16 bits), flags, a colour byte | q (3 x 16 bits), two colour bytes
    int32_t *bsum, *boff;         // [nb]: owners per block of 256 points, their exclusive scan
    int32_t *oslot;               // [max_points]: the table entry of an output cell
    unsigned long long *acc;      // [max_points][CLD_ACC]: the sums of p, q and colour, nn | nc << 32
    int32_t *meta;                // [0] n, [1] used, [2] normals, [3] colours, [4] cells, [5] cells kept
    int nb;                       // blocks of 256 points
    // the caller fills
    int *status;                  // more than max_points cells kept: PGX_ST_CLD_CAP
};
size_t pgx_cloud_ws_bytes(const CloudArgs &a);
void pgx_launch_cloud_merge(pgx_ctx *ctx, hipStream_t s, CloudArgs a, void *ws);

// ---- k_mesh.hip (a triangle mesh from the depth maps: a TSDF on a hashed grid and surface nets; pgx_mesh_dev semantics) ---
// ctx: the profiling groups mesh_plan / mesh_seed / mesh_dilate / mesh_tsdf / mesh_cubes / mesh_rank / mesh_vertices / mesh_tris
struct MeshArgs {
    // the caller fills
    const double *xyz;            // [max_in][3]
    const int32_t *src;           // [max_in][2] = (r, v W + u)
    const int32_t *count;         // [0] = the entries of the list, or nullptr: max_in
    int max_in;
    const double *depth;          // [R][H][W]
    const int32_t *views;         // [R][1 + S]: column 0 alone is read
    int R, S, W, H, n_frames;
    const double *P;              // [n_frames][12]
    const int32_t *agree;         // [R][H][W] or nullptr
    int min_agree;
    const uint32_t *rgba8;        // [F][H][W] or nullptr
    int F;
    const int32_t *frame_ids;     // [F] or nullptr
    double cell, ox, oy, oz;
    int band, trunc_cells, min_weight, max_voxels, max_vertices, max_tris;
    double *out_xyz;              // [max_vertices][3]
    float *out_normal;            // [max_vertices][3]
    uint32_t *out_rgba8;          // [max_vertices]
    int32_t *out_info;            // [max_vertices][4] = (c_0, c_1, c_2, mask | k << 8)
    int32_t *out_tri;             // [max_tris][3]
    int32_t *report;              // [8]
    // the launcher fills (workspace, derived)
    int lg_table;                 // the table has 1 << lg_table entries
    unsigned long long *keys;     // [table]: the node's key, MSH_EMPTY = none
    unsigned long long *ord;      // [table]: ord(c), MSH_NOORD = none yet
    int32_t *sfirst;              // [table]: the first point whose own cell is this node, MSH_NOSEED = none
    int32_t *wst;                 // [table][2]: w, st
    int32_t *col;                 // [table][4]: nc, sc
    int32_t *cflag;               // [table]: of the cube whose low node this is: mask | complete << 8 | active << 9
    int32_t *vidx, *qidx;         // [table]: the cube's vertex, the first quad of the node's edges
    unsigned char *nflag;         // [table]: valid | inside << 1
    unsigned char *qflag;         // [table]: bit a = the edge along axis a has a quad
    double *cam;                  // [R][FUSE_CAM]: the filter's camera table
    int32_t *cslot;               // [R]: the slot that shows the map's frame, -1 = none
    int32_t *slot;                // [max_in]: the table entry of the point's own cell's node, -1 = not used
    unsigned long long *bsum, *boff;   // [nb]: vertices | quads << 32 owned per block of 256 points, their exclusive scan
    int32_t *meta;                // [0] n, [1] used, [2] seed cells, [3] voxels, [4] valid voxels, [5] vertices, [6] quads
    int nb;                       // blocks of 256 points
    // the caller fills
    int *status;                  // a capacity exceeded: PGX_ST_MSH_CAP
};
size_t pgx_mesh_ws_bytes(const MeshArgs &a);
void pgx_launch_mesh(pgx_ctx *ctx, hipStream_t s, MeshArgs a, void *ws);

// ---- k_meshclean.hip (the mesh cleaned: small components dropped, Taubin smoothing, normals again; pgx_mesh_clean_dev semantics) ---
// ctx: the profiling groups mclean_init / mclean_union / mclean_count / mclean_rank / mclean_emit / mclean_rows / mclean_smooth /
// mclean_normals
struct MeshCleanArgs {
    // the caller fills
    const double *xyz;            // [max_vertices][3]
    const float *normal;          // [max_vertices][3]
    const uint32_t *rgba8;        // [max_vertices]
    const int32_t *info;          // [max_vertices][4]
    const int32_t *tri;           // [max_tris][3]
    const int32_t *counts;        // [5] = the vertices, [6] = the triangles (pgx_mesh_dev's report), or nullptr: the capacities
    int max_vertices, max_tris;
    double cell, ox, oy, oz, lambda, mu;
    int min_tris, min_frac_pm, iters, max_out_vertices, max_out_tris;
    double *out_xyz;              // [max_out_vertices][3]
    float *out_normal;            // [max_out_vertices][3]
    uint32_t *out_rgba8;          // [max_out_vertices]
    int32_t *out_info;            // [max_out_vertices][4]
    int32_t *out_tri;             // [max_out_tris][3]
    int32_t *vertex_map;          // [max_vertices] or nullptr
    int32_t *comp;                // [max_vertices] or nullptr
    int32_t *report;              // [8]
    // the launcher fills (workspace, derived)
    int32_t *parent;              // [max_vertices]: the union-find
    int32_t *root;                // [max_vertices]: the root of a vertex of a used triangle, -1 otherwise
    int32_t *rep;                 // [max_vertices]: at a root, the smallest vertex of its component: its name
    int32_t *tcnt;                // [max_vertices]: at a root, the used triangles of its component
    int32_t *deg;                 // [max_vertices]: the used triangles that hold the vertex
    int32_t *vnew;                // [max_vertices]: the new index, -1, -2 as vertex_map
    int32_t *roff;                // [max_vertices]: where the row of a kept vertex begins
    int32_t *cursor;              // [max_vertices]: the entries of the row filled so far
    long long *qa, *qb;           // [max_vertices][3] each: the fixed-point positions, the two buffers of the half-steps
    unsigned char *vvalid;        // [max_vertices]
    unsigned char *tused;         // [max_tris]
    int32_t *tnew;                // [max_tris]: the new index of a kept triangle, -1 otherwise
    int32_t *rows;                // [3 max_tris]: per kept vertex the kept triangles that hold it, in no order (iters > 0)
    unsigned long long *tnrm;     // [max_tris]: m of rule 4, 16 bits a component; MCL_NONRM = the triangle contributes nothing
    unsigned long long *bsum, *boff;   // [nb]: kept vertices | kept triangles << 32 per block of 256 indices, their exclusive scan
    unsigned long long *rsum, *rbase;  // [nb]: row entries per block, their exclusive scan
    int32_t *meta;                // [0] nv, [1] nt, [2] used, [3] components, [4] kept, [5] vertices out, [6] triangles out, [7] big
    int nb;                       // blocks of 256 indices of max(max_vertices, max_tris)
    // the caller fills
    int *status;                  // an output capacity exceeded: PGX_ST_MCL_CAP
};
size_t pgx_mesh_clean_ws_bytes(const MeshCleanArgs &a);
void pgx_launch_mesh_clean(pgx_ctx *ctx, hipStream_t s, MeshCleanArgs a, void *ws);

// ---- k_meshdecimate.hip (the mesh decimated: adaptive vertex clustering over grid blocks; pgx_mesh_decimate_dev semantics) ---
// ctx: the profiling groups mdec_init / mdec_tris / mdec_levels / mdec_clusters / mdec_dedup / mdec_rank / mdec_emit / mdec_normals
struct MeshDecimateArgs {
    // the caller fills
    const double *xyz;            // [max_vertices][3]
    const float *normal;          // [max_vertices][3]: of the layout, not read
    const uint32_t *rgba8;        // [max_vertices]
    const int32_t *info;          // [max_vertices][4]: of the layout, not read
    const int32_t *tri;           // [max_tris][3]
    const int32_t *counts;        // [5] = the vertices, [6] = the triangles (a mesh stage's report), or nullptr: the capacities
    int max_vertices, max_tris;
    double cell, ox, oy, oz;
    int lmin, lmax, flat_q, max_out_vertices, max_out_tris;
    double *out_xyz;              // [max_out_vertices][3]
    float *out_normal;            // [max_out_vertices][3]
    uint32_t *out_rgba8;          // [max_out_vertices]
    int32_t *out_info;            // [max_out_vertices][4] = (name, L, n, 0)
    int32_t *out_tri;             // [max_out_tris][3]
    int32_t *vertex_map;          // [max_vertices] or nullptr
    int32_t *level;               // [max_vertices] or nullptr
    int32_t *report;              // [8]
    // the launcher fills (workspace, derived)
    int lg_vcap, lg_tcap;         // the carved tables have 1 << lg_vcap and 1 << lg_tcap entries; the device uses 1 << meta[2], 1 << meta[3] of them
    long long *q;                 // [max_vertices][3]: the fixed-point positions
    unsigned char *member;        // [max_vertices]: the vertex is in a used triangle
    unsigned char *lev;           // [max_vertices]: L(v) so far
    int32_t *vslot;               // [max_vertices]: the entry of a member's cluster
    unsigned long long *fkey[2];  // [1 << lg_vcap] each: the blocks of one level (two tables, a level and the one above), MDC_EMPTY = none
    unsigned long long *fsum[2];  // [1 << lg_vcap][4] each: S_0, S_1, S_2, N of the block
    unsigned long long *ckey;     // [1 << lg_vcap]: the clusters' keys
    int32_t *cname;               // [..]: the cluster's smallest member
    int32_t *cn;                  // [..]: its members
    int32_t *cnew;                // [..]: its output index, -1 = in no kept triangle (then cused is 0)
    unsigned char *cused;         // [..]: a kept triangle holds it
    unsigned long long *cs;       // [..][3]: the sums of q - org; from k_mdc_emit on Q
    unsigned long long *csc;      // [..][4]: the sums of the colour bytes; from k_mdc_emit on [0..2] the sums of the triangles' m
    int32_t *trot;                // [max_tris][3]: the rotated triple of cluster entries, [0] = -1: not used or degenerate
    unsigned long long *tm;       // [max_tris]: m of rule 2, 16 bits a component
    int32_t *tslot;               // [max_tris]: the triangle's entry of the table of triples
    int32_t *towner;              // [1 << lg_tcap]: the smallest triangle of the entry's triple, -1 = none
    int32_t *tnew;                // [max_tris]: the new index of a kept triangle, -1 otherwise
    unsigned long long *bsum, *boff;   // [nb]: output vertices | kept triangles << 32 per block of 256 indices, their exclusive scan
    int32_t *meta;                // [16]: nv, nt, lg of the vertex tables, lg of the triple table, used, clusters, non-degenerate, vertices out, triangles out
    int nb;                       // blocks of 256 indices of max(max_vertices, max_tris)
    // the caller fills
    int *status;                  // an output capacity exceeded: PGX_ST_MDC_CAP
};
size_t pgx_mesh_decimate_ws_bytes(const MeshDecimateArgs &a);
void pgx_launch_mesh_decimate(pgx_ctx *ctx, hipStream_t s, MeshDecimateArgs a, void *ws);
