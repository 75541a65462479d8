// pgx_internal.h -- shared between the HIP translation units of libpgx.so (gfx950 only).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <map>
#include <mutex>
#include <string>
#include <type_traits>
#include <utility>
#include <vector>

#include "../../include/pgx.h"

// status bits set by kernels (device word 0), decoded by pgx_check_status
#define PGX_ST_OOB_SOURCE 1u
#define PGX_ST_RAW_CAP    2u
#define PGX_ST_KP_CAP     4u
#define PGX_ST_EMPTY_SET  8u
#define PGX_ST_INTERNAL   16u  /* a device loop made no progress (a bug, never an input property) */
#define PGX_ST_BADARG     32u  /* guided matching: a used keypoint coordinate outside [-2^20, 2^20) */
#define PGX_ST_DUP_FRAME  64u  /* pgx_tracks_split_dev: two slots of d_frame_ids name the same frame */
#define PGX_ST_TRI_CAP    128u /* pgx_triangulate_tracks_dev: n_tracks > max_tracks */
#define PGX_ST_TRI_NODE   256u /* pgx_triangulate_tracks_dev: a node outside the frames / keypoint slots, or malformed offsets */
#define PGX_ST_TRI_DUP    512u /* pgx_triangulate_tracks_dev: two slots of d_frame_ids name the same frame */
#define PGX_ST_BA_CAP     1024u  /* pgx_bundle_adjust_dev: n_tracks > max_tracks */
#define PGX_ST_BA_FREE    2048u  /* pgx_bundle_adjust_dev: more than 128 free frames */
#define PGX_ST_BA_NODE    4096u  /* pgx_bundle_adjust_dev: a bad node, malformed offsets, or two nodes of a track in one frame */
#define PGX_ST_BA_DUP     8192u  /* pgx_bundle_adjust_dev: two slots of d_frame_ids name the same frame */
#define PGX_ST_BA_ROT     16384u /* pgx_bundle_adjust_dev: a finite R that is not a rotation */
#define PGX_ST_BA_NOFIX   32768u /* pgx_bundle_adjust_dev: no known frame is fixed */
#define PGX_ST_REG_CAP    65536u  /* pgx_register_frames_dev: n_tracks > max_tracks */
#define PGX_ST_REG_NODE   131072u /* pgx_register_frames_dev: a node outside the frames / keypoint slots, or malformed offsets */
#define PGX_ST_REG_DUP    262144u /* pgx_register_frames_dev: two slots of d_frame_ids name the same frame */
#define PGX_ST_REG_TWICE  524288u /* pgx_register_frames_dev: a track with two nodes in one target frame */
#define PGX_ST_CNS_CAP    1048576u /* pgx_track_consensus_dev: n_tracks > max_tracks */
#define PGX_ST_CNS_NODE   2097152u /* pgx_track_consensus_dev: a node outside the frames / keypoint slots, or malformed offsets */
#define PGX_ST_CNS_DUP    4194304u /* pgx_track_consensus_dev: two slots of d_frame_ids name the same frame */
#define PGX_ST_VOC_FEW    8388608u  /* pgx_vocab_train_dev: fewer valid descriptors than words */
#define PGX_ST_SEL_CAP    16777216u /* pgx_select_pairs_dev: more than max_pairs pairs selected */
#define PGX_ST_DEP_CAP    33554432u /* pgx_depth_fuse_dev: more than max_points pixels kept */
#define PGX_ST_DVW_CAP    67108864u  /* pgx_dense_views_dev: n_tracks > max_tracks */
#define PGX_ST_DVW_NODE   134217728u /* pgx_dense_views_dev: a node of a used track outside the frames, or malformed offsets */
#define PGX_ST_CLD_CAP    268435456u /* pgx_cloud_merge_dev: more than max_points cells kept */
#define PGX_ST_MSH_CAP    536870912u /* pgx_mesh_dev: more than max_voxels voxels, max_vertices vertices or max_tris triangles */
#define PGX_ST_MCL_CAP    1073741824u /* pgx_mesh_clean_dev: more than max_out_vertices vertices or max_out_tris triangles kept */
/* bit 31, the last one: the word is an int on the device and in decode_status, where `bits & 2147483648u` converts it to unsigned */
#define PGX_ST_MDC_CAP    2147483648u /* pgx_mesh_decimate_dev: more than max_out_vertices vertices or max_out_tris triangles kept */

// key = (distance << PGX_IDX_BITS) | index ; limits: index < 2^20, distance < 2^12
#define PGX_IDX_BITS 20
#define PGX_IDX_MASK ((1u << PGX_IDX_BITS) - 1u)
#define PGX_KEY_NONE 0xFFFFFFFFu
// d_status layout (ints): [0] sticky error bits, [4..4+2*PGX_MAX_WIDE_ROUNDS) u64 evaluation counters per wide round
#define PGX_MAX_WIDE_ROUNDS 8
// ... and [PGX_DBG_OFF .. +16) eight u64 diagnostic counters of the match tail (pgx_debug_counters)
#define PGX_DBG_OFF 32
// residual size (rows and columns) from which one workgroup finishes an image pair out of LDS
#define PGX_TAIL_MAX 2048
// ... and the limit when the tail workgroup has to fill its distance cache itself (descriptors staged in LDS)
#define PGX_TAIL_FILL_MAX 1024
// chunks of at least this many image pairs run in order on one stream; smaller ones through the three-stream pipeline
#define PGX_PIPELINE_BELOW 1024

struct DevBuf {
    void *p = nullptr;
    size_t cap = 0;
    hipError_t ensure(size_t bytes)
    {
        if (bytes <= cap) return hipSuccess;
        if (p) { hipError_t e = hipFree(p); p = nullptr; cap = 0; if (e != hipSuccess) return e; }
        size_t want = bytes + bytes / 4 + 256;
        hipError_t e = hipMalloc(&p, want);
        if (e == hipSuccess) cap = want;
        return e;
    }
    void release() { if (p) (void)hipFree(p); p = nullptr; cap = 0; }
    template <class T> T *as() const { return reinterpret_cast<T *>(p); }
};

// pinned host staging (hipHostMalloc), grown on demand
struct PinBuf {
    void *p = nullptr;
    size_t cap = 0;
    hipError_t ensure(size_t bytes)
    {
        if (bytes <= cap) return hipSuccess;
        if (p) { (void)hipHostFree(p); p = nullptr; cap = 0; }
        const size_t want = bytes + bytes / 4 + 4096;
        hipError_t e = hipHostMalloc(&p, want, hipHostMallocDefault);
        if (e == hipSuccess) cap = want;
        return e;
    }
    void release() { if (p) (void)hipHostFree(p); p = nullptr; cap = 0; }
    template <class T> T *as() const { return reinterpret_cast<T *>(p); }
};

struct ProfEntry {
    std::vector<std::pair<hipEvent_t, hipEvent_t>> pending;
    int launches = 0;
    double total_ms = 0.0;
};

struct pgx_ctx {
    int device = 0;
    hipStream_t own_stream = nullptr;
    hipStream_t stream = nullptr;
    std::mutex mu;
    std::string err;     // text of the last failing call of any thread (written through pgx_note_error, under err_mu)
    std::mutex err_mu;

    // configuration
    float threshold = 0.f;
    int radius = 0;
    bool params_set = false;
    int P = 0, words = 0;
    bool pairs_set = false;
    DevBuf d_pairs;
    DevBuf d_plan; // P == 256 only: the table's row-sorted sample plan (pgx_brief_plan.h), rebuilt with every table
    // steered BRIEF (pgx_set_brief_steering; off by default and after every pgx_set_brief_pairs): B turned tables, their
    // sample plans when P == 256 (B x PGX_PLAN_WORDS), the B direction vectors and the disc radius of the orientation pass
    bool steer_on = false;
    int steer_B = 0, steer_R = 0;
    DevBuf d_steer_pairs, d_steer_plans, d_steer_dirs;
    // scale pyramid (pgx_set_pyramid; off = 1 level): levels and the 16.16 step between them
    int pyr_levels = 1, pyr_step = 0;
    int mapW = 0, mapH = 0;
    bool map_set = false;
    DevBuf d_map;
    // the map's gather plan, rebuilt behind every map that is installed and released when the map is cleared: W * H source
    // offsets (4 B/px beside the map's 8), then one word "some entry lies outside the image" (gather_flag)
    DevBuf d_gather;
    uint32_t *gather_flag() const { return d_gather.as<uint32_t>() + (size_t)mapW * mapH; }
    const void *fuse_rgba = nullptr; // enqueue_detect_bins -> its level-0 enqueue_from_gray: the source frames (one call)
    int raw_cap = 1 << 17;
    int kp_cap = 1 << PGX_IDX_BITS; // soft survivor limit of the fused path (pgx_set_capacity); default: none
    // image pairs per matcher workspace chunk (pgx_set_match_chunk).  The per-pair finish is one workgroup per image pair, and
    // the pairs of a sequence differ 3:1 in how long they take: the more of them one launch holds, the better the CUs are
    // balanced (stand-alone finish of the bench job's 2016 pairs: 2.15 ms at 256 pairs per chunk, 1.70 at 512, 1.24 in one
    // chunk; whole matcher 6.58 / 6.43 / 6.00 ms).  4.4 MiB of workspace per pair (+ 25 % slack of DevBuf::ensure): 11 GB at the default.
    int match_chunk = 2048;
    int src8 = 0; // pgx_set_source_format: 1 = the rgba arguments are 8-bit RGBA

    // status words: [0] sticky error bits
    int *d_status = nullptr;
    int *h_status = nullptr; // pinned

    // detect workspaces
    DevBuf ws_gray, ws_seg, ws_segoff, ws_nraw, ws_rawxy, ws_rawscore, ws_nms, ws_order, ws_nkept;
    // pyramid mode: two level images per frame (level l reads one and writes the other), the lists of levels >= 1
    // ([levels - 1][F][list stride] keypoints, descriptors and, in steered mode, bins) and the level counts ([8][F] survivors,
    // [8][F] raw hits)
    DevBuf ws_pyr_a, ws_pyr_b, ws_pyr_kp, ws_pyr_desc, ws_pyr_bins, ws_pyr_cnt;
    // host-API staging
    DevBuf st_a, st_b, st_c, st_d, st_e, st_f;
    PinBuf pin_in, pin_out; // pgx_match_batch
    // match workspaces: three, so that with several chunks of image pairs the stages of consecutive chunks run side by side
    DevBuf ws_matchn[3];
    DevBuf ws_pose, ws_tracks;
    DevBuf ws_tracks_split; // pgx_tracks_split_dev: ws_tracks' layout plus the active mask, live counters and frame owners
    DevBuf ws_knn; // pgx_match_nn_batch_dev: top-2 and column nearest of a chunk of image pairs
    DevBuf ws_guided; // guided matching: the keypoint grids of the frames of a chunk of image pairs
    DevBuf ws_tri;    // pgx_triangulate_tracks*: camera table, frame -> slot map, per-workgroup counters
    DevBuf ws_ba;     // pgx_bundle_adjust*: control block, cameras, reduced system, per-track and per-node state
    DevBuf ws_reg;    // pgx_register_frames*: target tables, correspondence lists, hypotheses of one chunk, scoring keys
    DevBuf ws_cns;    // pgx_track_consensus*: frame table, ray records and keep flags per node, per-track state, scan block sums
    DevBuf ws_ver;    // pgx_verify_pair*: candidate lists of a chunk of image pairs, hypotheses of one chunk of samples, keys
    DevBuf ws_vocab;  // pgx_vocab_train*, pgx_select_pairs*: words per descriptor, members by word, histograms, weights, scores
    DevBuf ws_depth;  // pgx_depth_maps*, pgx_depth_fuse*: census words per slot, warps, plane tables; camera table, keep flags, block sums
    DevBuf ws_cloud;  // pgx_cloud_merge*: the cell table, per-point records, block sums, the accumulators of the kept cells
    DevBuf ws_mesh;   // pgx_mesh*: the node table with its sums, flags and indices, per-point entries, block sums
    DevBuf ws_mclean; // pgx_mesh_clean*: the union-find, counts and indices per vertex, two position buffers, rows and flags per triangle, block sums
    DevBuf ws_mdec;   // pgx_mesh_decimate*: positions, levels and cluster entries per vertex, the level and cluster tables, triples per triangle, block sums
    DevBuf ws_dviews; // pgx_dense_views*: pair-count table, frame table, depths bucketed by frame, per-frame counts and cursors
    DevBuf ws_init;   // pgx_init_pair_dev, pgx_relative_pose: per image pair the two rotations, t, the intrinsics and the counters
    hipStream_t mstream[3] = {nullptr, nullptr, nullptr}; // [0] wide rounds, [1] residual distance rows, [2] per-pair finish
    hipEvent_t ev_in = nullptr, ev_wide[3] = {nullptr, nullptr, nullptr}, ev_rows[3] = {nullptr, nullptr, nullptr},
               ev_fin[3] = {nullptr, nullptr, nullptr}, ev_join[3] = {nullptr, nullptr, nullptr};
    // recorded behind the stages of the most recent calls (pgx_wait_stage: another context's work is held back until a stage
    // of this one is done -- e.g. its detect chain until the distance rounds here are over, so that it runs beside the
    // residual rows and the per-pair finish instead); [PGX_STAGE_*]
    hipEvent_t ev_stage[4] = {nullptr, nullptr, nullptr, nullptr};
    // pgx_gate_match: the next matcher call waits for this event between its init kernel and its first distance round (one shot)
    hipEvent_t match_gate = nullptr;

    // multi-GPU: the RCCL communicator of this context's process (pgx_comm.hip); world 1 = none
    void *comm = nullptr;
    int comm_rank = 0, comm_world = 1;
    std::string comm_agreed;   // rank-symmetric arguments + cfg_epoch of the last pgx_sequence_step_dev whose local part every rank confirmed
    unsigned cfg_epoch = 0;    // bumped by every pgx_set_* call (the status exchange of pgx_sequence_step_dev runs again after one)
    unsigned long long id = 0; // unique per created context (pgx_last_error tells a new context from a dead one at the same address)
    DevBuf ws_agree;

    // profiling
    bool prof_on = false;
    std::string prof_only; // when not empty: only this kernel group is bracketed (pgx_profile_filter)
    bool prof_serial = false; // matcher stages in order on one stream (stand-alone kernel times)
    std::map<std::string, ProfEntry> prof;
    std::vector<hipEvent_t> ev_pool; // recycled timing events (creating two per launch costs more than the record itself)

    // last match stats
    int last_rounds_mfma = 0;
    long long last_evals = 0;
};

// XCD-aware block -> (frame, block-in-frame) map for batched kernels whose blocks of one frame share data.
// Workgroup ids are dealt round-robin to the 8 XCDs (observed, not contractual), so id % 8 selects the frame
// inside a group of 8 frames and one frame's working set lives in ONE XCD's 4 MiB L2.  Speed only: any
// mapping is correct.  Launch with a 1-D grid of nblk * F blocks.
#ifdef __HIPCC__
__host__ __device__ __forceinline__ unsigned long long *pgx_dbg(int *status) { return reinterpret_cast<unsigned long long *>(status + PGX_DBG_OFF); }
__device__ __forceinline__ void pgx_xcd_map(int lin, int nblk, int F, int &f, int &b)
{
    const int F8 = (F >> 3) << 3;
    if (lin < nblk * F8) {
        const int j = lin >> 3;
        f = (j / nblk) * 8 + (lin & 7);
        b = j % nblk;
    } else {
        const int r = lin - nblk * F8;
        f = F8 + r / nblk;
        b = r % nblk;
    }
}
#endif

// error text of a failing call: kept per calling thread (what pgx_last_error returns to that thread) and on the context
void pgx_note_error(pgx_ctx *c, const std::string &msg);

// RAII event bracket used by the launchers' callers
// attach = true: the scope records nothing itself; the ONE kernel launched inside it takes the two events with
// hipExtLaunchKernelGGL, which stamps the dispatch's own begin and end -- no barrier packets between back-to-back kernels
// (two hipEventRecord per launch of the distance kernel cost 2.4 % of the bench step)
struct ProfScope {
    pgx_ctx *c;
    ProfEntry *e = nullptr;
    hipEvent_t a = nullptr, b = nullptr;
    hipStream_t st;
    bool attach;
    ProfScope(pgx_ctx *ctx, const char *name, hipStream_t s = nullptr, bool attach_to_kernel = false)
        : c(ctx), st(s ? s : ctx->stream), attach(attach_to_kernel)
    {
        if (!name || !c->prof_on || (!c->prof_only.empty() && c->prof_only != name)) return; // no name: brackets nothing
        e = &c->prof[name];
        auto take = [&](hipEvent_t &ev) {
            if (!c->ev_pool.empty()) { ev = c->ev_pool.back(); c->ev_pool.pop_back(); return true; }
            return hipEventCreate(&ev) == hipSuccess;
        };
        if (!take(a) || !take(b)) { e = nullptr; a = b = nullptr; return; }
        if (!attach) (void)hipEventRecord(a, st);
    }
    ~ProfScope()
    {
        if (!e) return;
        if (!attach) (void)hipEventRecord(b, st);
        e->pending.emplace_back(a, b);
    }
};

// ---------------------------------------------------------------------------------------
// kernel launchers (each .hip file owns its kernels)
// ---------------------------------------------------------------------------------------

// k_image.hip
// rgba: [F][H][W] pixels of 4 x uint16 (src8 = 0) or 4 x uint8 (src8 = 1, widened x257 in registers)
void pgx_launch_dewarp_gray(hipStream_t s, const void *rgba, int src8, const int32_t *map_uv, int F, int W, int H,
                            float *gray, uint16_t *dewarped, int *status);
void pgx_launch_dewarp_map(hipStream_t s, int W, int H, const double *k /*[5]*/, int32_t *map_uv, int *status);
// pgx_dewarp's pixel of F frames packed to 8 bits a channel (the high byte of a 16-bit channel): rgba8 [F][H][W]
void pgx_launch_dewarp_rgba8(hipStream_t s, const void *rgba, int src8, const int32_t *map_uv, int F, int W, int H, uint32_t *rgba8,
                             int *status);
// the map's gather plan: plan[W * H] source offsets (PGX_GATHER_OOB outside the image), *flag = 1 when any entry is outside
void pgx_launch_dewarp_plan(hipStream_t s, const int32_t *map_uv, int W, int H, uint32_t *plan, uint32_t *flag);

// k_fast.hip
size_t pgx_fast_seg_count(int W, int H);   // segments per frame
void pgx_launch_fast(hipStream_t s, const float *gray, int F, int W, int H, float T,
                     unsigned long long *seg /*[F][nseg][4]*/, uint32_t *segoff /*[F][nseg]*/,
                     int32_t *n_raw /*[F]*/, uint32_t *raw_xy /*[F][raw_cap]*/,
                     int32_t *raw_score /*[F][raw_cap]*/, int raw_cap, int *status,
                     bool compact = true /* false: planes and ranks only, raw_xy/raw_score are not written */,
                     bool planes = true /* false: pgx_launch_dewarp_fast has written seg and the counts in segoff; gray is not read */);
// dewarp + grey + the FAST planes of F frames in one tile kernel: gray, seg and the counts in segoff as pgx_launch_dewarp_gray
// and pgx_launch_fast's first kernel leave them.  plan / plan_oob: pgx_launch_dewarp_plan's, or nullptr with no map;
// PGX_ST_OOB_SOURCE is raised when *plan_oob is set
void pgx_launch_dewarp_fast(hipStream_t s, const void *rgba, int src8, const uint32_t *plan, const uint32_t *plan_oob, int F,
                            int W, int H, float T, float *gray, unsigned long long *seg, uint32_t *segoff, int *status);

// k_nms.hip
size_t pgx_nms_ws_bytes(int W, int H, int radius, int n_cap, bool planes);
// true when pgx_launch_nms with planes never reads raw_xy/raw_score and fills in the kept points' entries itself
bool pgx_nms_fills_raw_lists(int W, int H, int radius, int n_cap);  // per frame; planes: the fused detect path
void pgx_launch_nms(hipStream_t s, uint32_t *raw_xy, int32_t *raw_score, const int32_t *n_raw,
                    int F, int n_cap, int W, int H, int radius, void *ws, size_t ws_stride,
                    uint32_t *order /*[F][kp_cap]*/, int32_t *n_kept /*[F]*/, int kp_cap, int *status,
                    const unsigned long long *seg = nullptr /* FAST planes: enables atomic-free binning */,
                    const uint32_t *segoff = nullptr,
                    bool kp_soft = false /* true: kp_cap is the caller's soft limit, lists are cut without PGX_ST_KP_CAP */);
// stage API (one list, host waits): whole-chip rounds until nothing is left undecided, see k_nms.hip
hipError_t pgx_launch_nms_sync(hipStream_t s, const uint32_t *raw_xy, const int32_t *raw_score, const int32_t *n_raw,
                               int n_cap, int W, int H, int radius, void *ws, size_t ws_stride, uint32_t *order,
                               int32_t *n_kept, int kp_cap, int *status);

// steered BRIEF: what the launchers of k_brief.hip hand to k_steer.hip's when the mode is on (device pointers)
struct PgxSteer {
    const int32_t *pairs_rot; // [B][P][4]
    const int32_t *plans;     // [B][PGX_PLAN_WORDS]; read when P == 256
    const int32_t *dirs;      // [B][2]
    int B, R;
    int32_t *bins_out;        // fused path only, optional: [F][out_stride]
};

// k_brief.hip; steer != nullptr: the steered kernels of k_steer.hip on the same arguments
void pgx_launch_brief(hipStream_t s, const float *gray, int F, int W, int H,
                      const uint32_t *raw_xy, const int32_t *raw_score, int raw_cap,
                      const uint32_t *order, const int32_t *n_kept, int kp_cap /* order stride and list bound */,
                      const int32_t *pairs, const int32_t *plan /* pgx_brief_plan.h; read when P == 256 */, int P,
                      pgx_keypoint *kp_out, uint32_t *desc_out, int32_t *counts_out, int out_stride /* slots per frame in kp_out/desc_out */,
                      const PgxSteer *steer = nullptr);
// descriptors for an explicit keypoint list (stage API)
void pgx_launch_brief_list(hipStream_t s, const float *gray, int W, int H, const pgx_keypoint *kps, int n,
                           const int32_t *pairs, const int32_t *plan, int P, uint32_t *desc_out, const PgxSteer *steer = nullptr);

// k_steer.hip
void pgx_launch_steer(hipStream_t s, const float *gray, int F, int W, int H, const uint32_t *raw_xy, const int32_t *raw_score,
                      int raw_cap, const uint32_t *order, const int32_t *n_kept, int kp_cap, const PgxSteer &st, int P,
                      pgx_keypoint *kp_out, uint32_t *desc_out, int32_t *counts_out, int out_stride);
void pgx_launch_steer_list(hipStream_t s, const float *gray, int W, int H, const pgx_keypoint *kps, int n, const PgxSteer &st,
                           int P, uint32_t *desc_out);
void pgx_launch_orient_list(hipStream_t s, const float *gray, int W, int H, const pgx_keypoint *kps, int n, const PgxSteer &st,
                            int32_t *bins_out);

// k_pyramid.hip (scale pyramid; pgx_set_pyramid's rules, include/pgx.h)
// level l of F frames from level l - 1: src [F][Hs][Ws] -> dst [F][Hd][Wd]
void pgx_launch_pyr_down(hipStream_t s, const float *src, int F, int Ws, int Hs, float *dst, int Wd, int Hd, int step_q16);
// the merge of rule 5.  Level 0 is already in kp / desc / bins ([F][cap]); levels 1 .. n_run - 1 come from tmp_kp / tmp_desc /
// tmp_bins ([n_levels - 1][F][tmp_stride]); lvl_counts / lvl_nraw [.][F] hold the levels' survivors and raw hits (level-major,
// read for levels < n_run); scale [n_levels] = S_l (host).  origin [F][cap][3], stats [F][n_levels][2], bins: optional.
// A total above cap sets PGX_ST_KP_CAP.
void pgx_launch_pyr_append(hipStream_t s, const pgx_keypoint *tmp_kp, const uint32_t *tmp_desc, const int32_t *tmp_bins,
                           const int32_t *lvl_counts, const int32_t *lvl_nraw, int F, int tmp_stride, int words, int n_levels,
                           int n_run, int W, int H, const int32_t *scale, pgx_keypoint *kp, uint32_t *desc, int32_t *bins,
                           int32_t *counts, int32_t *nraw, int32_t *origin, int32_t *stats, int cap, int *status);

// k_pose.hip
size_t pgx_pose_ws_bytes(int M, int n_samples);
void pgx_launch_fundamental(hipStream_t s, const pgx_keypoint *kp, const pgx_pair *matches, const int32_t *counts,
                            const int32_t *pairlist, int M, int stride, int n_samples, int P, float threshold, int rank_check,
                            uint64_t seed, void *ws, float *F_out, int32_t *inliers, int32_t *best_sample);
void pgx_launch_pose(hipStream_t s, const pgx_keypoint *kp, const pgx_pair *matches, const int32_t *counts,
                     const int32_t *pairlist, int M, int stride, const float *F_in, float *Rt_out, int32_t *votes,
                     int32_t *best, float *points);

// k_tracks.hip
size_t pgx_tracks_ws_bytes(int n_frames, int stride);
void pgx_launch_tracks(hipStream_t s, const pgx_pair *d_matches, const int32_t *d_counts, const int32_t *d_pairlist, int M, int F,
                       int stride, const int32_t *d_frame_ids, int n_frames, int max_dist, int min_len, void *ws,
                       int32_t *d_track_of, int32_t *d_offsets, int32_t *d_nodes, int32_t *d_summary);
// the refinement levels of pgx_tracks_split_dev (include/pgx.h); gates: host array [n_gates], checked by the caller;
// d_summary [16]; duplicate frame ids set PGX_ST_DUP_FRAME in *status
size_t pgx_tracks_split_ws_bytes(int n_frames, int stride);
void pgx_launch_tracks_split(hipStream_t s, const pgx_pair *d_matches, const int32_t *d_counts, const int32_t *d_pairlist, int M,
                             int F, int stride, const int32_t *d_frame_ids, int n_frames, int max_dist, const int *gates,
                             int n_gates, int min_len, void *ws, int32_t *d_track_of, int32_t *d_offsets, int32_t *d_nodes,
                             int32_t *d_summary, int *status);

// k_match.hip
struct MatchPlan {
    int M;        // image pairs
    int stride;   // descriptor slots per frame
    int words;
    int max_n;    // upper bound of any count (<= stride)
    int rounds_mfma;
    int skip_below = PGX_TAIL_FILL_MAX; // a wide round leaves image pairs alone whose residual (rows and columns) is at most this
};
size_t pgx_match_ws_bytes(int M, int stride);
// the three stages of one chunk of image pairs -- wide part (init, whole-chip mutual-nearest rounds), residual distance
// rows (256-bit descriptors only), per-pair finish; they may run on different streams (the caller orders them with events)
// gate: an event the stream waits for between the init kernel and the first distance round (or nullptr)
void pgx_launch_match_wide(pgx_ctx *ctx, hipStream_t s, const uint32_t *d_desc, const int32_t *d_counts,
                           const int32_t *d_pairlist, const MatchPlan &plan, void *ws, int *status, hipEvent_t gate = nullptr);
void pgx_launch_match_rows(pgx_ctx *ctx, hipStream_t s, const uint32_t *d_desc, const int32_t *d_pairlist,
                           const MatchPlan &plan, void *ws, int *status);
void pgx_launch_match_finish(pgx_ctx *ctx, hipStream_t s, const uint32_t *d_desc, const int32_t *d_pairlist,
                             const MatchPlan &plan, void *ws, pgx_pair *d_out, int *status);

// k_knn.hip (exact nearest neighbours; pgx_knn_batch_dev semantics, include/pgx.h)
// d_idx / d_dist [M][S][k], d_col [M][S] or nullptr; max_n in [1, S], k in {1, 2}
void pgx_launch_knn(pgx_ctx *ctx, hipStream_t s, const uint32_t *d_desc, const int32_t *d_counts, const int32_t *d_pairlist, int M,
                    int S, int words, int max_n, int k, int32_t *d_idx, int32_t *d_dist, int32_t *d_col);
// the column output of a producer of (distance << 20 | row) keys, d_col [M][S]: finish = false sets the entries j < counts[b] to
// PGX_KEY_NONE ahead of it, finish = true turns the keys into row indices (-1: no row) behind it.  scope: profiling group or nullptr
void pgx_launch_colkeys(pgx_ctx *ctx, hipStream_t s, const char *scope, bool finish, const int32_t *d_counts,
                        const int32_t *d_pairlist, int M, int S, int max_n, int32_t *d_col);
// the NN list of every row from k = 2 results and the column nearest: d_out [M][S]
void pgx_launch_knn_select(pgx_ctx *ctx, hipStream_t s, const int32_t *d_counts, const int32_t *d_pairlist, int M, int S, int max_n,
                           const int32_t *d_idx, const int32_t *d_dist, const int32_t *d_col, int max_dist, float ratio,
                           int cross_check, pgx_pair *d_out);

// k_guided.hip (epipolar-guided exact matching; pgx_knn_guided_batch_dev semantics, include/pgx.h)
// workspace bytes for a chunk of M image pairs
size_t pgx_guided_ws_bytes(int M, int max_n);
// d_idx / d_dist [M][S][k], d_col [M][S] or nullptr; d_F [M][9]; max_n in [1, S], k in {1, 2}, band finite and >= 0
void pgx_launch_guided(pgx_ctx *ctx, hipStream_t s, const uint32_t *d_desc, const pgx_keypoint *d_kp, const int32_t *d_counts,
                       const int32_t *d_pairlist, int M, int S, int words, int max_n, const float *d_F, float band, int k,
                       int32_t *d_idx, int32_t *d_dist, int32_t *d_col, void *ws, int *status);

// the stages behind the matchers (k_triangulate.hip, k_bundle.hip, k_register.hip, k_consensus.hip, k_verify.hip,
// k_initpair.hip, k_depth.hip): pgx_stage_args.h, each launcher beside its argument struct

// k_vocab.hip (binary visual vocabulary and image-pair selection; pgx_vocab_quantize_dev, pgx_vocab_train_dev and
// pgx_select_pairs_dev semantics, include/pgx.h).  256-bit descriptors; F in [1, 4096], S in [1, 65535], V in [1, 65536]
// d_word / d_wdist [F][S], d_wdist or nullptr
void pgx_launch_vocab_quantize(pgx_ctx *ctx, hipStream_t s, const uint32_t *d_desc, const int32_t *d_counts, int F, int S,
                               const uint32_t *d_vocab, int V, int32_t *d_word, int32_t *d_wdist);
size_t pgx_vocab_train_ws_bytes(int F, int S, int V);
// fewer valid descriptors than words: PGX_ST_VOC_FEW in *status, d_vocab untouched
void pgx_launch_vocab_train(pgx_ctx *ctx, hipStream_t s, const uint32_t *d_desc, const int32_t *d_counts, int F, int S, int V, int iters,
                            uint64_t seed, uint32_t *d_vocab, int32_t *d_report, void *ws, int *status);
// own_scores: the [F][F] score matrix lives in the workspace (the caller passes no d_scores)
size_t pgx_select_pairs_ws_bytes(int F, int S, int V, bool own_scores);
// more than max_pairs pairs: PGX_ST_SEL_CAP in *status
void pgx_launch_select_pairs(pgx_ctx *ctx, hipStream_t s, const uint32_t *d_desc, const int32_t *d_counts, int F, int S,
                             const uint32_t *d_vocab, int V, int weighting, int top_k, int window, int min_score, int max_pairs,
                             int32_t *d_pairlist, int32_t *d_pair_score, int32_t *d_scores, int32_t *d_summary, void *ws, int *status);
