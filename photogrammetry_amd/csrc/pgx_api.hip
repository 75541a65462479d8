// pgx_api.hip -- the C ABI of libpgx.so (see include/pgx.h): context, configuration,
// host-buffer entry points (copy in -> kernels -> copy out) and the device-resident batched
// entry points.  All compute is in the k_*.hip kernels; there is no CPU fallback anywhere:
// every entry point needs a working gfx950 device and fails with PGX_E_HIP without one.
#include "pgx_stage_args.h"
#include "pgx_brief_plan.h"

#include <atomic>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <new>
#include <cstring>
#include <cstdlib>

#define PGX_VERSION_STR "pgx 0.1 (gfx950)"

static thread_local std::string tl_err;
static thread_local const pgx_ctx *tl_err_ctx = nullptr;
static thread_local unsigned long long tl_err_id = 0;   // the context's id: a new context at a dead one's address is not it
static std::atomic<unsigned long long> g_ctx_ids{0};

void pgx_note_error(pgx_ctx *c, const std::string &msg)
{
    tl_err = msg;
    tl_err_ctx = c;
    tl_err_id = c ? c->id : 0;
    if (c) {
        std::lock_guard<std::mutex> g(c->err_mu);
        c->err = msg;
    }
}

namespace {

int fail(pgx_ctx *c, int code, const char *fmt, ...)
{
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    pgx_note_error(c, buf);
    return code;
}

#define HIPCHK(c, expr)                                                                           \
    do {                                                                                          \
        hipError_t e_ = (expr);                                                                   \
        if (e_ != hipSuccess) return fail((c), PGX_E_HIP, "%s: %s", #expr, hipGetErrorString(e_)); \
    } while (0)

struct Lock {
    std::lock_guard<std::mutex> g;
    explicit Lock(pgx_ctx *c) : g(c->mu) { (void)hipSetDevice(c->device); }
};

int decode_status(pgx_ctx *c, int bits)
{
    if (bits & PGX_ST_OOB_SOURCE)
        return fail(c, PGX_E_OOB_SOURCE, "dewarp map points outside the source image (IndexOutOfRangeException)");
    if (bits & PGX_ST_EMPTY_SET)
        return fail(c, PGX_E_EMPTY_SET, "keypoints2 is empty while keypoints1 is not (ArgumentOutOfRangeException)");
    if (bits & PGX_ST_RAW_CAP)
        return fail(c, PGX_E_CAPACITY, "raw FAST hits exceed max_raw_per_frame (pgx_set_capacity)");
    if (bits & PGX_ST_KP_CAP) return fail(c, PGX_E_CAPACITY, "NMS survivors exceed the output capacity");
    if (bits & PGX_ST_INTERNAL) return fail(c, PGX_E_HIP, "internal error: a device-side loop stopped without progress");
    if (bits & PGX_ST_BADARG)
        return fail(c, PGX_E_BADARG, "guided matching: a keypoint coordinate is outside [-2^20, 2^20) (its pairs' rows were rejected)");
    if (bits & PGX_ST_DUP_FRAME)
        return fail(c, PGX_E_BADARG, "track graph: two slots of d_frame_ids name the same frame (the split graph's result is undefined)");
    if (bits & PGX_ST_TRI_CAP) return fail(c, PGX_E_CAPACITY, "triangulation: n_tracks exceeds max_tracks (only the first max_tracks were written)");
    if (bits & PGX_ST_TRI_NODE)
        return fail(c, PGX_E_BADARG, "triangulation: a node names a frame outside [0, n_frames), a keypoint outside [0, stride) or a frame no slot "
                                     "holds, or the offsets are malformed (those nodes were skipped)");
    if (bits & PGX_ST_TRI_DUP)
        return fail(c, PGX_E_BADARG, "triangulation: two slots of d_frame_ids name the same frame");
    if (bits & PGX_ST_BA_CAP)
        return fail(c, PGX_E_CAPACITY, "bundle adjustment: n_tracks exceeds max_tracks (only the first max_tracks took part)");
    if (bits & PGX_ST_BA_FREE) return fail(c, PGX_E_CAPACITY, "bundle adjustment: more than 128 free frames (no iteration ran)");
    if (bits & PGX_ST_BA_NODE)
        return fail(c, PGX_E_BADARG, "bundle adjustment: a node outside the frames / keypoint slots, malformed offsets, or a track with two "
                                     "nodes in one frame (those nodes or tracks were skipped)");
    if (bits & PGX_ST_BA_DUP) return fail(c, PGX_E_BADARG, "bundle adjustment: two slots of d_frame_ids name the same frame");
    if (bits & PGX_ST_BA_ROT)
        return fail(c, PGX_E_BADARG, "bundle adjustment: a finite R is not a rotation (max |R R^T - I| > 1e-9 or det R <= 0; the frame was "
                                     "treated as unknown)");
    if (bits & PGX_ST_BA_NOFIX) return fail(c, PGX_E_BADARG, "bundle adjustment: no known frame is fixed (no iteration ran)");
    if (bits & PGX_ST_REG_CAP)
        return fail(c, PGX_E_CAPACITY, "registration: n_tracks exceeds max_tracks (only the first max_tracks were used)");
    if (bits & PGX_ST_REG_NODE)
        return fail(c, PGX_E_BADARG, "registration: a node outside the frames / keypoint slots, or malformed offsets (those nodes or "
                                     "tracks were skipped)");
    if (bits & PGX_ST_REG_DUP) return fail(c, PGX_E_BADARG, "registration: two slots of d_frame_ids name the same frame");
    if (bits & PGX_ST_REG_TWICE)
        return fail(c, PGX_E_BADARG, "registration: a track has two nodes in one target frame (those nodes were skipped)");
    if (bits & PGX_ST_CNS_CAP)
        return fail(c, PGX_E_CAPACITY, "track consensus: n_tracks exceeds max_tracks (only the first max_tracks were processed)");
    if (bits & PGX_ST_CNS_NODE)
        return fail(c, PGX_E_BADARG, "track consensus: a node outside the frames / keypoint slots, or malformed offsets (those nodes "
                                     "were dropped)");
    if (bits & PGX_ST_CNS_DUP) return fail(c, PGX_E_BADARG, "track consensus: two slots of d_frame_ids name the same frame");
    if (bits & PGX_ST_VOC_FEW)
        return fail(c, PGX_E_BADARG, "vocabulary training: fewer valid descriptors than words (d_vocab was not written)");
    if (bits & PGX_ST_SEL_CAP)
        return fail(c, PGX_E_CAPACITY, "pair selection: more than max_pairs pairs were selected (the first max_pairs were written)");
    if (bits & PGX_ST_DEP_CAP)
        return fail(c, PGX_E_CAPACITY, "depth fusion: more than max_points pixels were kept (the first max_points were written)");
    if (bits & PGX_ST_CLD_CAP)
        return fail(c, PGX_E_CAPACITY, "cloud merge: more than max_points cells were kept (the first max_points were written)");
    if (bits & PGX_ST_MSH_CAP)
        return fail(c, PGX_E_CAPACITY, "mesh: more than max_voxels voxels (nothing was written), or more than max_vertices vertices or "
                                       "max_tris triangles (the first ones were written)");
    if (bits & PGX_ST_MCL_CAP)
        return fail(c, PGX_E_CAPACITY, "mesh clean: more than max_out_vertices vertices or max_out_tris triangles were kept (the first "
                                       "ones were written)");
    if (bits & PGX_ST_MDC_CAP)
        return fail(c, PGX_E_CAPACITY, "mesh decimate: more than max_out_vertices vertices or max_out_tris triangles were kept (the "
                                       "first ones were written)");
    if (bits & PGX_ST_DVW_CAP)
        return fail(c, PGX_E_CAPACITY, "dense views: n_tracks exceeds max_tracks (only the first max_tracks were processed)");
    if (bits & PGX_ST_DVW_NODE)
        return fail(c, PGX_E_BADARG, "dense views: a node of a used track names a frame outside [0, n_frames), or the offsets are "
                                     "malformed (those nodes were skipped)");
    return PGX_OK;
}

// wait for the stream, read and clear the sticky status word
int sync_status(pgx_ctx *c)
{
    HIPCHK(c, hipMemcpyAsync(c->h_status, c->d_status, sizeof(int), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemsetAsync(c->d_status, 0, sizeof(int), c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    HIPCHK(c, hipGetLastError());
    return decode_status(c, c->h_status[0]);
}

// image dimensions: PGX_OK, or PGX_E_BADARG with the text `what`
int dims_ok(pgx_ctx *c, int W, int H, const char *what = "dimensions must fit ushort")
{
    return W <= 0 || H <= 0 || W > 65535 || H > 65535 ? fail(c, PGX_E_BADARG, "%s", what) : PGX_OK;
}

} // namespace

// The next four are also called by pgx_comm.hip (the caller holds the context's mutex).

namespace {

// the levels of a W x H frame under the context's pyramid (rules 1 and 2 of pgx_set_pyramid); mode off: level 0 alone
struct PyrPlan {
    int n_levels = 1, n_run = 1; // levels of the mode; those of them that are not empty
    int32_t dims[8][2] = {};
    int32_t scale[8] = {};
};

PyrPlan pyr_plan(const pgx_ctx *c, int W, int H)
{
    PyrPlan p;
    p.dims[0][0] = W; p.dims[0][1] = H; p.scale[0] = 65536;
    if (c->pyr_levels <= 1) return p;
    p.n_levels = c->pyr_levels;
    (void)pgx_pyramid_dims(W, H, p.n_levels, c->pyr_step, &p.dims[0][0], p.scale); // the caller has checked W and H
    while (p.n_run < p.n_levels && p.dims[p.n_run][0] > 0) p.n_run++;
    return p;
}

} // namespace

// every check and workspace allocation of the detect chain (no kernel launch): pgx_sequence_step_dev calls it before its
// first collective so that no rank can fail locally between two collectives.  In pyramid mode every workspace holds the
// largest requirement over the levels, and the level images and per-level lists are allocated here too.
int pgx_prepare_detect(pgx_ctx *c, int F, int W, int H, int cap)
{
    if (!c->params_set) return fail(c, PGX_E_NOT_CONFIGURED, "pgx_set_detect_params not called");
    if (!c->pairs_set) return fail(c, PGX_E_NOT_CONFIGURED, "pgx_set_brief_pairs not called");
    if (dims_ok(c, W, H) != PGX_OK) return PGX_E_BADARG;
    if (c->map_set && (c->mapW != W || c->mapH != H))
        return fail(c, PGX_E_DIM_MISMATCH, "image %dx%d vs dewarp map %dx%d (ArgumentException)", W, H, c->mapW, c->mapH);
    if (F <= 0) return PGX_OK;
    const PyrPlan pl = pyr_plan(c, W, H);
    const size_t npix = (size_t)W * H;
    const int raw_cap = c->raw_cap;
    size_t nseg = 0, nms_stride = 0; // neither is assumed monotone in the frame size
    for (int l = 0; l < pl.n_run; l++) {
        const size_t sg = pgx_fast_seg_count(pl.dims[l][0], pl.dims[l][1]);
        const size_t ns = pgx_nms_ws_bytes(pl.dims[l][0], pl.dims[l][1], c->radius, raw_cap, true);
        nseg = sg > nseg ? sg : nseg;
        nms_stride = ns > nms_stride ? ns : nms_stride;
    }
    HIPCHK(c, c->ws_gray.ensure((size_t)F * npix * 4));
    HIPCHK(c, c->ws_seg.ensure((size_t)F * nseg * 32));
    HIPCHK(c, c->ws_segoff.ensure((size_t)F * nseg * 4));
    HIPCHK(c, c->ws_rawxy.ensure((size_t)F * raw_cap * 4));
    HIPCHK(c, c->ws_rawscore.ensure((size_t)F * raw_cap * 4));
    HIPCHK(c, c->ws_nms.ensure((size_t)F * nms_stride));
    const int kp_eff = c->kp_cap <= cap ? c->kp_cap : cap;
    HIPCHK(c, c->ws_order.ensure((size_t)F * kp_eff * 4));
    HIPCHK(c, c->ws_nkept.ensure((size_t)F * 4));
    if (pl.n_levels > 1) {
        HIPCHK(c, c->ws_pyr_cnt.ensure((size_t)16 * F * 4));
        if (pl.n_run > 1) {
            const size_t slots = (size_t)(pl.n_run - 1) * F * kp_eff;
            HIPCHK(c, c->ws_pyr_a.ensure((size_t)F * pl.dims[1][0] * pl.dims[1][1] * 4));
            if (pl.n_run > 2) HIPCHK(c, c->ws_pyr_b.ensure((size_t)F * pl.dims[2][0] * pl.dims[2][1] * 4));
            HIPCHK(c, c->ws_pyr_kp.ensure(slots * sizeof(pgx_keypoint)));
            HIPCHK(c, c->ws_pyr_desc.ensure(slots * c->words * 4));
            if (c->steer_on) HIPCHK(c, c->ws_pyr_bins.ensure(slots * 4));
        }
    }
    return PGX_OK;
}

namespace {

// the context's steering tables as the BRIEF launchers take them
PgxSteer steer_of(const pgx_ctx *c, int32_t *d_bins = nullptr)
{
    return PgxSteer{c->d_steer_pairs.as<int32_t>(), c->d_steer_plans.as<int32_t>(), c->d_steer_dirs.as<int32_t>(), c->steer_B,
                    c->steer_R, d_bins};
}

// the chain behind the grey image, FAST -> NMS -> BRIEF, on F grey images of W x H (enqueue only): survivor lists of
// out_stride slots per frame
void enqueue_from_gray(pgx_ctx *c, const float *gray, int F, int W, int H, int kp_eff, bool kp_soft, pgx_keypoint *d_kp,
                       uint32_t *d_desc, int32_t *d_counts, int32_t *d_nraw, int out_stride, int32_t *d_bins)
{
    const int raw_cap = c->raw_cap;
    const size_t nms_stride = pgx_nms_ws_bytes(W, H, c->radius, raw_cap, true);
    // level 0 of the batch path (enqueue_detect_bins sets fuse_rgba for that one call): gray is not there yet, the fused
    // kernel makes it together with the planes
    const void *rgba = c->fuse_rgba;
    c->fuse_rgba = nullptr;
    {
        ProfScope ps(c, "fast");
        if (rgba)
            pgx_launch_dewarp_fast(c->stream, rgba, c->src8, c->map_set ? c->d_gather.as<uint32_t>() : nullptr,
                                   c->map_set ? c->gather_flag() : nullptr, F, W, H, c->threshold, const_cast<float *>(gray),
                                   c->ws_seg.as<unsigned long long>(), c->ws_segoff.as<uint32_t>(), c->d_status);
        pgx_launch_fast(c->stream, gray, F, W, H, c->threshold, c->ws_seg.as<unsigned long long>(),
                        c->ws_segoff.as<uint32_t>(), d_nraw, c->ws_rawxy.as<uint32_t>(),
                        c->ws_rawscore.as<int32_t>(), raw_cap, c->d_status,
                        !pgx_nms_fills_raw_lists(W, H, c->radius, raw_cap), rgba == nullptr);
    }
    {
        ProfScope ps(c, "nms");
        pgx_launch_nms(c->stream, c->ws_rawxy.as<uint32_t>(), c->ws_rawscore.as<int32_t>(), d_nraw, F, raw_cap, W, H,
                       c->radius, c->ws_nms.p, nms_stride, c->ws_order.as<uint32_t>(), c->ws_nkept.as<int32_t>(),
                       kp_eff, c->d_status, c->ws_seg.as<unsigned long long>(), c->ws_segoff.as<uint32_t>(), kp_soft);
    }
    {
        ProfScope ps(c, "brief");
        const PgxSteer st = steer_of(c, d_bins);
        pgx_launch_brief(c->stream, gray, F, W, H, c->ws_rawxy.as<uint32_t>(), c->ws_rawscore.as<int32_t>(), raw_cap,
                         c->ws_order.as<uint32_t>(), c->ws_nkept.as<int32_t>(), kp_eff, c->d_pairs.as<int32_t>(), c->d_plan.as<int32_t>(), c->P,
                         d_kp, d_desc, d_counts, out_stride, c->steer_on ? &st : nullptr);
    }
}

// detect chain on device-resident frames (enqueue only); d_bins (steered mode only, optional): each survivor's direction.
// Pyramid mode: the chain behind the grey image runs once per level, level 0 straight into the caller's buffers, and
// k_pyr_append merges the rest behind it; d_origin / d_stats (optional) as pgx_detect_batch_pyramid_dev describes them.
int enqueue_detect_bins(pgx_ctx *c, const uint16_t *d_rgba, int F, int W, int H, pgx_keypoint *d_kp, uint32_t *d_desc,
                        int32_t *d_counts, int32_t *d_nraw, int cap, int32_t *d_bins, int32_t *d_origin = nullptr,
                        int32_t *d_stats = nullptr)
{
    const int rcp = pgx_prepare_detect(c, F, W, H, cap);
    if (rcp != PGX_OK) return rcp;
    if (F <= 0) return PGX_OK;
    // pgx_set_capacity's survivor limit: lists are cut to their first kp_cap entries (NMS order) without an error;
    // only an overflow of the caller's own `cap` raises PGX_E_CAPACITY
    const bool kp_soft = c->kp_cap <= cap;
    const int kp_eff = kp_soft ? c->kp_cap : cap;

    // No dewarped RGBA is wanted here, so level 0 gathers, greys and runs FAST in one tile kernel (k_dewarp_fast, inside the
    // "fast" group of enqueue_from_gray): the grey plane is written for BRIEF and the pyramid and never read back by FAST
    float *gray = c->ws_gray.as<float>();
    c->fuse_rgba = d_rgba;
    if (c->pyr_levels <= 1) {
        enqueue_from_gray(c, gray, F, W, H, kp_eff, kp_soft, d_kp, d_desc, d_counts, d_nraw, cap, d_bins);
    } else {
        const PyrPlan pl = pyr_plan(c, W, H);
        int32_t *lvl_counts = c->ws_pyr_cnt.as<int32_t>(), *lvl_nraw = lvl_counts + (size_t)8 * F;
        const size_t lvl_slots = (size_t)F * kp_eff;
        int32_t *tmp_bins = d_bins ? c->ws_pyr_bins.as<int32_t>() : nullptr;
        enqueue_from_gray(c, gray, F, W, H, kp_eff, kp_soft, d_kp, d_desc, lvl_counts, lvl_nraw, cap, d_bins);
        const float *src = gray;
        for (int l = 1; l < pl.n_run; l++) {
            float *dst = (l & 1) ? c->ws_pyr_a.as<float>() : c->ws_pyr_b.as<float>();
            {
                ProfScope ps(c, "pyramid");
                pgx_launch_pyr_down(c->stream, src, F, pl.dims[l - 1][0], pl.dims[l - 1][1], dst, pl.dims[l][0], pl.dims[l][1],
                                    c->pyr_step);
            }
            enqueue_from_gray(c, dst, F, pl.dims[l][0], pl.dims[l][1], kp_eff, kp_soft,
                              c->ws_pyr_kp.as<pgx_keypoint>() + (l - 1) * lvl_slots,
                              c->ws_pyr_desc.as<uint32_t>() + (l - 1) * lvl_slots * c->words, lvl_counts + (size_t)l * F,
                              lvl_nraw + (size_t)l * F, kp_eff, tmp_bins ? tmp_bins + (l - 1) * lvl_slots : nullptr);
            src = dst;
        }
        {
            ProfScope ps(c, "pyramid_append");
            pgx_launch_pyr_append(c->stream, c->ws_pyr_kp.as<pgx_keypoint>(), c->ws_pyr_desc.as<uint32_t>(), tmp_bins, lvl_counts,
                                  lvl_nraw, F, kp_eff, c->words, pl.n_levels, pl.n_run, W, H, pl.scale, d_kp, d_desc, d_bins,
                                  d_counts, d_nraw, d_origin, d_stats, cap, c->d_status);
        }
    }
    HIPCHK(c, hipEventRecord(c->ev_stage[PGX_STAGE_DETECT], c->stream));
    HIPCHK(c, hipGetLastError());
    return PGX_OK;
}

} // namespace

int pgx_enqueue_detect(pgx_ctx *c, const uint16_t *d_rgba, int F, int W, int H, pgx_keypoint *d_kp, uint32_t *d_desc,
                       int32_t *d_counts, int32_t *d_nraw, int cap)
{
    return enqueue_detect_bins(c, d_rgba, F, W, H, d_kp, d_desc, d_counts, d_nraw, cap, nullptr);
}

// checks and workspace allocation of the matcher for M image pairs of `stride` descriptor slots (no kernel launch)
int pgx_prepare_match(pgx_ctx *c, int stride, int words, int M)
{
    if (M <= 0) return PGX_OK;
    if (stride <= 0 || stride > (1 << PGX_IDX_BITS)) return fail(c, PGX_E_BADARG, "stride must be in [1, 2^20]");
    if (words <= 0 || words > 127) return fail(c, PGX_E_BADARG, "words must be in [1, 127] (P <= 4064)");
    const int CHUNK = c->match_chunk;
    const int mc = M < CHUNK ? M : CHUNK;
    const int nws = (M <= CHUNK || c->prof_serial || CHUNK >= PGX_PIPELINE_BELOW) ? 1 : 3;
    for (int k = 0; k < nws; k++) HIPCHK(c, c->ws_matchn[k].ensure(pgx_match_ws_bytes(mc, stride)));
    return PGX_OK;
}

int pgx_enqueue_match(pgx_ctx *c, const uint32_t *d_desc, const int32_t *d_counts, int stride, int words,
                      const int32_t *d_pairlist, int M, int max_n, pgx_pair *d_out)
{
    // pgx_gate_match is one shot on the NEXT matcher call, whatever becomes of that call: taken and cleared before any
    // early return, so that a gate never stays armed for some later call (its event belongs to another context)
    hipEvent_t gate = c->match_gate;
    c->match_gate = nullptr;
    if (M <= 0) return PGX_OK;
    const int rcp = pgx_prepare_match(c, stride, words, M);
    if (rcp != PGX_OK) return rcp;
    // image pairs go through in chunks so the per-pair workspace stays bounded
    const int CHUNK = c->match_chunk;
    MatchPlan plan;
    plan.stride = stride; plan.words = words;
    plan.max_n = max_n > stride ? stride : (max_n < 1 ? 1 : max_n);
    // all-CU rounds until the residual fits the per-pair tail (random data halves per round; each launch
    // skips image pairs that already fit, so extra rounds only cost their launch)
    plan.rounds_mfma = 0;
    // 256-bit descriptors: k_tail_rows caches the residual's distance rows up to PGX_TAIL_MAX, so wide rounds stop there;
    // other lengths: the tail workgroup stages the descriptors itself (PGX_TAIL_FILL_MAX)
    plan.skip_below = words == 8 ? PGX_TAIL_MAX : PGX_TAIL_FILL_MAX;
    // One or two image pairs (a pgx_match call): the per-pair finish is one workgroup per pair and leaves the chip idle, so the
    // whole-chip rounds go on to half that size first.  Measured at N = 4096 (tools/call_latency.py): random descriptor sets
    // 0.33 -> 0.27 ms per call, detect-chain sets of translated frames 0.29 -> 0.30 (their finish is bound by the number of
    // its rounds, not by the residual's size), true-match sets unchanged.  From 8 pairs per call on the lower threshold costs
    // more than it saves on the frame sets (+6 %), and at full chunks +0.6 ms per bench step: those keep PGX_TAIL_MAX.
    if (words == 8 && M <= 2) plan.skip_below = PGX_TAIL_MAX / 2;
    for (int n = plan.max_n; n > plan.skip_below && plan.rounds_mfma < PGX_MAX_WIDE_ROUNDS; n = (n + 1) / 2) plan.rounds_mfma++;
    if (plan.rounds_mfma > 0 && plan.rounds_mfma < PGX_MAX_WIDE_ROUNDS) plan.rounds_mfma++;
    HIPCHK(c, hipMemsetAsync(c->d_status + 4, 0, PGX_MAX_WIDE_ROUNDS * 8, c->stream));
    // Chunks of PGX_PIPELINE_BELOW image pairs or more go through in order on the context's stream, one workspace: every
    // stage of the matcher is bound by vector-instruction issue, so running the stages of consecutive chunks side by side
    // buys nothing (round 4: 6.43 ms side by side against 6.25 in order at 1024 pairs per chunk), while a large chunk gives
    // the per-pair finish several workgroups per CU to balance (2016 pairs in one chunk: 6.0 ms).
    if (M <= CHUNK || c->prof_serial || CHUNK >= PGX_PIPELINE_BELOW) { // everything in order on the context's stream
        for (int m0 = 0; m0 < M; m0 += CHUNK) {
            plan.M = (M - m0 < CHUNK) ? M - m0 : CHUNK;
            const int32_t *pl = d_pairlist + 2 * (size_t)m0;
            pgx_launch_match_wide(c, c->stream, d_desc, d_counts, pl, plan, c->ws_matchn[0].p, c->d_status, m0 == 0 ? gate : nullptr);
            const bool last = m0 + CHUNK >= M; // pgx_wait_stage: the stages of the last chunk stand for the call
            if (last) HIPCHK(c, hipEventRecord(c->ev_stage[PGX_STAGE_MATCH_WIDE], c->stream));
            pgx_launch_match_rows(c, c->stream, d_desc, pl, plan, c->ws_matchn[0].p, c->d_status);
            if (last) HIPCHK(c, hipEventRecord(c->ev_stage[PGX_STAGE_MATCH_ROWS], c->stream));
            pgx_launch_match_finish(c, c->stream, d_desc, pl, plan, c->ws_matchn[0].p, d_out + (size_t)m0 * stride, c->d_status);
        }
    } else {
        // Several chunks: a three-stage pipeline over chunks on three streams -- the whole-chip mutual-nearest rounds
        // (matrix pipe) of chunk i + 2 beside the residual distance rows (matrix pipe + stores) of chunk i + 1 beside the
        // per-pair finish of chunk i (latency-bound, one small workgroup per pair on half of the CUs).  Three workspaces
        // rotate; events order "inputs ready -> wide(i) -> rows(i) -> finish(i) -> wide(i + 3)".  The streams sit in
        // different stream-priority classes where the device has three: streams of one class share a small pool of hardware
        // queues round-robin, and two streams that land on one queue run strictly in order.  (Two finishes in flight on
        // alternating streams were measured too: 15.3 ms per step of config 3 against 12.6 -- their registers and LDS
        // crowd the matrix kernels out of every CU.)
        const int NS = 3;
        int lo = 0, hi = 0;
        HIPCHK(c, hipDeviceGetStreamPriorityRange(&lo, &hi)); // lo = least priority (numerically greatest)
        for (int k = 0; k < NS; k++) {
            if (!c->mstream[k]) {
                const int prio = k == 0 ? lo : (k == 2 ? hi : (lo + hi) / 2);
                HIPCHK(c, hipStreamCreateWithPriority(&c->mstream[k], hipStreamNonBlocking, prio));
            }
            if (!c->ev_wide[k]) HIPCHK(c, hipEventCreateWithFlags(&c->ev_wide[k], hipEventDisableTiming));
            if (!c->ev_rows[k]) HIPCHK(c, hipEventCreateWithFlags(&c->ev_rows[k], hipEventDisableTiming));
            if (!c->ev_fin[k]) HIPCHK(c, hipEventCreateWithFlags(&c->ev_fin[k], hipEventDisableTiming));
            if (!c->ev_join[k]) HIPCHK(c, hipEventCreateWithFlags(&c->ev_join[k], hipEventDisableTiming));
        }
        if (!c->ev_in) HIPCHK(c, hipEventCreateWithFlags(&c->ev_in, hipEventDisableTiming));
        hipStream_t sw = c->mstream[0], sr = c->mstream[1];
        if (gate) HIPCHK(c, hipStreamWaitEvent(c->stream, gate, 0)); // the three-stream form takes the gate in front of everything
        HIPCHK(c, hipEventRecord(c->ev_in, c->stream));
        for (int k = 0; k < NS; k++) HIPCHK(c, hipStreamWaitEvent(c->mstream[k], c->ev_in, 0));
        int i = 0;
        for (int m0 = 0; m0 < M; m0 += CHUNK, i++) {
            const int b = i % NS;
            hipStream_t sf = c->mstream[2];
            void *ws = c->ws_matchn[b].p;
            const int32_t *pl = d_pairlist + 2 * (size_t)m0;
            plan.M = (M - m0 < CHUNK) ? M - m0 : CHUNK;
            if (i >= NS) HIPCHK(c, hipStreamWaitEvent(sw, c->ev_fin[b], 0)); // this workspace's previous chunk is finished
            pgx_launch_match_wide(c, sw, d_desc, d_counts, pl, plan, ws, c->d_status);
            HIPCHK(c, hipEventRecord(c->ev_wide[b], sw));
            if (m0 + CHUNK >= M) HIPCHK(c, hipEventRecord(c->ev_stage[PGX_STAGE_MATCH_WIDE], sw));
            HIPCHK(c, hipStreamWaitEvent(sr, c->ev_wide[b], 0));
            pgx_launch_match_rows(c, sr, d_desc, pl, plan, ws, c->d_status);
            HIPCHK(c, hipEventRecord(c->ev_rows[b], sr));
            if (m0 + CHUNK >= M) HIPCHK(c, hipEventRecord(c->ev_stage[PGX_STAGE_MATCH_ROWS], sr));
            HIPCHK(c, hipStreamWaitEvent(sf, c->ev_rows[b], 0));
            pgx_launch_match_finish(c, sf, d_desc, pl, plan, ws, d_out + (size_t)m0 * stride, c->d_status);
            HIPCHK(c, hipEventRecord(c->ev_fin[b], sf));
        }
        for (int k = 0; k < NS; k++) {
            HIPCHK(c, hipEventRecord(c->ev_join[k], c->mstream[k]));
            HIPCHK(c, hipStreamWaitEvent(c->stream, c->ev_join[k], 0));
        }
    }
    c->last_rounds_mfma = plan.rounds_mfma;
    HIPCHK(c, hipEventRecord(c->ev_stage[PGX_STAGE_MATCH_DONE], c->stream));
    HIPCHK(c, hipGetLastError());
    return PGX_OK;
}

extern "C" {

const char *pgx_version(void) { return PGX_VERSION_STR; }

int pgx_ctx_create(int device, pgx_ctx **out)
{
    if (!out) return PGX_E_BADARG;
    *out = nullptr;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0 || device < 0 || device >= ndev) return PGX_E_HIP;
    if (hipSetDevice(device) != hipSuccess) return PGX_E_HIP;
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, device) != hipSuccess) return PGX_E_HIP;
    if (strncmp(prop.gcnArchName, "gfx950", 6) != 0) {
        fprintf(stderr, "pgx: device %d is %s; this library is built for gfx950 only\n", device, prop.gcnArchName);
        return PGX_E_HIP;
    }
    pgx_ctx *c = new (std::nothrow) pgx_ctx();
    if (!c) return PGX_E_HIP;
    c->device = device;
    c->id = ++g_ctx_ids;
    if (hipStreamCreateWithFlags(&c->own_stream, hipStreamNonBlocking) != hipSuccess ||
        hipEventCreateWithFlags(&c->ev_stage[0], hipEventDisableTiming) != hipSuccess ||
        hipEventCreateWithFlags(&c->ev_stage[1], hipEventDisableTiming) != hipSuccess ||
        hipEventCreateWithFlags(&c->ev_stage[2], hipEventDisableTiming) != hipSuccess ||
        hipEventCreateWithFlags(&c->ev_stage[3], hipEventDisableTiming) != hipSuccess ||
        hipMalloc(reinterpret_cast<void **>(&c->d_status), 256) != hipSuccess ||
        hipHostMalloc(reinterpret_cast<void **>(&c->h_status), 64, hipHostMallocDefault) != hipSuccess ||
        hipMemset(c->d_status, 0, 256) != hipSuccess) {
        pgx_ctx_destroy(c);
        return PGX_E_HIP;
    }
    c->stream = c->own_stream;
    *out = c;
    return PGX_OK;
}

void pgx_ctx_destroy(pgx_ctx *c)
{
    if (!c) return;
    (void)hipSetDevice(c->device);
    if (c->stream) (void)hipStreamSynchronize(c->stream);
    if (c->comm) (void)pgx_comm_destroy(c);
    for (auto &kv : c->prof)
        for (auto &ev : kv.second.pending) { (void)hipEventDestroy(ev.first); (void)hipEventDestroy(ev.second); }
    for (hipEvent_t ev : c->ev_pool) (void)hipEventDestroy(ev);
    DevBuf *bufs[] = {&c->d_pairs, &c->d_plan, &c->d_steer_pairs, &c->d_steer_plans, &c->d_steer_dirs, &c->d_map, &c->d_gather, &c->ws_gray, &c->ws_seg, &c->ws_segoff, &c->ws_nraw, &c->ws_rawxy,
                      &c->ws_rawscore, &c->ws_nms, &c->ws_order, &c->ws_nkept, &c->st_a, &c->st_b, &c->st_c,
                      &c->st_d, &c->st_e, &c->st_f, &c->ws_pose, &c->ws_tracks, &c->ws_tracks_split, &c->ws_agree, &c->ws_matchn[0], &c->ws_matchn[1], &c->ws_matchn[2], &c->ws_knn, &c->ws_guided, &c->ws_tri, &c->ws_ba, &c->ws_reg, &c->ws_ver, &c->ws_init, &c->ws_cns, &c->ws_vocab, &c->ws_depth, &c->ws_dviews, &c->ws_cloud, &c->ws_mesh, &c->ws_mclean, &c->ws_mdec,
                      &c->ws_pyr_a, &c->ws_pyr_b, &c->ws_pyr_kp, &c->ws_pyr_desc, &c->ws_pyr_bins, &c->ws_pyr_cnt};
    for (DevBuf *b : bufs) b->release();
    c->pin_in.release();
    c->pin_out.release();
    if (c->d_status) (void)hipFree(c->d_status);
    if (c->h_status) (void)hipHostFree(c->h_status);
    for (int k = 0; k < 3; k++) {
        if (c->mstream[k]) (void)hipStreamDestroy(c->mstream[k]);
        if (c->ev_wide[k]) (void)hipEventDestroy(c->ev_wide[k]);
        if (c->ev_rows[k]) (void)hipEventDestroy(c->ev_rows[k]);
        if (c->ev_fin[k]) (void)hipEventDestroy(c->ev_fin[k]);
        if (c->ev_join[k]) (void)hipEventDestroy(c->ev_join[k]);
    }
    if (c->ev_in) (void)hipEventDestroy(c->ev_in);
    for (int k = 0; k < 4; k++) if (c->ev_stage[k]) (void)hipEventDestroy(c->ev_stage[k]);
    if (c->own_stream) (void)hipStreamDestroy(c->own_stream);
    delete c;
}

const char *pgx_last_error(pgx_ctx *c)
{
    if (!c) return "null context";
    if (tl_err_ctx == c && tl_err_id == c->id) return tl_err.c_str();   // this thread's own last failure on this context
    static thread_local std::string copy;         // another thread's: a private copy, valid until this thread asks again
    {
        std::lock_guard<std::mutex> g(c->err_mu);
        copy = c->err;
    }
    return copy.c_str();
}

int pgx_set_stream(pgx_ctx *c, void *hip_stream)
{
    if (!c) return PGX_E_BADARG;
    Lock l(c);
    c->cfg_epoch++;
    HIPCHK(c, hipStreamSynchronize(c->stream));
    c->stream = hip_stream ? reinterpret_cast<hipStream_t>(hip_stream) : c->own_stream;
    return PGX_OK;
}

int pgx_check_status(pgx_ctx *c)
{
    if (!c) return PGX_E_BADARG;
    Lock l(c);
    return sync_status(c);
}

int pgx_set_dewarp_map(pgx_ctx *c, const int32_t *uv, int W, int H)
{
    if (!c) return PGX_E_BADARG;
    Lock l(c);
    c->cfg_epoch++;
    if (!uv) {
        HIPCHK(c, hipStreamSynchronize(c->stream)); // a chain in flight may still read the plan
        c->d_gather.release();
        c->map_set = false; c->mapW = c->mapH = 0;
        return PGX_OK;
    }
    if (dims_ok(c, W, H, "map dimensions must fit ushort") != PGX_OK) return PGX_E_BADARG;
    const size_t bytes = (size_t)W * H * 8;
    HIPCHK(c, hipStreamSynchronize(c->stream));
    HIPCHK(c, c->d_map.ensure(bytes + 32));
    HIPCHK(c, c->d_gather.ensure(bytes / 2 + 4));
    HIPCHK(c, hipMemcpy(c->d_map.p, uv, bytes, hipMemcpyHostToDevice));
    c->mapW = W; c->mapH = H; c->map_set = true;
    pgx_launch_dewarp_plan(c->stream, c->d_map.as<int32_t>(), W, H, c->d_gather.as<uint32_t>(), c->gather_flag());
    HIPCHK(c, hipGetLastError());
    return PGX_OK;
}

int pgx_set_dewarp_coeffs(pgx_ctx *c, int W, int H, const double *coeffs, int ncoeffs)
{
    if (!c || !coeffs) return c ? fail(c, PGX_E_BADARG, "null pointer") : PGX_E_BADARG;
    Lock l(c);
    c->cfg_epoch++;
    if (ncoeffs != 5) return fail(c, PGX_E_BADARG, "You must pass exactly 5 distortion coefficients (ArgumentException)"); // DeWarp.cs:46-48
    if (dims_ok(c, W, H, "map dimensions must fit ushort") != PGX_OK) return PGX_E_BADARG;
    const size_t bytes = (size_t)W * H * 8;
    HIPCHK(c, hipStreamSynchronize(c->stream));
    HIPCHK(c, c->d_map.ensure(bytes + 32));
    HIPCHK(c, c->d_gather.ensure(bytes / 2 + 4));
    pgx_launch_dewarp_map(c->stream, W, H, coeffs, c->d_map.as<int32_t>(), c->d_status);
    c->mapW = W; c->mapH = H; c->map_set = true;
    pgx_launch_dewarp_plan(c->stream, c->d_map.as<int32_t>(), W, H, c->d_gather.as<uint32_t>(), c->gather_flag());
    HIPCHK(c, hipGetLastError());
    return sync_status(c);
}

int pgx_get_dewarp_map(pgx_ctx *c, int32_t *uv_out, int W, int H)
{
    if (!c || !uv_out) return c ? fail(c, PGX_E_BADARG, "null pointer") : PGX_E_BADARG;
    Lock l(c);
    if (!c->map_set) return fail(c, PGX_E_NOT_CONFIGURED, "no dewarp map is set");
    if (W != c->mapW || H != c->mapH) return fail(c, PGX_E_DIM_MISMATCH, "map is %dx%d, asked for %dx%d", c->mapW, c->mapH, W, H);
    HIPCHK(c, hipStreamSynchronize(c->stream));
    HIPCHK(c, hipMemcpy(uv_out, c->d_map.p, (size_t)W * H * 8, hipMemcpyDeviceToHost));
    return PGX_OK;
}

int pgx_set_brief_pairs(pgx_ctx *c, const int32_t *pairs, int P)
{
    if (!c) return PGX_E_BADARG;
    Lock l(c);
    c->cfg_epoch++;
    if (!pairs || P <= 0 || P > 4064) return fail(c, PGX_E_BADARG, "P must be in [1, 4064]");
    HIPCHK(c, hipStreamSynchronize(c->stream));
    HIPCHK(c, c->d_pairs.ensure((size_t)P * 16));
    HIPCHK(c, hipMemcpy(c->d_pairs.p, pairs, (size_t)P * 16, hipMemcpyHostToDevice));
    if (P == PGX_PLAN_PAIRS) { // brief_256 reads the table through its row-sorted sample plan (pgx_brief_plan.h)
        int32_t plan[PGX_PLAN_WORDS];
        pgx_build_brief_plan(pairs, plan);
        HIPCHK(c, c->d_plan.ensure(sizeof plan));
        HIPCHK(c, hipMemcpy(c->d_plan.p, plan, sizeof plan, hipMemcpyHostToDevice));
    }
    c->P = P; c->words = (P + 31) / 32; c->pairs_set = true;
    c->steer_on = false; // turned tables belong to the table they were turned from
    return PGX_OK;
}

int pgx_set_brief_steering(pgx_ctx *c, const int32_t *pairs_rot, const int32_t *dirs, int B, int radius)
{
    if (!c) return PGX_E_BADARG;
    Lock l(c);
    c->cfg_epoch++;
    if (!pairs_rot) { c->steer_on = false; return PGX_OK; }
    if (!c->pairs_set) return fail(c, PGX_E_NOT_CONFIGURED, "pgx_set_brief_pairs not called");
    if (!dirs) return fail(c, PGX_E_BADARG, "null pointer");
    if (B < 4 || B > 64 || B % 4 != 0) return fail(c, PGX_E_BADARG, "B must be a multiple of 4 in [4, 64]");
    if (radius < 1 || radius > 31) return fail(c, PGX_E_BADARG, "radius must be in [1, 31]");
    for (int i = 0; i < 2 * B; i++)
        if (dirs[i] < -32767 || dirs[i] > 32767) return fail(c, PGX_E_BADARG, "dirs components must be in [-32767, 32767]");
    const size_t tbytes = (size_t)B * c->P * 16;
    HIPCHK(c, hipStreamSynchronize(c->stream));
    c->steer_on = false; // until everything below is in place
    HIPCHK(c, c->d_steer_pairs.ensure(tbytes));
    HIPCHK(c, hipMemcpy(c->d_steer_pairs.p, pairs_rot, tbytes, hipMemcpyHostToDevice));
    HIPCHK(c, c->d_steer_dirs.ensure((size_t)B * 8));
    HIPCHK(c, hipMemcpy(c->d_steer_dirs.p, dirs, (size_t)B * 8, hipMemcpyHostToDevice));
    if (c->P == PGX_PLAN_PAIRS) { // one row-sorted sample plan per direction: brief_256 as it is
        std::vector<int32_t> plans((size_t)B * PGX_PLAN_WORDS);
        for (int k = 0; k < B; k++) pgx_build_brief_plan(pairs_rot + (size_t)k * PGX_PLAN_PAIRS * 4, plans.data() + (size_t)k * PGX_PLAN_WORDS);
        HIPCHK(c, c->d_steer_plans.ensure(plans.size() * 4));
        HIPCHK(c, hipMemcpy(c->d_steer_plans.p, plans.data(), plans.size() * 4, hipMemcpyHostToDevice));
    }
    c->steer_B = B; c->steer_R = radius; c->steer_on = true;
    return PGX_OK;
}

int pgx_set_pyramid(pgx_ctx *c, int n_levels, int step_q16)
{
    if (!c) return PGX_E_BADARG;
    Lock l(c);
    c->cfg_epoch++;
    if (n_levels < 1 || n_levels > 8) return fail(c, PGX_E_BADARG, "n_levels must be in [1, 8]");
    if (step_q16 < 69632 || step_q16 > 131072) return fail(c, PGX_E_BADARG, "step_q16 must be in [69632, 131072] (1.0625 ... 2.0)");
    c->pyr_levels = n_levels; c->pyr_step = step_q16;
    return PGX_OK;
}

int pgx_set_detect_params(pgx_ctx *c, float threshold, int suppression_radius)
{
    if (!c) return PGX_E_BADARG;
    Lock l(c);
    c->cfg_epoch++;
    c->threshold = threshold; c->radius = suppression_radius; c->params_set = true;
    return PGX_OK;
}

int pgx_set_match_chunk(pgx_ctx *c, int pairs)
{
    if (!c) return PGX_E_BADARG;
    Lock l(c);
    c->cfg_epoch++;
    if (pairs < 16 || pairs > 4096) return fail(c, PGX_E_BADARG, "image pairs per chunk must be in [16, 4096]");
    c->match_chunk = pairs;
    return PGX_OK;
}

int pgx_wait_stage(pgx_ctx *c, pgx_ctx *other, int stage)
{
    if (!c || !other) return c ? fail(c, PGX_E_BADARG, "null context") : PGX_E_BADARG;
    Lock l(c);
    if (stage < 0 || stage > PGX_STAGE_MATCH_DONE) return fail(c, PGX_E_BADARG, "unknown stage %d", stage);
    if (c == other) return PGX_OK; // a stream is in order with itself
    if (c->device != other->device) return fail(c, PGX_E_BADARG, "contexts on different devices (%d, %d)", c->device, other->device);
    // other->ev_stage[] are created with the context and never replaced: no lock on `other` (taking two context mutexes
    // here could deadlock against a thread that calls the two contexts the other way round); an event that has not been
    // recorded yet does not hold the stream
    HIPCHK(c, hipStreamWaitEvent(c->stream, other->ev_stage[stage], 0));
    return PGX_OK;
}

int pgx_gate_match(pgx_ctx *c, pgx_ctx *other, int stage)
{
    if (!c || !other) return c ? fail(c, PGX_E_BADARG, "null context") : PGX_E_BADARG;
    Lock l(c);
    if (stage < 0 || stage > PGX_STAGE_MATCH_DONE) return fail(c, PGX_E_BADARG, "unknown stage %d", stage);
    if (c->device != other->device) return fail(c, PGX_E_BADARG, "contexts on different devices (%d, %d)", c->device, other->device);
    c->match_gate = c == other ? nullptr : other->ev_stage[stage]; // events live as long as their context (see pgx_wait_stage)
    return PGX_OK;
}

int pgx_set_source_format(pgx_ctx *c, int format)
{
    if (!c) return PGX_E_BADARG;
    Lock l(c);
    c->cfg_epoch++;
    if (format != PGX_SRC_RGBA64 && format != PGX_SRC_RGBA8) return fail(c, PGX_E_BADARG, "unknown source format %d", format);
    c->src8 = format == PGX_SRC_RGBA8;
    return PGX_OK;
}

int pgx_set_capacity(pgx_ctx *c, int max_raw, int max_kp)
{
    if (!c) return PGX_E_BADARG;
    Lock l(c);
    c->cfg_epoch++;
    if (max_raw <= 0 || max_kp <= 0 || max_kp > (1 << PGX_IDX_BITS)) return fail(c, PGX_E_BADARG, "bad capacity");
    c->raw_cap = max_raw; c->kp_cap = max_kp;
    return PGX_OK;
}

// ---- stage-granular host entry points ---------------------------------------------------

int pgx_dewarp(pgx_ctx *c, const uint16_t *rgba, int W, int H, uint16_t *out)
{
    if (!c || !rgba || !out) return c ? fail(c, PGX_E_BADARG, "null pointer") : PGX_E_BADARG;
    Lock l(c);
    if (!c->map_set) return fail(c, PGX_E_NOT_CONFIGURED, "pgx_set_dewarp_map not called");
    if (W != c->mapW || H != c->mapH)   // DeWarp.cs:22-23
        return fail(c, PGX_E_DIM_MISMATCH, "image %dx%d vs dewarp map %dx%d (ArgumentException)", W, H, c->mapW, c->mapH);
    const size_t bytes = (size_t)W * H * 8, in_bytes = (size_t)W * H * (c->src8 ? 4 : 8);
    HIPCHK(c, c->st_a.ensure(bytes + 32));
    HIPCHK(c, c->st_b.ensure(bytes + 32));
    HIPCHK(c, hipMemcpyAsync(c->st_a.p, rgba, in_bytes, hipMemcpyHostToDevice, c->stream));
    pgx_launch_dewarp_gray(c->stream, c->st_a.p, c->src8, c->d_map.as<int32_t>(), 1, W, H, nullptr,
                           c->st_b.as<uint16_t>(), c->d_status);
    HIPCHK(c, hipMemcpyAsync(out, c->st_b.p, bytes, hipMemcpyDeviceToHost, c->stream));
    return sync_status(c);
}

int pgx_gray(pgx_ctx *c, const uint16_t *rgba, int W, int H, float *out)
{
    if (!c || !rgba || !out) return c ? fail(c, PGX_E_BADARG, "null pointer") : PGX_E_BADARG;
    Lock l(c);
    if (dims_ok(c, W, H) != PGX_OK) return PGX_E_BADARG;
    const size_t npix = (size_t)W * H;
    HIPCHK(c, c->st_a.ensure(npix * 8 + 32));
    HIPCHK(c, c->st_b.ensure(npix * 4 + 32));
    HIPCHK(c, hipMemcpyAsync(c->st_a.p, rgba, npix * (c->src8 ? 4 : 8), hipMemcpyHostToDevice, c->stream));
    pgx_launch_dewarp_gray(c->stream, c->st_a.p, c->src8, nullptr, 1, W, H, c->st_b.as<float>(), nullptr,
                           c->d_status);
    HIPCHK(c, hipMemcpyAsync(out, c->st_b.p, npix * 4, hipMemcpyDeviceToHost, c->stream));
    return sync_status(c);
}

int pgx_fast(pgx_ctx *c, const float *gray, int W, int H, pgx_keypoint *out, int capacity, int *n_out)
{
    if (!c || !gray || !n_out || (capacity > 0 && !out) || capacity < 0)
        return c ? fail(c, PGX_E_BADARG, "null pointer") : PGX_E_BADARG;
    Lock l(c);
    if (!c->params_set) return fail(c, PGX_E_NOT_CONFIGURED, "pgx_set_detect_params not called");
    if (dims_ok(c, W, H) != PGX_OK) return PGX_E_BADARG;
    const size_t npix = (size_t)W * H, nseg = pgx_fast_seg_count(W, H);
    const int cap = capacity > 0 ? capacity : 1;
    HIPCHK(c, c->st_a.ensure(npix * 4 + 32));
    HIPCHK(c, c->ws_seg.ensure(nseg * 32));
    HIPCHK(c, c->ws_segoff.ensure(nseg * 4));
    HIPCHK(c, c->ws_nraw.ensure(64));
    HIPCHK(c, c->st_b.ensure((size_t)cap * 4));
    HIPCHK(c, c->st_c.ensure((size_t)cap * 4));
    HIPCHK(c, hipMemcpyAsync(c->st_a.p, gray, npix * 4, hipMemcpyHostToDevice, c->stream));
    pgx_launch_fast(c->stream, c->st_a.as<float>(), 1, W, H, c->threshold, c->ws_seg.as<unsigned long long>(),
                    c->ws_segoff.as<uint32_t>(), c->ws_nraw.as<int32_t>(), c->st_b.as<uint32_t>(),
                    c->st_c.as<int32_t>(), cap, c->d_status);
    int n = 0;
    HIPCHK(c, hipMemcpyAsync(&n, c->ws_nraw.p, 4, hipMemcpyDeviceToHost, c->stream));
    int rc = sync_status(c);
    *n_out = n;
    const int nw = n < capacity ? n : capacity;
    if (nw > 0) {
        std::vector<uint32_t> xy(nw);
        std::vector<int32_t> sc(nw);
        HIPCHK(c, hipMemcpy(xy.data(), c->st_b.p, (size_t)nw * 4, hipMemcpyDeviceToHost));
        HIPCHK(c, hipMemcpy(sc.data(), c->st_c.p, (size_t)nw * 4, hipMemcpyDeviceToHost));
        for (int i = 0; i < nw; i++) {
            out[i].x = (int32_t)(xy[i] & 0xFFFFu);
            out[i].y = (int32_t)(xy[i] >> 16);
            out[i].fast_score = sc[i];
            out[i].value = gray[(size_t)out[i].y * W + out[i].x]; // Keypoint.cs:26 (a copy of the caller's pixel)
        }
    }
    if (rc == PGX_OK && n > capacity) return fail(c, PGX_E_CAPACITY, "%d hits, capacity %d", n, capacity);
    return rc;
}

int pgx_brief(pgx_ctx *c, const float *gray, int W, int H, const pgx_keypoint *kps, int n, uint32_t *desc_out)
{
    if (!c || !gray || n < 0 || (n > 0 && (!kps || !desc_out)))
        return c ? fail(c, PGX_E_BADARG, "null pointer") : PGX_E_BADARG;
    Lock l(c);
    if (!c->pairs_set) return fail(c, PGX_E_NOT_CONFIGURED, "pgx_set_brief_pairs not called");
    if (dims_ok(c, W, H) != PGX_OK) return PGX_E_BADARG;
    if (n == 0) return PGX_OK;
    const size_t npix = (size_t)W * H;
    HIPCHK(c, c->st_a.ensure(npix * 4 + 32));
    HIPCHK(c, c->st_b.ensure((size_t)n * sizeof(pgx_keypoint)));
    HIPCHK(c, c->st_c.ensure((size_t)n * c->words * 4));
    HIPCHK(c, hipMemcpyAsync(c->st_a.p, gray, npix * 4, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(c->st_b.p, kps, (size_t)n * sizeof(pgx_keypoint), hipMemcpyHostToDevice, c->stream));
    const PgxSteer st = steer_of(c);
    pgx_launch_brief_list(c->stream, c->st_a.as<float>(), W, H, c->st_b.as<pgx_keypoint>(), n,
                          c->d_pairs.as<int32_t>(), c->d_plan.as<int32_t>(), c->P, c->st_c.as<uint32_t>(), c->steer_on ? &st : nullptr);
    HIPCHK(c, hipMemcpyAsync(desc_out, c->st_c.p, (size_t)n * c->words * 4, hipMemcpyDeviceToHost, c->stream));
    return sync_status(c);
}

int pgx_orient(pgx_ctx *c, const float *gray, int W, int H, const pgx_keypoint *kps, int n, int32_t *bins_out)
{
    if (!c || !gray || n < 0 || (n > 0 && (!kps || !bins_out)))
        return c ? fail(c, PGX_E_BADARG, "null pointer") : PGX_E_BADARG;
    Lock l(c);
    if (!c->steer_on) return fail(c, PGX_E_NOT_CONFIGURED, "pgx_set_brief_steering not called");
    if (dims_ok(c, W, H) != PGX_OK) return PGX_E_BADARG;
    if (n == 0) return PGX_OK;
    const size_t npix = (size_t)W * H;
    HIPCHK(c, c->st_a.ensure(npix * 4 + 32));
    HIPCHK(c, c->st_b.ensure((size_t)n * sizeof(pgx_keypoint)));
    HIPCHK(c, c->st_c.ensure((size_t)n * 4));
    HIPCHK(c, hipMemcpyAsync(c->st_a.p, gray, npix * 4, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(c->st_b.p, kps, (size_t)n * sizeof(pgx_keypoint), hipMemcpyHostToDevice, c->stream));
    pgx_launch_orient_list(c->stream, c->st_a.as<float>(), W, H, c->st_b.as<pgx_keypoint>(), n, steer_of(c), c->st_c.as<int32_t>());
    HIPCHK(c, hipMemcpyAsync(bins_out, c->st_c.p, (size_t)n * 4, hipMemcpyDeviceToHost, c->stream));
    return sync_status(c);
}

int pgx_pyramid_level(pgx_ctx *c, const float *gray, int W, int H, int level, float *out)
{
    if (!c || !gray || !out) return c ? fail(c, PGX_E_BADARG, "null pointer") : PGX_E_BADARG;
    Lock l(c);
    if (c->pyr_levels <= 1) return fail(c, PGX_E_NOT_CONFIGURED, "pgx_set_pyramid not called (or called with one level)");
    if (dims_ok(c, W, H) != PGX_OK) return PGX_E_BADARG;
    const PyrPlan pl = pyr_plan(c, W, H);
    if (level < 0 || level >= pl.n_levels) return fail(c, PGX_E_BADARG, "level %d outside [0, %d)", level, pl.n_levels);
    if (level >= pl.n_run) return fail(c, PGX_E_BADARG, "level %d of a %dx%d image is empty", level, W, H);
    const size_t npix = (size_t)W * H;
    HIPCHK(c, c->st_a.ensure(npix * 4 + 32));
    if (level >= 1) HIPCHK(c, c->st_b.ensure((size_t)pl.dims[1][0] * pl.dims[1][1] * 4 + 32));
    if (level >= 2) HIPCHK(c, c->st_c.ensure((size_t)pl.dims[2][0] * pl.dims[2][1] * 4 + 32));
    HIPCHK(c, hipMemcpyAsync(c->st_a.p, gray, npix * 4, hipMemcpyHostToDevice, c->stream));
    const float *src = c->st_a.as<float>();
    for (int k = 1; k <= level; k++) {
        float *dst = (k & 1) ? c->st_b.as<float>() : c->st_c.as<float>();
        ProfScope ps(c, "pyramid");
        pgx_launch_pyr_down(c->stream, src, 1, pl.dims[k - 1][0], pl.dims[k - 1][1], dst, pl.dims[k][0], pl.dims[k][1], c->pyr_step);
        src = dst;
    }
    HIPCHK(c, hipMemcpyAsync(out, src, (size_t)pl.dims[level][0] * pl.dims[level][1] * 4, hipMemcpyDeviceToHost, c->stream));
    return sync_status(c);
}

int pgx_nms(pgx_ctx *c, const pgx_keypoint *kps, int n, int W, int H, int32_t *order_out, int *n_out)
{
    if (!c || !n_out || n < 0 || (n > 0 && (!kps || !order_out)))
        return c ? fail(c, PGX_E_BADARG, "null pointer") : PGX_E_BADARG;
    Lock l(c);
    if (!c->params_set) return fail(c, PGX_E_NOT_CONFIGURED, "pgx_set_detect_params not called");
    if (dims_ok(c, W, H) != PGX_OK) return PGX_E_BADARG;
    *n_out = 0;
    if (n == 0) return PGX_OK;
    std::vector<uint32_t> xy(n);
    std::vector<int32_t> sc(n);
    for (int i = 0; i < n; i++) {
        if (kps[i].x < 0 || kps[i].x >= W || kps[i].y < 0 || kps[i].y >= H)
            return fail(c, PGX_E_BADARG, "keypoint %d (%d,%d) outside %dx%d", i, kps[i].x, kps[i].y, W, H);
        xy[i] = ((uint32_t)kps[i].y << 16) | (uint32_t)kps[i].x;
        sc[i] = kps[i].fast_score;
    }
    const size_t wsb = pgx_nms_ws_bytes(W, H, c->radius, n, false);
    HIPCHK(c, c->st_a.ensure((size_t)n * 4));
    HIPCHK(c, c->st_b.ensure((size_t)n * 4));
    HIPCHK(c, c->st_c.ensure((size_t)n * 4));
    HIPCHK(c, c->st_d.ensure(64));
    HIPCHK(c, c->ws_nms.ensure(wsb));
    HIPCHK(c, hipMemcpyAsync(c->st_a.p, xy.data(), (size_t)n * 4, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(c->st_b.p, sc.data(), (size_t)n * 4, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(c->st_d.p, &n, 4, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, pgx_launch_nms_sync(c->stream, c->st_a.as<uint32_t>(), c->st_b.as<int32_t>(), c->st_d.as<int32_t>(), n, W, H,
                                  c->radius, c->ws_nms.p, wsb, c->st_c.as<uint32_t>(), c->st_d.as<int32_t>() + 1, n,
                                  c->d_status));
    int nk = 0;
    HIPCHK(c, hipMemcpyAsync(&nk, c->st_d.as<int32_t>() + 1, 4, hipMemcpyDeviceToHost, c->stream));
    int rc = sync_status(c);
    if (rc != PGX_OK) return rc;
    *n_out = nk;
    if (nk > 0) HIPCHK(c, hipMemcpy(order_out, c->st_c.p, (size_t)nk * 4, hipMemcpyDeviceToHost));
    return PGX_OK;
}

namespace {

// A host form's images (pgx_hoststage.h) onto the device: inputs packed in pin_in and uploaded to st_a in one copy, outputs in st_b
int stage_images(pgx_ctx *c, HostImage &in, HostImage &out)
{
    HIPCHK(c, c->pin_in.ensure(in.total()));
    HIPCHK(c, c->st_a.ensure(in.total()));
    HIPCHK(c, c->st_b.ensure(out.total()));
    in.pack(c->pin_in.as<char>());
    in.base = c->st_a.as<char>();
    out.base = c->st_b.as<char>();
    HIPCHK(c, hipMemcpyAsync(c->st_a.p, c->pin_in.p, in.total(), hipMemcpyHostToDevice, c->stream));
    return PGX_OK;
}

// ... and back: one copy per output section that has a destination, then the call's status
int download_images(pgx_ctx *c, const HostImage &out)
{
    for (const HostImage::Move &m : out.moves) HIPCHK(c, hipMemcpyAsync(m.host, out.base + m.off, m.bytes, hipMemcpyDeviceToHost, c->stream));
    return sync_status(c);
}

// ... and the first n rows of the sections that were added without a destination, once a downloaded report has told n
struct FetchRows {
    int sec;       // of out
    void *host;
    size_t elem;   // bytes per row
};
int fetch_rows(pgx_ctx *c, const HostImage &out, std::initializer_list<FetchRows> rows, size_t n)
{
    if (n == 0) return PGX_OK;
    for (const FetchRows &r : rows) HIPCHK(c, hipMemcpy(r.host, out.dev<char>(r.sec), n * r.elem, hipMemcpyDeviceToHost));
    return PGX_OK;
}

// ... of a mesh list (mesh_out) into the caller's arrays: report[5] vertices and report[6] triangles, at most the capacities
int fetch_mesh(pgx_ctx *c, const HostImage &out, const MeshOut &o, const MeshRows &host, const int32_t *report, int max_vertices, int max_tris)
{
    const size_t nv = (size_t)(report[5] < max_vertices ? report[5] : max_vertices), nt = (size_t)(report[6] < max_tris ? report[6] : max_tris);
    const int rf = fetch_rows(c, out, {{o.xyz, host.xyz, 24}, {o.normal, host.normal, 12}, {o.rgba8, host.rgba8, 4}, {o.info, host.info, 16}}, nv);
    return rf != PGX_OK ? rf : fetch_rows(c, out, {{o.tri, host.tri, 12}}, nt);
}

} // namespace

int pgx_match(pgx_ctx *c, const uint32_t *desc1, int n1, const uint32_t *desc2, int n2, int words, pgx_pair *out)
{
    if (!c || n1 < 0 || n2 < 0 || (n1 > 0 && (!desc1 || !out)) || (n2 > 0 && !desc2))
        return c ? fail(c, PGX_E_BADARG, "null pointer") : PGX_E_BADARG;
    Lock l(c);
    if (n1 == 0) return PGX_OK;                                  // KeypointMatching.cs:38: loop never runs
    if (n2 == 0) return fail(c, PGX_E_EMPTY_SET, "keypoints2 is empty (ArgumentOutOfRangeException)"); // :61
    if (words <= 0 || words > 127) return fail(c, PGX_E_BADARG, "words must be in [1, 127]");
    const int S = n1 > n2 ? n1 : n2;
    if (S > (1 << PGX_IDX_BITS)) return fail(c, PGX_E_BADARG, "more than 2^20 keypoints");
    HostImage in, ot;
    const TwoSetsIn i = two_sets_in(in, desc1, nullptr, n1, desc2, nullptr, n2, S, words, nullptr);
    const int o_out = ot.add(out, n1, sizeof(pgx_pair), S);
    if (const int rs = stage_images(c, in, ot); rs != PGX_OK) return rs;
    const int32_t *d_meta = in.dev<int32_t>(i.meta);
    const int rc = pgx_enqueue_match(c, in.dev<uint32_t>(i.desc), d_meta, S, words, d_meta + 2, 1, S, ot.dev<pgx_pair>(o_out));
    if (rc != PGX_OK) return rc;
    return download_images(c, ot);
}

int pgx_match_batch(pgx_ctx *c, const uint32_t *const *descs, const int32_t *counts, int n_frames, int words,
                    const int32_t *pair_list, int n_pairs, pgx_pair *out, int64_t *out_offsets)
{
    if (!c || n_frames < 0 || n_pairs < 0 || (n_frames > 0 && (!descs || !counts)) || (n_pairs > 0 && !pair_list))
        return c ? fail(c, PGX_E_BADARG, "null pointer") : PGX_E_BADARG;
    Lock l(c);
    if (words <= 0 || words > 127) return fail(c, PGX_E_BADARG, "words must be in [1, 127]");
    for (int f = 0; f < n_frames; f++) {
        if (counts[f] < 0 || counts[f] > (1 << PGX_IDX_BITS)) return fail(c, PGX_E_BADARG, "counts[%d] = %d", f, counts[f]);
        if (counts[f] > 0 && !descs[f]) return fail(c, PGX_E_BADARG, "descs[%d] is null", f);
    }
    // the slot size S (descriptor slots per frame, entries per list) is the largest set that some image pair REFERENCES:
    // a large frame nobody matches costs neither upload nor workspace nor download
    int S = 1;
    std::vector<char> used((size_t)(n_frames > 0 ? n_frames : 1), 0);
    int64_t total = 0;
    bool empty_set = false;
    for (int m = 0; m < n_pairs; m++) {
        const int fa = pair_list[2 * m], fb = pair_list[2 * m + 1];
        if (fa < 0 || fa >= n_frames || fb < 0 || fb >= n_frames) return fail(c, PGX_E_BADARG, "pair %d names frame %d / %d of %d", m, fa, fb, n_frames);
        if (out_offsets) out_offsets[m] = total;
        total += counts[fa];
        if (counts[fa] > 0 && counts[fb] == 0) empty_set = true;
        used[(size_t)fa] = used[(size_t)fb] = 1;
        if (counts[fa] > S) S = counts[fa];
        if (counts[fb] > S) S = counts[fb];
    }
    if (out_offsets) out_offsets[n_pairs] = total;
    if (n_pairs == 0 || total == 0) return PGX_OK;
    if (!out) return fail(c, PGX_E_BADARG, "null pointer");
    // one upload (an unreferenced frame's count is never read on the device); the lists [n_pairs][S] are carved and come back
    // in ONE copy to pin_out, not one per image pair, and are scattered to `out` from there
    HostImage in, ot;
    const BatchIn i = batch_in(in, descs, counts, used.data(), n_frames, S, words, pair_list, n_pairs);
    const int o_out = ot.add(nullptr, 0, sizeof(pgx_pair), (size_t)n_pairs * S);
    const size_t out_bytes = (size_t)n_pairs * S * sizeof(pgx_pair);
    HIPCHK(c, c->pin_out.ensure(out_bytes));
    if (const int rs = stage_images(c, in, ot); rs != PGX_OK) return rs;
    int rc = pgx_enqueue_match(c, in.dev<uint32_t>(i.desc), in.dev<int32_t>(i.counts), S, words, in.dev<int32_t>(i.pairs), n_pairs, S,
                               ot.dev<pgx_pair>(o_out));
    if (rc != PGX_OK) return rc;
    HIPCHK(c, hipMemcpyAsync(c->pin_out.p, ot.dev<pgx_pair>(o_out), out_bytes, hipMemcpyDeviceToHost, c->stream));
    rc = sync_status(c);
    if (rc != PGX_OK && rc != PGX_E_EMPTY_SET) return rc;
    const pgx_pair *hout = c->pin_out.as<pgx_pair>();
    int64_t o = 0;
    for (int m = 0; m < n_pairs; m++) {
        const int n = counts[pair_list[2 * m]];
        if (n > 0) memcpy(out + o, hout + (size_t)m * S, (size_t)n * sizeof(pgx_pair));
        o += n;
    }
    if (empty_set || rc == PGX_E_EMPTY_SET) return fail(c, PGX_E_EMPTY_SET, "keypoints2 is empty while keypoints1 is not (ArgumentOutOfRangeException)");
    return PGX_OK;
}

int pgx_detect(pgx_ctx *c, const uint16_t *rgba, int W, int H, pgx_keypoint *kp_out, uint32_t *desc_out,
               int capacity, int *n_out, int *n_raw)
{
    if (!c || !rgba || !kp_out || !desc_out || !n_out || capacity <= 0)
        return c ? fail(c, PGX_E_BADARG, "null pointer") : PGX_E_BADARG;
    Lock l(c);
    if (dims_ok(c, W, H) != PGX_OK) return PGX_E_BADARG;
    const size_t npix = (size_t)W * H;
    HIPCHK(c, c->st_e.ensure(npix * 8 + 32));
    HIPCHK(c, c->st_f.ensure((size_t)capacity * (sizeof(pgx_keypoint) + (size_t)(c->words ? c->words : 1) * 4) + 64));
    pgx_keypoint *d_kp = c->st_f.as<pgx_keypoint>();
    uint32_t *d_desc = reinterpret_cast<uint32_t *>(d_kp + capacity);
    int32_t *d_cnt = reinterpret_cast<int32_t *>(d_desc + (size_t)capacity * (c->words ? c->words : 1));
    HIPCHK(c, hipMemcpyAsync(c->st_e.p, rgba, npix * (c->src8 ? 4 : 8), hipMemcpyHostToDevice, c->stream));
    int rc = pgx_enqueue_detect(c, c->st_e.as<uint16_t>(), 1, W, H, d_kp, d_desc, d_cnt, d_cnt + 1, capacity);
    if (rc != PGX_OK) return rc;
    int cnt[2] = {0, 0};
    HIPCHK(c, hipMemcpyAsync(cnt, d_cnt, 8, hipMemcpyDeviceToHost, c->stream));
    rc = sync_status(c);
    *n_out = cnt[0];
    if (n_raw) *n_raw = cnt[1];
    if (cnt[0] > 0) {
        HIPCHK(c, hipMemcpy(kp_out, d_kp, (size_t)cnt[0] * sizeof(pgx_keypoint), hipMemcpyDeviceToHost));
        HIPCHK(c, hipMemcpy(desc_out, d_desc, (size_t)cnt[0] * c->words * 4, hipMemcpyDeviceToHost));
    }
    return rc;
}

// ---- device-resident batched entry points -------------------------------------------------

int pgx_detect_batch_dev(pgx_ctx *c, const uint16_t *d_rgba, int F, int W, int H, pgx_keypoint *d_kp,
                         uint32_t *d_desc, int32_t *d_counts, int32_t *d_nraw, int capacity)
{
    if (!c || !d_rgba || !d_kp || !d_desc || !d_counts || !d_nraw || capacity <= 0 || F < 0)
        return c ? fail(c, PGX_E_BADARG, "null pointer") : PGX_E_BADARG;
    Lock l(c);
    if (dims_ok(c, W, H) != PGX_OK) return PGX_E_BADARG;
    return pgx_enqueue_detect(c, d_rgba, F, W, H, d_kp, d_desc, d_counts, d_nraw, capacity);
}

int pgx_detect_batch_steered_dev(pgx_ctx *c, const uint16_t *d_rgba, int F, int W, int H, pgx_keypoint *d_kp,
                                 uint32_t *d_desc, int32_t *d_counts, int32_t *d_nraw, int capacity, int32_t *d_bins)
{
    if (!c || !d_rgba || !d_kp || !d_desc || !d_counts || !d_nraw || !d_bins || capacity <= 0 || F < 0)
        return c ? fail(c, PGX_E_BADARG, "null pointer") : PGX_E_BADARG;
    Lock l(c);
    if (!c->steer_on) return fail(c, PGX_E_NOT_CONFIGURED, "pgx_set_brief_steering not called");
    if (dims_ok(c, W, H) != PGX_OK) return PGX_E_BADARG;
    return enqueue_detect_bins(c, d_rgba, F, W, H, d_kp, d_desc, d_counts, d_nraw, capacity, d_bins);
}

int pgx_detect_batch_pyramid_dev(pgx_ctx *c, const uint16_t *d_rgba, int F, int W, int H, pgx_keypoint *d_kp, uint32_t *d_desc,
                                 int32_t *d_counts, int32_t *d_nraw, int capacity, int32_t *d_origin, int32_t *d_level_stats,
                                 int32_t *d_bins)
{
    if (!c || !d_rgba || !d_kp || !d_desc || !d_counts || !d_nraw || !d_origin || !d_level_stats || capacity <= 0 || F < 0)
        return c ? fail(c, PGX_E_BADARG, "null pointer") : PGX_E_BADARG;
    Lock l(c);
    if (c->pyr_levels <= 1) return fail(c, PGX_E_NOT_CONFIGURED, "pgx_set_pyramid not called (or called with one level)");
    if (d_bins && !c->steer_on) return fail(c, PGX_E_NOT_CONFIGURED, "d_bins given but pgx_set_brief_steering not called");
    if (dims_ok(c, W, H) != PGX_OK) return PGX_E_BADARG;
    return enqueue_detect_bins(c, d_rgba, F, W, H, d_kp, d_desc, d_counts, d_nraw, capacity, d_bins, d_origin, d_level_stats);
}

int pgx_match_batch_dev(pgx_ctx *c, const uint32_t *d_desc, const int32_t *d_counts, int stride, int words,
                        const int32_t *d_pairlist, int M, int max_count, pgx_pair *d_out)
{
    if (!c || !d_desc || !d_counts || !d_pairlist || !d_out || M < 0)
        return c ? fail(c, PGX_E_BADARG, "null pointer") : PGX_E_BADARG;
    Lock l(c);
    return pgx_enqueue_match(c, d_desc, d_counts, stride, words, d_pairlist, M, max_count, d_out);
}

// ---- exact nearest-neighbour matching (k_knn.hip) -------------------------------------------------------------------

namespace {

int knn_args(pgx_ctx *c, int stride, int words, int M, int k)
{
    if (stride <= 0 || stride > (1 << PGX_IDX_BITS)) return fail(c, PGX_E_BADARG, "stride must be in [1, 2^20]");
    if (words <= 0 || words > 127) return fail(c, PGX_E_BADARG, "words must be in [1, 127] (P <= 4064)");
    if (k != 1 && k != 2) return fail(c, PGX_E_BADARG, "k must be 1 or 2");
    if ((long long)M * ((stride + 255) / 256) > 0x7FFFFFFFll) return fail(c, PGX_E_BADARG, "too many image pairs for one call");
    return PGX_OK;
}

int clamp_max_count(int max_count, int stride) { return max_count > stride ? stride : (max_count < 1 ? 1 : max_count); }

// The NN list of every row of M image pairs (pgx_match_nn_batch_dev, pgx_match_guided_batch_dev), in chunks of
// pgx_set_match_chunk pairs: produce(m0, n, max_n, idx, dist, col) enqueues the top-2 and column nearest of the pairs
// [m0, m0 + n) into ws_knn (20 bytes per slot) and returns PGX_OK or its error; the shared selection follows it.
extern "C++" template <class Produce>
int enqueue_select(pgx_ctx *c, const int32_t *d_counts, int stride, const int32_t *d_pairlist, int M, int max_count, int max_dist,
                   float ratio, int cross_check, pgx_pair *d_out, Produce &&produce)
{
    if (!(ratio <= 1.0f)) return fail(c, PGX_E_BADARG, "ratio must be <= 1 (0 or less: no ratio test)");
    if (M == 0) return PGX_OK;
    const int max_n = clamp_max_count(max_count, stride);
    const int CHUNK = c->match_chunk, mc = M < CHUNK ? M : CHUNK;
    const size_t slots = (size_t)mc * stride;
    HIPCHK(c, c->ws_knn.ensure(slots * 5 * sizeof(int32_t)));
    int32_t *idx = c->ws_knn.as<int32_t>(), *dist = idx + 2 * slots, *col = dist + 2 * slots;
    for (int m0 = 0; m0 < M; m0 += CHUNK) {
        const int n = M - m0 < CHUNK ? M - m0 : CHUNK;
        const int rp = produce(m0, n, max_n, idx, dist, col);
        if (rp != PGX_OK) return rp;
        pgx_launch_knn_select(c, c->stream, d_counts, d_pairlist + 2 * (size_t)m0, n, stride, max_n, idx, dist, col, max_dist, ratio,
                              cross_check ? 1 : 0, d_out + (size_t)m0 * stride);
    }
    HIPCHK(c, hipGetLastError());
    return PGX_OK;
}

} // namespace

int pgx_knn_batch_dev(pgx_ctx *c, const uint32_t *d_desc, const int32_t *d_counts, int stride, int words, const int32_t *d_pairlist,
                      int M, int max_count, int k, int32_t *d_idx, int32_t *d_dist, int32_t *d_col_nn)
{
    if (!c || !d_desc || !d_counts || !d_pairlist || !d_idx || !d_dist || M < 0)
        return c ? fail(c, PGX_E_BADARG, "null pointer") : PGX_E_BADARG;
    Lock l(c);
    const int rc = knn_args(c, stride, words, M, k);
    if (rc != PGX_OK || M == 0) return rc;
    pgx_launch_knn(c, c->stream, d_desc, d_counts, d_pairlist, M, stride, words, clamp_max_count(max_count, stride), k, d_idx, d_dist,
                   d_col_nn);
    HIPCHK(c, hipGetLastError());
    return PGX_OK;
}

int pgx_match_nn_batch_dev(pgx_ctx *c, const uint32_t *d_desc, const int32_t *d_counts, int stride, int words,
                           const int32_t *d_pairlist, int M, int max_count, int max_dist, float ratio, int cross_check, pgx_pair *d_out)
{
    if (!c || !d_desc || !d_counts || !d_pairlist || !d_out || M < 0)
        return c ? fail(c, PGX_E_BADARG, "null pointer") : PGX_E_BADARG;
    Lock l(c);
    const int rc = knn_args(c, stride, words, M, 2);
    if (rc != PGX_OK) return rc;
    return enqueue_select(c, d_counts, stride, d_pairlist, M, max_count, max_dist, ratio, cross_check, d_out,
                          [&](int m0, int n, int max_n, int32_t *idx, int32_t *dist, int32_t *col) {
                              pgx_launch_knn(c, c->stream, d_desc, d_counts, d_pairlist + 2 * (size_t)m0, n, stride, words, max_n, 2, idx,
                                             dist, col);
                              return PGX_OK;
                          });
}

int pgx_knn(pgx_ctx *c, const uint32_t *desc1, int n1, const uint32_t *desc2, int n2, int words, int k, int32_t *idx_out,
            int32_t *dist_out, int32_t *col_nn_out)
{
    if (!c || n1 < 0 || n2 < 0 || (n1 > 0 && (!desc1 || !idx_out || !dist_out)) || (n2 > 0 && !desc2))
        return c ? fail(c, PGX_E_BADARG, "null pointer") : PGX_E_BADARG;
    Lock l(c);
    const int S = n1 > n2 ? n1 : (n2 > 0 ? n2 : 1);
    if (S > (1 << PGX_IDX_BITS)) return fail(c, PGX_E_BADARG, "more than 2^20 keypoints");
    int rc = knn_args(c, S, words, 1, k);
    if (rc != PGX_OK) return rc;
    if (n1 == 0 && (n2 == 0 || !col_nn_out)) return PGX_OK;
    HostImage in, ot;
    const TwoSetsIn i = two_sets_in(in, desc1, nullptr, n1, desc2, nullptr, n2, S, words, nullptr);
    const KnnOut o = knn_out(ot, n1, n2, S, k, idx_out, dist_out, col_nn_out);
    if ((rc = stage_images(c, in, ot)) != PGX_OK) return rc;
    const int32_t *d_meta = in.dev<int32_t>(i.meta);
    pgx_launch_knn(c, c->stream, in.dev<uint32_t>(i.desc), d_meta, d_meta + 2, 1, S, words, S, k, ot.dev<int32_t>(o.idx),
                   ot.dev<int32_t>(o.dist), ot.dev<int32_t>(o.col));
    HIPCHK(c, hipGetLastError());
    return download_images(c, ot);
}

// ---- epipolar-guided exact matching (k_guided.hip) ------------------------------------------------------------------

namespace {

int guided_args(pgx_ctx *c, int stride, int words, int M, int k, float band)
{
    const int rc = knn_args(c, stride, words, M, k);
    if (rc != PGX_OK) return rc;
    if (!std::isfinite(band) || band < 0.f) return fail(c, PGX_E_BADARG, "band must be finite and >= 0");
    return PGX_OK;
}

// the guided top-k (and column nearest) of M image pairs, in chunks of pgx_set_match_chunk pairs that share one grid workspace
int enqueue_guided(pgx_ctx *c, const uint32_t *d_desc, const pgx_keypoint *d_kp, const int32_t *d_counts, int stride, int words,
                   const int32_t *d_pairlist, int M, int max_n, const float *d_F, float band, int k, int32_t *d_idx, int32_t *d_dist,
                   int32_t *d_col)
{
    const int CHUNK = c->match_chunk, mc = M < CHUNK ? M : CHUNK;
    HIPCHK(c, c->ws_guided.ensure(pgx_guided_ws_bytes(mc, max_n)));
    for (int m0 = 0; m0 < M; m0 += CHUNK) {
        const int n = M - m0 < CHUNK ? M - m0 : CHUNK;
        const size_t o = (size_t)m0 * stride;
        pgx_launch_guided(c, c->stream, d_desc, d_kp, d_counts, d_pairlist + 2 * (size_t)m0, n, stride, words, max_n, d_F + 9 * (size_t)m0,
                          band, k, d_idx + o * k, d_dist + o * k, d_col ? d_col + o : nullptr, c->ws_guided.p, c->d_status);
    }
    HIPCHK(c, hipGetLastError());
    return PGX_OK;
}

} // namespace

int pgx_knn_guided_batch_dev(pgx_ctx *c, const uint32_t *d_desc, const pgx_keypoint *d_kp, const int32_t *d_counts, int stride, int words,
                             const int32_t *d_pairlist, int M, int max_count, const float *d_F, float band, int k, int32_t *d_idx,
                             int32_t *d_dist, int32_t *d_col_nn)
{
    if (!c || !d_desc || !d_kp || !d_counts || !d_pairlist || !d_F || !d_idx || !d_dist || M < 0)
        return c ? fail(c, PGX_E_BADARG, "null pointer") : PGX_E_BADARG;
    Lock l(c);
    const int rc = guided_args(c, stride, words, M, k, band);
    if (rc != PGX_OK || M == 0) return rc;
    return enqueue_guided(c, d_desc, d_kp, d_counts, stride, words, d_pairlist, M, clamp_max_count(max_count, stride), d_F, band, k, d_idx,
                          d_dist, d_col_nn);
}

int pgx_match_guided_batch_dev(pgx_ctx *c, const uint32_t *d_desc, const pgx_keypoint *d_kp, const int32_t *d_counts, int stride,
                               int words, const int32_t *d_pairlist, int M, int max_count, const float *d_F, float band, int max_dist,
                               float ratio, int cross_check, pgx_pair *d_out)
{
    if (!c || !d_desc || !d_kp || !d_counts || !d_pairlist || !d_F || !d_out || M < 0)
        return c ? fail(c, PGX_E_BADARG, "null pointer") : PGX_E_BADARG;
    Lock l(c);
    const int rc = guided_args(c, stride, words, M, 2, band);
    if (rc != PGX_OK) return rc;
    return enqueue_select(c, d_counts, stride, d_pairlist, M, max_count, max_dist, ratio, cross_check, d_out,
                          [&](int m0, int n, int max_n, int32_t *idx, int32_t *dist, int32_t *col) {
                              return enqueue_guided(c, d_desc, d_kp, d_counts, stride, words, d_pairlist + 2 * (size_t)m0, n, max_n,
                                                    d_F + 9 * (size_t)m0, band, 2, idx, dist, col);
                          });
}

int pgx_knn_guided(pgx_ctx *c, const uint32_t *desc1, const pgx_keypoint *kp1, int n1, const uint32_t *desc2, const pgx_keypoint *kp2,
                   int n2, int words, const float *F, float band, int k, int32_t *idx_out, int32_t *dist_out, int32_t *col_nn_out)
{
    if (!c || !F || n1 < 0 || n2 < 0 || (n1 > 0 && (!desc1 || !kp1 || !idx_out || !dist_out)) || (n2 > 0 && (!desc2 || !kp2)))
        return c ? fail(c, PGX_E_BADARG, "null pointer") : PGX_E_BADARG;
    Lock l(c);
    const int S = n1 > n2 ? n1 : (n2 > 0 ? n2 : 1);
    if (S > (1 << PGX_IDX_BITS)) return fail(c, PGX_E_BADARG, "more than 2^20 keypoints");
    const int rc = guided_args(c, S, words, 1, k, band);
    if (rc != PGX_OK) return rc;
    if (n1 == 0 && (n2 == 0 || !col_nn_out)) return PGX_OK;
    HostImage in, ot;
    const TwoSetsIn i = two_sets_in(in, desc1, kp1, n1, desc2, kp2, n2, S, words, F);
    const KnnOut o = knn_out(ot, n1, n2, S, k, idx_out, dist_out, col_nn_out);
    if (const int rs = stage_images(c, in, ot); rs != PGX_OK) return rs;
    const int32_t *d_meta = in.dev<int32_t>(i.meta);
    const int rq = enqueue_guided(c, in.dev<uint32_t>(i.desc), in.dev<pgx_keypoint>(i.kp), d_meta, S, words, d_meta + 2, 1, S,
                                  in.dev<float>(i.F), band, k, ot.dev<int32_t>(o.idx), ot.dev<int32_t>(o.dist), ot.dev<int32_t>(o.col));
    if (rq != PGX_OK) return rq;
    return download_images(c, ot);
}

// ---- RANSAC fundamental matrix and pose ----------------------------------------------------------

int pgx_fundamental_ransac_dev(pgx_ctx *c, const pgx_keypoint *d_kp, const pgx_pair *d_matches, const int32_t *d_counts,
                               const int32_t *d_pairlist, int M, int stride, int n_samples, int pairs_per_sample,
                               float threshold, int rank_check, uint64_t seed, float *d_F, int32_t *d_inliers,
                               int32_t *d_best_sample)
{
    if (!c || !d_kp || !d_matches || !d_counts || !d_pairlist || !d_F || !d_inliers || !d_best_sample || M < 0 || stride <= 0)
        return c ? fail(c, PGX_E_BADARG, "null pointer") : PGX_E_BADARG;
    Lock l(c);
    if (pairs_per_sample < 8) // CameraPoseEstimation.cs:28-29
        return fail(c, PGX_E_BADARG, "At least 8 keypoint pairs must be included per sample (InvalidOperationException)");
    if (pairs_per_sample > 64 || n_samples <= 0 || n_samples > 65535 * 64)
        return fail(c, PGX_E_BADARG, "pairs_per_sample must be <= 64 and n_samples in [1, 4194240]");
    if (M == 0) return PGX_OK;
    HIPCHK(c, c->ws_pose.ensure(pgx_pose_ws_bytes(M, n_samples)));
    pgx_launch_fundamental(c->stream, d_kp, d_matches, d_counts, d_pairlist, M, stride, n_samples, pairs_per_sample, threshold,
                           rank_check, seed, c->ws_pose.p, d_F, d_inliers, d_best_sample);
    HIPCHK(c, hipGetLastError());
    return PGX_OK;
}

int pgx_pose_dev(pgx_ctx *c, const pgx_keypoint *d_kp, const pgx_pair *d_matches, const int32_t *d_counts,
                 const int32_t *d_pairlist, int M, int stride, const float *d_F, float *d_Rt, int32_t *d_votes,
                 int32_t *d_best, float *d_points)
{
    if (!c || !d_kp || !d_matches || !d_counts || !d_pairlist || !d_F || !d_Rt || !d_votes || !d_best || M < 0 || stride <= 0)
        return c ? fail(c, PGX_E_BADARG, "null pointer") : PGX_E_BADARG;
    Lock l(c);
    pgx_launch_pose(c->stream, d_kp, d_matches, d_counts, d_pairlist, M, stride, d_F, d_Rt, d_votes, d_best, d_points);
    HIPCHK(c, hipGetLastError());
    return PGX_OK;
}

// ---- the track graph on the device ---------------------------------------------------------------

namespace {
// the argument checks that the device forms of the track graph and of its consumers share
int geom_dev_args(pgx_ctx *c, int F, int stride, int n_frames, const int32_t *d_frame_ids, int max_tracks)
{
    if (F <= 0 || stride <= 0 || n_frames <= 0) return fail(c, PGX_E_BADARG, "F, stride and n_frames must be positive");
    if (!d_frame_ids && n_frames != F) return fail(c, PGX_E_BADARG, "without d_frame_ids, n_frames must equal F");
    if ((long long)n_frames * stride > (1ll << 30)) return fail(c, PGX_E_BADARG, "n_frames * stride must be <= 2^30");
    if (max_tracks < 0) return fail(c, PGX_E_BADARG, "max_tracks must be >= 0");
    return PGX_OK;
}

// ... and those of pgx_tracks_dev and pgx_tracks_split_dev (no track limit; one block per 256 slots of a pair and of a frame)
int tracks_dev_args(pgx_ctx *c, int M, int F, int stride, int n_frames, const int32_t *d_frame_ids)
{
    const int rc = geom_dev_args(c, F, stride, n_frames, d_frame_ids, 0);
    if (rc != PGX_OK) return rc;
    if ((long long)M * ((stride + 255) / 256) > 0x7FFFFFFFll || (long long)F * ((stride + 255) / 256) > 0x7FFFFFFFll)
        return fail(c, PGX_E_BADARG, "too many image pairs for one call");
    return PGX_OK;
}
} // namespace

int pgx_tracks_dev(pgx_ctx *c, const pgx_pair *d_matches, const int32_t *d_counts, const int32_t *d_pairlist, int M, int F,
                   int stride, const int32_t *d_frame_ids, int n_frames, int max_dist, int min_len, int32_t *d_track_of,
                   int32_t *d_offsets, int32_t *d_nodes, int32_t *d_summary)
{
    if (!c || !d_counts || !d_track_of || !d_offsets || !d_nodes || !d_summary || M < 0 || (M > 0 && (!d_matches || !d_pairlist)))
        return c ? fail(c, PGX_E_BADARG, "null pointer") : PGX_E_BADARG;
    Lock l(c);
    const int rc = tracks_dev_args(c, M, F, stride, n_frames, d_frame_ids);
    if (rc != PGX_OK) return rc;
    HIPCHK(c, c->ws_tracks.ensure(pgx_tracks_ws_bytes(n_frames, stride)));
    {
        ProfScope ps(c, "tracks");
        pgx_launch_tracks(c->stream, d_matches, d_counts, d_pairlist, M, F, stride, d_frame_ids, n_frames, max_dist, min_len,
                          c->ws_tracks.p, d_track_of, d_offsets, d_nodes, d_summary);
    }
    HIPCHK(c, hipGetLastError());
    return PGX_OK;
}

int pgx_tracks_split_dev(pgx_ctx *c, const pgx_pair *d_matches, const int32_t *d_counts, const int32_t *d_pairlist, int M, int F,
                         int stride, const int32_t *d_frame_ids, int n_frames, int max_dist, const int32_t *gates, int n_gates,
                         int min_len, int32_t *d_track_of, int32_t *d_offsets, int32_t *d_nodes, int32_t *d_summary)
{
    if (!c || !d_counts || !d_track_of || !d_offsets || !d_nodes || !d_summary || M < 0 || (M > 0 && (!d_matches || !d_pairlist)) ||
        (n_gates > 0 && !gates))
        return c ? fail(c, PGX_E_BADARG, "null pointer") : PGX_E_BADARG;
    Lock l(c);
    const int rc = tracks_dev_args(c, M, F, stride, n_frames, d_frame_ids);
    if (rc != PGX_OK) return rc;
    if (n_gates < 0 || n_gates > 7) return fail(c, PGX_E_BADARG, "n_gates = %d, must be in [0, 7]", n_gates);
    int g[7];
    for (int i = 0; i < n_gates; i++) {
        g[i] = gates[i];
        const int above = i == 0 ? max_dist : g[i - 1];
        if (g[i] < 0 || g[i] >= above)
            return fail(c, PGX_E_BADARG, "gates[%d] = %d: the gates must be >= 0, below max_dist (%d) and strictly decreasing", i, g[i],
                        max_dist);
    }
    HIPCHK(c, c->ws_tracks_split.ensure(pgx_tracks_split_ws_bytes(n_frames, stride)));
    {
        ProfScope ps(c, "tracks_split");
        pgx_launch_tracks_split(c->stream, d_matches, d_counts, d_pairlist, M, F, stride, d_frame_ids, n_frames, max_dist, g, n_gates,
                                min_len, c->ws_tracks_split.p, d_track_of, d_offsets, d_nodes, d_summary, c->d_status);
    }
    HIPCHK(c, hipGetLastError());
    return PGX_OK;
}

// ---- the consumers of the track graph: triangulation, bundle adjustment, frame registration --------------------------

namespace {
// the host forms' checks of counts, offsets and nodes (the device then sees no out-of-range node); stride = max(counts, 1)
int check_host_tracks(pgx_ctx *c, const pgx_keypoint *kps, const int32_t *counts, int n_frames, const int32_t *track_offsets,
                      const int32_t *nodes, int n_tracks, HostTracks *out)
{
    long long n_kp = 0;
    int stride = 1;
    for (int f = 0; f < n_frames; f++) {
        if (counts[f] < 0) return fail(c, PGX_E_BADARG, "counts[%d] = %d is negative", f, counts[f]);
        n_kp += counts[f];
        stride = counts[f] > stride ? counts[f] : stride;
    }
    if (n_kp > 0 && !kps) return fail(c, PGX_E_BADARG, "null pointer (kps)");
    if ((long long)n_frames * stride > (1ll << 30)) return fail(c, PGX_E_BADARG, "n_frames * max(counts) must be <= 2^30");
    if (track_offsets[0] != 0) return fail(c, PGX_E_BADARG, "track_offsets[0] must be 0");
    for (int t = 0; t < n_tracks; t++)
        if (track_offsets[t + 1] < track_offsets[t]) return fail(c, PGX_E_BADARG, "track_offsets decrease at track %d", t);
    const long long n_nodes = track_offsets[n_tracks];
    if (n_nodes > 0 && !nodes) return fail(c, PGX_E_BADARG, "null pointer (nodes)");
    for (long long o = 0; o < n_nodes; o++) {
        const int f = nodes[2 * o], k = nodes[2 * o + 1];
        if (f < 0 || f >= n_frames || k < 0 || k >= counts[f])
            return fail(c, PGX_E_BADARG, "node %lld = (%d, %d) is outside [0, n_frames) x [0, counts[frame])", o, f, k);
    }
    *out = {kps, counts, track_offsets, nodes, n_frames, n_tracks, stride, n_nodes};
    return PGX_OK;
}

// the range checks that the stages share: PGX_OK, or PGX_E_BADARG with the one text
int samples_ok(pgx_ctx *c, int n) { return n < 1 || n > 65536 ? fail(c, PGX_E_BADARG, "n_samples = %d, must be in [1, 65536]", n) : PGX_OK; }
int inlier_px_ok(pgx_ctx *c, double px) { return px > 0.0 && std::isfinite(px) ? PGX_OK : fail(c, PGX_E_BADARG, "inlier_px must be finite and > 0"); }
int iters_ok(pgx_ctx *c, const char *name, int n, int most)
{
    return n < 0 || n > most ? fail(c, PGX_E_BADARG, "%s = %d, must be in [0, %d]", name, n, most) : PGX_OK;
}
int pairs_ok(pgx_ctx *c, int M, int stride)
{
    if (M < 0) return fail(c, PGX_E_BADARG, "M = %d, must be >= 0", M);
    return stride < 1 || stride > (1 << PGX_IDX_BITS) ? fail(c, PGX_E_BADARG, "stride must be in [1, 2^20]") : PGX_OK;
}

int tri_args(pgx_ctx *c, double min_parallax_deg, double max_reproj_px, int refine_iters)
{
    if (iters_ok(c, "refine_iters", refine_iters, 32) != PGX_OK) return PGX_E_BADARG;
    if (!(min_parallax_deg >= 0.0)) return fail(c, PGX_E_BADARG, "min_parallax_deg must be >= 0 (and not NaN)");
    if (!(max_reproj_px > 0.0)) return fail(c, PGX_E_BADARG, "max_reproj_px must be > 0 (and not NaN; +inf disables the test)");
    return PGX_OK;
}

int ba_args(pgx_ctx *c, int max_iters, double huber_px, double lambda0)
{
    if (iters_ok(c, "max_iters", max_iters, 100) != PGX_OK) return PGX_E_BADARG;
    if (!(huber_px > 0.0)) return fail(c, PGX_E_BADARG, "huber_px must be > 0 (and not NaN; +inf is plain least squares)");
    if (!(lambda0 > 0.0) || !std::isfinite(lambda0)) return fail(c, PGX_E_BADARG, "lambda0 must be finite and > 0");
    return PGX_OK;
}

int reg_args(pgx_ctx *c, int n_samples, double inlier_px, int min_inliers, int refine_iters)
{
    if (samples_ok(c, n_samples) != PGX_OK || inlier_px_ok(c, inlier_px) != PGX_OK) return PGX_E_BADARG;
    if (min_inliers < 3) return fail(c, PGX_E_BADARG, "min_inliers = %d, must be >= 3", min_inliers);
    return iters_ok(c, "refine_iters", refine_iters, 32);
}

// *cos2 = the square of the cosine of min_parallax_deg
int cns_args(pgx_ctx *c, double inlier_px, double min_parallax_deg, int min_inliers, int max_hyp, double *cos2)
{
    if (inlier_px_ok(c, inlier_px) != PGX_OK) return PGX_E_BADARG;
    if (!(min_parallax_deg >= 0.0 && min_parallax_deg < 90.0)) return fail(c, PGX_E_BADARG, "min_parallax_deg must be in [0, 90)");
    if (min_inliers < 2) return fail(c, PGX_E_BADARG, "min_inliers = %d, must be >= 2", min_inliers);
    if (max_hyp < 1 || max_hyp > 4096) return fail(c, PGX_E_BADARG, "max_hyp = %d, must be in [1, 4096]", max_hyp);
    const double cs = std::cos(min_parallax_deg * M_PI / 180.0);
    *cos2 = cs * cs;
    return PGX_OK;
}

int ver_args(pgx_ctx *c, int M, int stride, int n_samples, double inlier_px, int min_inliers, int refit_iters)
{
    if (pairs_ok(c, M, stride) != PGX_OK || samples_ok(c, n_samples) != PGX_OK || inlier_px_ok(c, inlier_px) != PGX_OK) return PGX_E_BADARG;
    if (min_inliers < 8) return fail(c, PGX_E_BADARG, "min_inliers = %d, must be >= 8", min_inliers);
    return iters_ok(c, "refit_iters", refit_iters, 8);
}

// ---- one body per stage: a stage's arguments are its kernels' struct (pgx_stage_args.h), filled by name by the device form and
// the host form; run_X sizes the workspace from them, brackets the launch for the profile and picks up a launch error

int run_triangulate(pgx_ctx *c, TriArgs &a)
{
    a.status = c->d_status;
    HIPCHK(c, c->ws_tri.ensure(pgx_triangulate_ws_bytes(a)));
    {
        ProfScope ps(c, "triangulate");
        pgx_launch_triangulate(c->stream, a, c->ws_tri.p);
    }
    HIPCHK(c, hipGetLastError());
    return PGX_OK;
}

int run_bundle(pgx_ctx *c, BaArgs &a)
{
    a.status = c->d_status;
    HIPCHK(c, c->ws_ba.ensure(pgx_bundle_ws_bytes(a)));
    {
        ProfScope ps(c, "bundle");
        pgx_launch_bundle(c->stream, a, c->ws_ba.p);
    }
    HIPCHK(c, hipGetLastError());
    return PGX_OK;
}

int run_register(pgx_ctx *c, RegArgs &a)
{
    a.status = c->d_status;
    HIPCHK(c, c->ws_reg.ensure(pgx_register_ws_bytes(a)));
    {
        ProfScope ps(c, "register");
        pgx_launch_register(c->stream, a, c->ws_reg.p);
    }
    HIPCHK(c, hipGetLastError());
    return PGX_OK;
}

int run_consensus(pgx_ctx *c, CnsArgs &a)
{
    a.status = c->d_status;
    HIPCHK(c, c->ws_cns.ensure(pgx_consensus_ws_bytes(a)));
    {
        ProfScope ps(c, "consensus");
        pgx_launch_consensus(c, c->stream, a, c->ws_cns.p);
    }
    HIPCHK(c, hipGetLastError());
    return PGX_OK;
}

// the M pairs of a call (a's pointers are the first pair's) in chunks of pgx_set_match_chunk pairs that share ws_ver, then the report
int run_verify(pgx_ctx *c, VerArgs &a, int M, int32_t *d_report)
{
    const int CHUNK = c->match_chunk < 65535 ? c->match_chunk : 65535, mc = M < CHUNK ? M : CHUNK;
    const int chunk = pgx_verify_chunk(mc, a.n_samples);   // one value for every launch: a shorter last chunk of pairs fits too
    HIPCHK(c, c->ws_ver.ensure(pgx_verify_ws_bytes(mc, a.stride, a.n_samples, chunk)));
    {
        ProfScope ps(c, "verify");
        for (int m0 = 0; m0 < M; m0 += CHUNK) {
            const size_t o = (size_t)m0 * a.stride, os = (size_t)m0 * a.n_samples;
            VerArgs b = a;
            b.matches = a.matches + o;
            b.pairlist = a.pairlist + 2 * (size_t)m0;
            b.out = a.out + o;
            b.F = a.F + 9 * (size_t)m0;
            b.F32 = a.F32 ? a.F32 + 9 * (size_t)m0 : nullptr;
            b.stats = a.stats + 8 * (size_t)m0;
            b.inlier = a.inlier ? a.inlier + o : nullptr;
            b.sample_F = a.sample_F ? a.sample_F + 9 * os : nullptr;
            b.sample_count = a.sample_count ? a.sample_count + os : nullptr;
            pgx_launch_verify(c->stream, b, M - m0 < CHUNK ? M - m0 : CHUNK, chunk, c->ws_ver.p);
        }
        pgx_launch_verify_summary(c->stream, a.stats, M, d_report);
    }
    HIPCHK(c, hipGetLastError());
    return PGX_OK;
}

int run_init_pair(pgx_ctx *c, InitArgs &a)
{
    HIPCHK(c, c->ws_init.ensure(pgx_init_pair_ws_bytes(a)));
    {
        ProfScope ps(c, "init_pair");
        pgx_launch_init_pair(c->stream, a, c->ws_init.p);
    }
    HIPCHK(c, hipGetLastError());
    return PGX_OK;
}

// the dense stages' launchers bracket their own parts
int run_depth_maps(pgx_ctx *c, DepArgs &a, int agg_radius)
{
    HIPCHK(c, c->ws_depth.ensure(pgx_depth_ws_bytes(a)));
    pgx_launch_depth_maps(c, c->stream, a, agg_radius, c->ws_depth.p);
    HIPCHK(c, hipGetLastError());
    return PGX_OK;
}

int run_depth_fuse(pgx_ctx *c, FuseArgs &a)
{
    a.status = c->d_status;
    HIPCHK(c, c->ws_depth.ensure(pgx_depth_fuse_ws_bytes(a)));
    pgx_launch_depth_fuse(c, c->stream, a, c->ws_depth.p);
    HIPCHK(c, hipGetLastError());
    return PGX_OK;
}

// the launcher brackets its own parts
int run_dense_views(pgx_ctx *c, DvwArgs &a)
{
    a.status = c->d_status;
    HIPCHK(c, c->ws_dviews.ensure(pgx_dense_views_ws_bytes(a)));
    pgx_launch_dense_views(c, c->stream, a, c->ws_dviews.p);
    HIPCHK(c, hipGetLastError());
    return PGX_OK;
}

// the launcher brackets its own parts
int run_cloud_merge(pgx_ctx *c, CloudArgs &a)
{
    a.status = c->d_status;
    HIPCHK(c, c->ws_cloud.ensure(pgx_cloud_ws_bytes(a)));
    pgx_launch_cloud_merge(c, c->stream, a, c->ws_cloud.p);
    HIPCHK(c, hipGetLastError());
    return PGX_OK;
}

// the launcher brackets its own parts; the workspace is sized before any launch
int run_mesh(pgx_ctx *c, MeshArgs &a)
{
    a.status = c->d_status;
    HIPCHK(c, c->ws_mesh.ensure(pgx_mesh_ws_bytes(a)));
    pgx_launch_mesh(c, c->stream, a, c->ws_mesh.p);
    HIPCHK(c, hipGetLastError());
    return PGX_OK;
}

// the launcher brackets its own parts; the workspace is sized before any launch
int run_mesh_clean(pgx_ctx *c, MeshCleanArgs &a)
{
    a.status = c->d_status;
    HIPCHK(c, c->ws_mclean.ensure(pgx_mesh_clean_ws_bytes(a)));
    pgx_launch_mesh_clean(c, c->stream, a, c->ws_mclean.p);
    HIPCHK(c, hipGetLastError());
    return PGX_OK;
}

// the launcher brackets its own parts; the workspace is sized before any launch
int run_mesh_decimate(pgx_ctx *c, MeshDecimateArgs &a)
{
    a.status = c->d_status;
    HIPCHK(c, c->ws_mdec.ensure(pgx_mesh_decimate_ws_bytes(a)));
    pgx_launch_mesh_decimate(c, c->stream, a, c->ws_mdec.p);
    HIPCHK(c, hipGetLastError());
    return PGX_OK;
}

// ---- the track graph as a stage sees it (inv: the launcher's)

// a device form's: an offset may reach every slot
TrackView dev_tracks(const pgx_keypoint *d_kp, int F, int stride, const int32_t *d_frame_ids, int n_frames, const int32_t *d_offsets,
                     const int32_t *d_nodes, const int32_t *d_track_summary, int max_tracks)
{
    TrackView tv{};
    tv.kp = d_kp; tv.frame_ids = d_frame_ids; tv.offsets = d_offsets; tv.nodes = d_nodes; tv.track_summary = d_track_summary;
    tv.F = F; tv.stride = stride; tv.n_frames = n_frames; tv.max_tracks = max_tracks; tv.node_cap = (long long)n_frames * stride;
    return tv;
}

// a host form's, out of its upload image: slot = frame, exactly the caller's tracks and nodes
TrackView host_tracks(const HostImage &in, const TracksIn &i, const HostTracks &t, int n_tracks)
{
    TrackView tv{};
    tv.kp = in.dev<pgx_keypoint>(i.kp); tv.offsets = in.dev<int32_t>(i.off); tv.nodes = in.dev<int32_t>(i.nodes);
    tv.track_summary = in.dev<int32_t>(i.ts);
    tv.F = tv.n_frames = t.n_frames; tv.stride = t.stride; tv.max_tracks = n_tracks; tv.node_cap = t.n_nodes;
    return tv;
}
} // namespace

// ---- multi-view triangulation of tracks --------------------------------------------------------------------------

int pgx_triangulate_tracks_dev(pgx_ctx *c, const pgx_keypoint *d_kp, int F, int stride, const int32_t *d_frame_ids, int n_frames,
                               const double *d_P, const int32_t *d_offsets, const int32_t *d_nodes, const int32_t *d_track_summary,
                               int max_tracks, double min_parallax_deg, double max_reproj_px, int refine_iters, double *d_xyz,
                               double *d_quality, int32_t *d_flags, double *d_node_err, int32_t *d_summary)
{
    if (!c || !d_kp || !d_P || !d_offsets || !d_nodes || !d_track_summary || !d_xyz || !d_quality || !d_flags || !d_summary)
        return c ? fail(c, PGX_E_BADARG, "null pointer") : PGX_E_BADARG;
    Lock l(c);
    int rc = geom_dev_args(c, F, stride, n_frames, d_frame_ids, max_tracks);
    if (rc == PGX_OK) rc = tri_args(c, min_parallax_deg, max_reproj_px, refine_iters);
    if (rc != PGX_OK) return rc;
    TriArgs a{};
    a.tv = dev_tracks(d_kp, F, stride, d_frame_ids, n_frames, d_offsets, d_nodes, d_track_summary, max_tracks);
    a.P = d_P;
    a.refine_iters = refine_iters; a.min_par = min_parallax_deg; a.max_reproj = max_reproj_px;
    a.xyz = d_xyz; a.quality = d_quality; a.flags = d_flags; a.node_err = d_node_err; a.summary = d_summary;
    return run_triangulate(c, a);
}

int pgx_triangulate_tracks(pgx_ctx *c, const pgx_keypoint *kps, const int32_t *counts, int n_frames, const double *P,
                           const int32_t *track_offsets, const int32_t *nodes, int n_tracks, double min_parallax_deg,
                           double max_reproj_px, int refine_iters, double *xyz, double *quality, int32_t *flags, double *node_err,
                           int32_t *summary)
{
    if (!c || !counts || !P || !track_offsets || !summary || n_frames <= 0 || n_tracks < 0 ||
        (n_tracks > 0 && (!xyz || !quality || !flags)))
        return c ? fail(c, PGX_E_BADARG, "null pointer or bad size") : PGX_E_BADARG;
    Lock l(c);
    int rc = tri_args(c, min_parallax_deg, max_reproj_px, refine_iters);
    HostTracks t;
    if (rc == PGX_OK) rc = check_host_tracks(c, kps, counts, n_frames, track_offsets, nodes, n_tracks, &t);
    if (rc != PGX_OK) return rc;
    for (int i = 0; i < 8; i++) summary[i] = 0;
    if (n_tracks == 0) return PGX_OK;
    HostImage in, out;
    const TracksIn i = tracks_in(in, t, {P, nullptr, nullptr}, {96, 0, 0}, false, nullptr, nullptr);
    const int o_xyz = out.add(xyz, n_tracks, 24), o_q = out.add(quality, n_tracks, 24),
              o_err = out.add(node_err, t.n_nodes, 8, 1, node_err != nullptr), o_fl = out.add(flags, n_tracks, 4),
              o_sum = out.add(summary, 8, 4, 64);
    if ((rc = stage_images(c, in, out)) != PGX_OK) return rc;
    TriArgs a{};
    a.tv = host_tracks(in, i, t, n_tracks);
    a.P = in.dev<double>(i.frame[0]);
    a.refine_iters = refine_iters; a.min_par = min_parallax_deg; a.max_reproj = max_reproj_px;
    a.xyz = out.dev<double>(o_xyz); a.quality = out.dev<double>(o_q); a.flags = out.dev<int32_t>(o_fl);
    a.node_err = out.dev<double>(o_err); a.summary = out.dev<int32_t>(o_sum);
    if ((rc = run_triangulate(c, a)) != PGX_OK) return rc;
    return download_images(c, out);
}

// ---- bundle adjustment of cameras and track points ----------------------------------------------------------------

int pgx_bundle_adjust_dev(pgx_ctx *c, const pgx_keypoint *d_kp, int F, int stride, const int32_t *d_frame_ids, int n_frames,
                          const double *d_K, const double *d_Rt_in, const int32_t *d_fixed, const int32_t *d_offsets, const int32_t *d_nodes,
                          const int32_t *d_track_summary, int max_tracks, const double *d_xyz_in, const int32_t *d_track_flags,
                          int max_iters, double huber_px, double lambda0, double *d_Rt_out, double *d_P_out, double *d_xyz_out,
                          double *d_node_err, double *d_trace, int32_t *d_report)
{
    if (!c || !d_kp || !d_K || !d_Rt_in || !d_fixed || !d_offsets || !d_nodes || !d_track_summary || !d_xyz_in || !d_Rt_out ||
        !d_P_out || !d_xyz_out || !d_trace || !d_report)
        return c ? fail(c, PGX_E_BADARG, "null pointer") : PGX_E_BADARG;
    Lock l(c);
    int rc = geom_dev_args(c, F, stride, n_frames, d_frame_ids, max_tracks);
    if (rc == PGX_OK) rc = ba_args(c, max_iters, huber_px, lambda0);
    if (rc != PGX_OK) return rc;
    BaArgs a{};
    a.tv = dev_tracks(d_kp, F, stride, d_frame_ids, n_frames, d_offsets, d_nodes, d_track_summary, max_tracks);
    a.K = d_K; a.Rt_in = d_Rt_in; a.fixed = d_fixed; a.xyz_in = d_xyz_in; a.track_flags = d_track_flags;
    a.max_iters = max_iters; a.huber = huber_px; a.lambda0 = lambda0;
    a.Rt_out = d_Rt_out; a.P_out = d_P_out; a.xyz_out = d_xyz_out; a.node_err = d_node_err; a.trace = d_trace; a.report = d_report;
    return run_bundle(c, a);
}

int pgx_bundle_adjust(pgx_ctx *c, const pgx_keypoint *kps, const int32_t *counts, int n_frames, const double *K, const double *Rt_in,
                      const int32_t *fixed, const int32_t *track_offsets, const int32_t *nodes, int n_tracks, const double *xyz_in,
                      const int32_t *track_flags, int max_iters, double huber_px, double lambda0, double *Rt_out, double *P_out,
                      double *xyz_out, double *node_err, double *trace, int32_t *report)
{
    if (!c || !counts || !K || !Rt_in || !fixed || !track_offsets || !Rt_out || !P_out || !trace || !report || n_frames <= 0 ||
        n_tracks < 0 || (n_tracks > 0 && (!xyz_in || !xyz_out)))
        return c ? fail(c, PGX_E_BADARG, "null pointer or bad size") : PGX_E_BADARG;
    Lock l(c);
    int rc = ba_args(c, max_iters, huber_px, lambda0);
    HostTracks t;
    if (rc == PGX_OK) rc = check_host_tracks(c, kps, counts, n_frames, track_offsets, nodes, n_tracks, &t);
    if (rc != PGX_OK) return rc;
    HostImage in, out;
    const TracksIn i = tracks_in(in, t, {K, Rt_in, fixed}, {32, 96, 4}, true, xyz_in, track_flags);
    const int o_Rt = out.add(Rt_out, n_frames, 96), o_P = out.add(P_out, n_frames, 96), o_xyz = out.add(xyz_out, n_tracks, 24, 1),
              o_err = out.add(node_err, t.n_nodes, 8, 1, node_err != nullptr), o_tr = out.add(trace, max_iters + 1, 16),
              o_rep = out.add(report, 8, 4, 64);
    if ((rc = stage_images(c, in, out)) != PGX_OK) return rc;
    BaArgs a{};
    a.tv = host_tracks(in, i, t, n_tracks);
    a.K = in.dev<double>(i.frame[0]); a.Rt_in = in.dev<double>(i.frame[1]); a.fixed = in.dev<int32_t>(i.frame[2]);
    a.xyz_in = in.dev<double>(i.xyz); a.track_flags = in.dev<int32_t>(i.flags);
    a.max_iters = max_iters; a.huber = huber_px; a.lambda0 = lambda0;
    a.Rt_out = out.dev<double>(o_Rt); a.P_out = out.dev<double>(o_P); a.xyz_out = out.dev<double>(o_xyz);
    a.node_err = out.dev<double>(o_err); a.trace = out.dev<double>(o_tr); a.report = out.dev<int32_t>(o_rep);
    if ((rc = run_bundle(c, a)) != PGX_OK) return rc;
    return download_images(c, out);
}

// ---- frame registration by P3P RANSAC ------------------------------------------------------------------------------

int pgx_register_frames_dev(pgx_ctx *c, const pgx_keypoint *d_kp, int F, int stride, const int32_t *d_frame_ids, int n_frames,
                            const double *d_K, const double *d_Rt_in, const int32_t *d_register, const int32_t *d_offsets,
                            const int32_t *d_nodes, const int32_t *d_track_summary, int max_tracks, const double *d_xyz,
                            const int32_t *d_track_flags, int n_samples, double inlier_px, int min_inliers, int refine_iters,
                            uint64_t seed, double *d_Rt_out, double *d_P_out, int32_t *d_frame_stats, double *d_frame_err,
                            int32_t *d_node_inlier, int32_t *d_report)
{
    if (!c || !d_kp || !d_K || !d_Rt_in || !d_register || !d_offsets || !d_nodes || !d_track_summary || !d_xyz || !d_Rt_out ||
        !d_P_out || !d_frame_stats || !d_frame_err || !d_report)
        return c ? fail(c, PGX_E_BADARG, "null pointer") : PGX_E_BADARG;
    Lock l(c);
    int rc = geom_dev_args(c, F, stride, n_frames, d_frame_ids, max_tracks);
    if (rc == PGX_OK) rc = reg_args(c, n_samples, inlier_px, min_inliers, refine_iters);
    if (rc != PGX_OK) return rc;
    RegArgs a{};
    a.tv = dev_tracks(d_kp, F, stride, d_frame_ids, n_frames, d_offsets, d_nodes, d_track_summary, max_tracks);
    a.K = d_K; a.Rt_in = d_Rt_in; a.reg = d_register; a.xyz = d_xyz; a.track_flags = d_track_flags;
    a.n_samples = n_samples; a.inlier_px = inlier_px; a.min_inliers = min_inliers; a.refine_iters = refine_iters; a.seed = seed;
    a.Rt_out = d_Rt_out; a.P_out = d_P_out; a.frame_stats = d_frame_stats; a.frame_err = d_frame_err;
    a.node_inlier = d_node_inlier; a.report = d_report;
    return run_register(c, a);
}

int pgx_register_frames(pgx_ctx *c, const pgx_keypoint *kps, const int32_t *counts, int n_frames, const double *K, const double *Rt_in,
                        const int32_t *reg, const int32_t *track_offsets, const int32_t *nodes, int n_tracks, const double *xyz,
                        const int32_t *track_flags, int n_samples, double inlier_px, int min_inliers, int refine_iters, uint64_t seed,
                        double *Rt_out, double *P_out, int32_t *frame_stats, double *frame_err, int32_t *node_inlier, int32_t *report)
{
    if (!c || !counts || !K || !Rt_in || !reg || !track_offsets || !Rt_out || !P_out || !frame_stats || !frame_err || !report ||
        n_frames <= 0 || n_tracks < 0 || (n_tracks > 0 && !xyz))
        return c ? fail(c, PGX_E_BADARG, "null pointer or bad size") : PGX_E_BADARG;
    Lock l(c);
    int rc = reg_args(c, n_samples, inlier_px, min_inliers, refine_iters);
    HostTracks t;
    if (rc == PGX_OK) rc = check_host_tracks(c, kps, counts, n_frames, track_offsets, nodes, n_tracks, &t);
    if (rc != PGX_OK) return rc;
    HostImage in, out;
    const TracksIn i = tracks_in(in, t, {K, Rt_in, reg}, {32, 96, 4}, true, xyz, track_flags);
    const int o_Rt = out.add(Rt_out, n_frames, 96), o_P = out.add(P_out, n_frames, 96), o_st = out.add(frame_stats, n_frames, 16),
              o_er = out.add(frame_err, n_frames, 16), o_ni = out.add(node_inlier, t.n_nodes, 4, 1, node_inlier != nullptr),
              o_rep = out.add(report, 8, 4, 64);
    if ((rc = stage_images(c, in, out)) != PGX_OK) return rc;
    RegArgs a{};
    a.tv = host_tracks(in, i, t, n_tracks);
    a.K = in.dev<double>(i.frame[0]); a.Rt_in = in.dev<double>(i.frame[1]); a.reg = in.dev<int32_t>(i.frame[2]);
    a.xyz = in.dev<double>(i.xyz); a.track_flags = in.dev<int32_t>(i.flags);
    a.n_samples = n_samples; a.inlier_px = inlier_px; a.min_inliers = min_inliers; a.refine_iters = refine_iters; a.seed = seed;
    a.Rt_out = out.dev<double>(o_Rt); a.P_out = out.dev<double>(o_P); a.frame_stats = out.dev<int32_t>(o_st);
    a.frame_err = out.dev<double>(o_er); a.node_inlier = out.dev<int32_t>(o_ni); a.report = out.dev<int32_t>(o_rep);
    if ((rc = run_register(c, a)) != PGX_OK) return rc;
    return download_images(c, out);
}

// ---- track consensus: outlier observations dropped from tracks ------------------------------------------------------

int pgx_track_consensus_dev(pgx_ctx *c, const pgx_keypoint *d_kp, int F, int stride, const int32_t *d_frame_ids, int n_frames,
                            const double *d_P, const int32_t *d_offsets, const int32_t *d_nodes, const int32_t *d_track_summary,
                            int max_tracks, double inlier_px, double min_parallax_deg, int min_inliers, int min_len, int max_hyp,
                            uint64_t seed, int32_t *d_offsets_out, int32_t *d_nodes_out, int32_t *d_summary_out, int32_t *d_track_map,
                            double *d_xyz_out, int32_t *d_flags_out, int32_t *d_track_stats, int32_t *d_track_of, int32_t *d_report)
{
    if (!c || !d_kp || !d_P || !d_offsets || !d_nodes || !d_track_summary || !d_offsets_out || !d_nodes_out || !d_summary_out ||
        !d_track_map || !d_xyz_out || !d_flags_out || !d_track_stats || !d_report)
        return c ? fail(c, PGX_E_BADARG, "null pointer") : PGX_E_BADARG;
    Lock l(c);
    int rc = geom_dev_args(c, F, stride, n_frames, d_frame_ids, max_tracks);
    double cos2 = 0.0;
    if (rc == PGX_OK) rc = cns_args(c, inlier_px, min_parallax_deg, min_inliers, max_hyp, &cos2);
    if (rc != PGX_OK) return rc;
    if (d_offsets_out == d_offsets || d_nodes_out == d_nodes || d_summary_out == d_track_summary)
        return fail(c, PGX_E_BADARG, "the output graph must not alias the input graph");
    CnsArgs a{};
    a.tv = dev_tracks(d_kp, F, stride, d_frame_ids, n_frames, d_offsets, d_nodes, d_track_summary, max_tracks);
    a.P = d_P;
    a.inlier_px = inlier_px; a.cos2 = cos2; a.min_inliers = min_inliers; a.min_len = min_len; a.max_hyp = max_hyp; a.seed = seed;
    a.off_out = d_offsets_out; a.nodes_out = d_nodes_out; a.summary_out = d_summary_out; a.map = d_track_map;
    a.xyz_out = d_xyz_out; a.flags_out = d_flags_out; a.stats = d_track_stats; a.track_of = d_track_of; a.report = d_report;
    return run_consensus(c, a);
}

int pgx_track_consensus(pgx_ctx *c, const pgx_keypoint *kps, const int32_t *counts, int n_frames, const double *P,
                        const int32_t *track_offsets, const int32_t *nodes, int n_tracks, double inlier_px, double min_parallax_deg,
                        int min_inliers, int min_len, int max_hyp, uint64_t seed, int32_t *offsets_out, int32_t *nodes_out,
                        int32_t *summary_out, int32_t *track_map, double *xyz_out, int32_t *flags_out, int32_t *track_stats,
                        int32_t *report)
{
    if (!c || !counts || !P || !track_offsets || !offsets_out || !summary_out || !report || n_frames <= 0 || n_tracks < 0)
        return c ? fail(c, PGX_E_BADARG, "null pointer or bad size") : PGX_E_BADARG;
    Lock l(c);
    double cos2 = 0.0;
    int rc = cns_args(c, inlier_px, min_parallax_deg, min_inliers, max_hyp, &cos2);
    HostTracks t;
    if (rc == PGX_OK) rc = check_host_tracks(c, kps, counts, n_frames, track_offsets, nodes, n_tracks, &t);
    if (rc != PGX_OK) return rc;
    if (t.n_nodes > 0 && !nodes_out) return fail(c, PGX_E_BADARG, "null pointer (nodes_out)");
    if (offsets_out == track_offsets || (nodes_out && nodes_out == nodes))
        return fail(c, PGX_E_BADARG, "the output graph must not alias the input graph");
    for (int i = 0; i < 8; i++) summary_out[i] = report[i] = 0;
    offsets_out[0] = 0;
    if (n_tracks == 0) return PGX_OK;
    HostImage in, out;
    const TracksIn i = tracks_in(in, t, {P, nullptr, nullptr}, {96, 0, 0}, false, nullptr, nullptr);
    const int o_off = out.add(offsets_out, n_tracks + 1, 4), o_nd = out.add(nodes_out, t.n_nodes, 8, 1),
              o_sum = out.add(summary_out, 8, 4, 64), o_map = out.add(track_map, n_tracks, 4), o_xyz = out.add(xyz_out, n_tracks, 24),
              o_fl = out.add(flags_out, n_tracks, 4), o_st = out.add(track_stats, n_tracks, 16), o_rep = out.add(report, 8, 4, 64);
    if ((rc = stage_images(c, in, out)) != PGX_OK) return rc;
    CnsArgs a{};
    a.tv = host_tracks(in, i, t, n_tracks);
    a.P = in.dev<double>(i.frame[0]);
    a.inlier_px = inlier_px; a.cos2 = cos2; a.min_inliers = min_inliers; a.min_len = min_len; a.max_hyp = max_hyp; a.seed = seed;
    a.off_out = out.dev<int32_t>(o_off); a.nodes_out = out.dev<int32_t>(o_nd); a.summary_out = out.dev<int32_t>(o_sum);
    a.map = out.dev<int32_t>(o_map); a.xyz_out = out.dev<double>(o_xyz); a.flags_out = out.dev<int32_t>(o_fl);
    a.stats = out.dev<int32_t>(o_st); a.report = out.dev<int32_t>(o_rep);   // no track_of
    if ((rc = run_consensus(c, a)) != PGX_OK) return rc;
    return download_images(c, out);
}

// ---- binary visual vocabulary and image-pair selection ---------------------------------------------------------------

namespace {

int vocab_args(pgx_ctx *c, int F, int stride, int V)
{
    if (F < 1 || F > 4096) return fail(c, PGX_E_BADARG, "F must be in [1, 4096]");
    if (stride < 1 || stride > 65535) return fail(c, PGX_E_BADARG, "stride must be in [1, 65535]");
    if (V < 1 || V > 65536) return fail(c, PGX_E_BADARG, "V must be in [1, 65536]");
    return PGX_OK;
}

int train_args(pgx_ctx *c, int F, int stride, int V, int iters)
{
    if (const int rc = vocab_args(c, F, stride, V); rc != PGX_OK) return rc;
    if (iters < 0 || iters > 64) return fail(c, PGX_E_BADARG, "iters must be in [0, 64]");
    return PGX_OK;
}

int select_args(pgx_ctx *c, int F, int stride, int V, int weighting, int top_k, int window, int max_pairs)
{
    if (const int rc = vocab_args(c, F, stride, V); rc != PGX_OK) return rc;
    if (weighting != 0 && weighting != 1) return fail(c, PGX_E_BADARG, "weighting must be 0 or 1");
    if (top_k < 0 || window < 0 || max_pairs < 0) return fail(c, PGX_E_BADARG, "top_k, window and max_pairs must not be negative");
    return PGX_OK;
}

} // namespace

int pgx_vocab_quantize_dev(pgx_ctx *c, const uint32_t *d_desc, const int32_t *d_counts, int F, int stride, const uint32_t *d_vocab,
                           int V, int32_t *d_word, int32_t *d_wdist)
{
    if (!c || !d_desc || !d_counts || !d_vocab || !d_word) return c ? fail(c, PGX_E_BADARG, "null pointer") : PGX_E_BADARG;
    Lock l(c);
    if (const int rc = vocab_args(c, F, stride, V); rc != PGX_OK) return rc;
    pgx_launch_vocab_quantize(c, c->stream, d_desc, d_counts, F, stride, d_vocab, V, d_word, d_wdist);
    HIPCHK(c, hipGetLastError());
    return PGX_OK;
}

int pgx_vocab_train_dev(pgx_ctx *c, const uint32_t *d_desc, const int32_t *d_counts, int F, int stride, int V, int iters,
                        uint64_t seed, uint32_t *d_vocab, int32_t *d_report)
{
    if (!c || !d_desc || !d_counts || !d_vocab || !d_report) return c ? fail(c, PGX_E_BADARG, "null pointer") : PGX_E_BADARG;
    Lock l(c);
    if (const int rc = train_args(c, F, stride, V, iters); rc != PGX_OK) return rc;
    HIPCHK(c, c->ws_vocab.ensure(pgx_vocab_train_ws_bytes(F, stride, V)));
    pgx_launch_vocab_train(c, c->stream, d_desc, d_counts, F, stride, V, iters, seed, d_vocab, d_report, c->ws_vocab.p, c->d_status);
    HIPCHK(c, hipGetLastError());
    return PGX_OK;
}

int pgx_select_pairs_dev(pgx_ctx *c, const uint32_t *d_desc, const int32_t *d_counts, int F, int stride, const uint32_t *d_vocab, int V,
                         int weighting, int top_k, int window, int min_score, int max_pairs, int32_t *d_pairlist,
                         int32_t *d_pair_score, int32_t *d_scores, int32_t *d_summary)
{
    if (!c || !d_desc || !d_counts || !d_vocab || !d_summary || (max_pairs > 0 && (!d_pairlist || !d_pair_score)))
        return c ? fail(c, PGX_E_BADARG, "null pointer") : PGX_E_BADARG;
    Lock l(c);
    if (const int rc = select_args(c, F, stride, V, weighting, top_k, window, max_pairs); rc != PGX_OK) return rc;
    HIPCHK(c, c->ws_vocab.ensure(pgx_select_pairs_ws_bytes(F, stride, V, d_scores == nullptr)));
    pgx_launch_select_pairs(c, c->stream, d_desc, d_counts, F, stride, d_vocab, V, weighting, top_k, window, min_score, max_pairs,
                            d_pairlist, d_pair_score, d_scores, d_summary, c->ws_vocab.p, c->d_status);
    HIPCHK(c, hipGetLastError());
    return PGX_OK;
}

int pgx_vocab_train(pgx_ctx *c, const uint32_t *desc, const int32_t *counts, int F, int stride, int V, int iters, uint64_t seed,
                    uint32_t *vocab, int32_t *report)
{
    if (!c || !desc || !counts || !vocab || !report) return c ? fail(c, PGX_E_BADARG, "null pointer") : PGX_E_BADARG;
    Lock l(c);
    if (const int rc = train_args(c, F, stride, V, iters); rc != PGX_OK) return rc;
    long long N = 0;
    for (int f = 0; f < F; f++) N += counts[f] < 0 ? 0 : (counts[f] > stride ? stride : counts[f]);
    if (N < V) return fail(c, PGX_E_BADARG, "fewer valid descriptors (%lld) than words (%d)", N, V);
    HostImage in, out;
    const int i_desc = in.add(desc, (size_t)F * stride, 32), i_cnt = in.add(counts, F, 4);
    const int o_voc = out.add(vocab, V, 32), o_rep = out.add(report, 4, 4, 16);
    if (const int rs = stage_images(c, in, out); rs != PGX_OK) return rs;
    HIPCHK(c, c->ws_vocab.ensure(pgx_vocab_train_ws_bytes(F, stride, V)));
    pgx_launch_vocab_train(c, c->stream, in.dev<uint32_t>(i_desc), in.dev<int32_t>(i_cnt), F, stride, V, iters, seed,
                           out.dev<uint32_t>(o_voc), out.dev<int32_t>(o_rep), c->ws_vocab.p, c->d_status);
    HIPCHK(c, hipGetLastError());
    return download_images(c, out);
}

int pgx_select_pairs(pgx_ctx *c, const uint32_t *desc, const int32_t *counts, int F, int stride, const uint32_t *vocab, int V,
                     int weighting, int top_k, int window, int min_score, int max_pairs, int32_t *pairlist, int32_t *pair_score,
                     int32_t *scores, int32_t *summary)
{
    if (!c || !desc || !counts || !vocab || !summary || (max_pairs > 0 && (!pairlist || !pair_score)))
        return c ? fail(c, PGX_E_BADARG, "null pointer") : PGX_E_BADARG;
    Lock l(c);
    if (const int rc = select_args(c, F, stride, V, weighting, top_k, window, max_pairs); rc != PGX_OK) return rc;
    HostImage in, out;
    const int i_desc = in.add(desc, (size_t)F * stride, 32), i_cnt = in.add(counts, F, 4), i_voc = in.add(vocab, V, 32);
    const int o_pl = out.add(pairlist, max_pairs, 8, 1), o_ps = out.add(pair_score, max_pairs, 4, 1),
              o_sc = out.add(scores, (size_t)F * F, 4, 0, scores != nullptr), o_sum = out.add(summary, 8, 4, 16);
    if (const int rs = stage_images(c, in, out); rs != PGX_OK) return rs;
    HIPCHK(c, c->ws_vocab.ensure(pgx_select_pairs_ws_bytes(F, stride, V, scores == nullptr)));
    pgx_launch_select_pairs(c, c->stream, in.dev<uint32_t>(i_desc), in.dev<int32_t>(i_cnt), F, stride, in.dev<uint32_t>(i_voc), V,
                            weighting, top_k, window, min_score, max_pairs, out.dev<int32_t>(o_pl), out.dev<int32_t>(o_ps),
                            out.dev<int32_t>(o_sc), out.dev<int32_t>(o_sum), c->ws_vocab.p, c->d_status);
    HIPCHK(c, hipGetLastError());
    // the outputs travel even when the list was cut: PGX_E_CAPACITY leaves the first max_pairs pairs in the caller's buffers
    return download_images(c, out);
}

// ---- two-view verification by epipolar RANSAC ----------------------------------------------------------------------

int pgx_verify_pairs_dev(pgx_ctx *c, const pgx_keypoint *d_kp, const pgx_pair *d_matches, const int32_t *d_counts,
                         const int32_t *d_pairlist, int M, int stride, int max_dist, int n_samples, double inlier_px, int min_inliers,
                         int refit_iters, uint64_t seed, pgx_pair *d_out, double *d_F, float *d_F32, int32_t *d_stats,
                         int32_t *d_inlier, double *d_sample_F, int32_t *d_sample_count, int32_t *d_report)
{
    if (!c || !d_kp || !d_matches || !d_counts || !d_pairlist || !d_out || !d_F || !d_stats || !d_report)
        return c ? fail(c, PGX_E_BADARG, "null pointer") : PGX_E_BADARG;
    Lock l(c);
    const int rc = ver_args(c, M, stride, n_samples, inlier_px, min_inliers, refit_iters);
    if (rc != PGX_OK) return rc;
    VerArgs a{};
    a.kp = d_kp; a.matches = d_matches; a.counts = d_counts; a.pairlist = d_pairlist; a.stride = stride;
    a.max_dist = max_dist; a.n_samples = n_samples; a.inlier_px = inlier_px; a.min_inliers = min_inliers; a.refit_iters = refit_iters;
    a.seed = seed;
    a.out = d_out; a.F = d_F; a.F32 = d_F32; a.stats = d_stats; a.inlier = d_inlier;
    a.sample_F = d_sample_F; a.sample_count = d_sample_count;
    return run_verify(c, a, M, d_report);
}

int pgx_verify_pair(pgx_ctx *c, const pgx_keypoint *kp1, int n1, const pgx_keypoint *kp2, int n2, const pgx_pair *matches, int max_dist,
                    int n_samples, double inlier_px, int min_inliers, int refit_iters, uint64_t seed, pgx_pair *out, double *F,
                    int32_t *stats, int32_t *inlier)
{
    if (!c || !F || !stats || n1 < 0 || n2 < 0 || n1 > (1 << PGX_IDX_BITS) || n2 > (1 << PGX_IDX_BITS) ||
        (n1 > 0 && (!kp1 || !matches || !out)) || (n2 > 0 && !kp2))
        return c ? fail(c, PGX_E_BADARG, "null pointer or bad size") : PGX_E_BADARG;
    Lock l(c);
    const int S = n1 > n2 ? n1 : (n2 > 0 ? n2 : 1);
    const int rc = ver_args(c, 1, S, n_samples, inlier_px, min_inliers, refit_iters);
    if (rc != PGX_OK) return rc;
    HostImage in, ot;
    const PairIn i = pair_in(in, kp1, n1, kp2, n2, matches, S);
    // the report is the device form's: carved, not downloaded
    const int o_out = ot.add(out, n1, sizeof(pgx_pair), S), o_F = ot.add(F, 9, 8), o_st = ot.add(stats, 8, 4),
              o_in = ot.add(inlier, n1, 4, S, inlier != nullptr), o_rep = ot.add(nullptr, 0, 4, 8);
    if (const int rs = stage_images(c, in, ot); rs != PGX_OK) return rs;
    VerArgs a{};
    a.kp = in.dev<pgx_keypoint>(i.kp); a.matches = in.dev<pgx_pair>(i.list);
    a.counts = in.dev<int32_t>(i.meta); a.pairlist = a.counts + 3; a.stride = S;
    a.max_dist = max_dist; a.n_samples = n_samples; a.inlier_px = inlier_px; a.min_inliers = min_inliers; a.refit_iters = refit_iters;
    a.seed = seed;
    a.out = ot.dev<pgx_pair>(o_out); a.F = ot.dev<double>(o_F); a.stats = ot.dev<int32_t>(o_st); a.inlier = ot.dev<int32_t>(o_in);
    if (const int rq = run_verify(c, a, 1, ot.dev<int32_t>(o_rep)); rq != PGX_OK) return rq;
    return download_images(c, ot);
}

// ---- relative pose per image pair and the choice of the initial pair ------------------------------------------------

namespace {
// cos^2 of the angle gate through *cos2
int init_args(pgx_ctx *c, int M, int stride, double min_angle_deg, double min_front_frac, int min_points, double *cos2)
{
    if (pairs_ok(c, M, stride) != PGX_OK) return PGX_E_BADARG;
    if (!(min_angle_deg >= 0.0 && min_angle_deg < 90.0)) return fail(c, PGX_E_BADARG, "min_angle_deg must be in [0, 90) (and not NaN)");
    if (!(min_front_frac > 0.0 && min_front_frac <= 1.0)) return fail(c, PGX_E_BADARG, "min_front_frac must be in (0, 1] (and not NaN)");
    if (min_points < 1) return fail(c, PGX_E_BADARG, "min_points = %d, must be >= 1", min_points);
    const double cs = std::cos(min_angle_deg * (M_PI / 180));
    *cos2 = cs * cs;
    return PGX_OK;
}
} // namespace

int pgx_init_pair_dev(pgx_ctx *c, const pgx_keypoint *d_kp, const pgx_pair *d_matches, const int32_t *d_counts,
                      const int32_t *d_pairlist, int M, int F, int stride, const int32_t *d_frame_ids, int n_frames, int max_dist,
                      const double *d_F, const double *d_K, double min_angle_deg, double min_front_frac, int min_points,
                      double *d_Rt_pair, int32_t *d_pair_stats, double *d_sigma, double *d_cand_Rt, double *d_Rt_out, double *d_P_out,
                      int32_t *d_fixed_out, int32_t *d_register_out, int32_t *d_report)
{
    if (!c || !d_kp || !d_matches || !d_counts || !d_pairlist || !d_F || !d_K || !d_Rt_pair || !d_pair_stats || !d_Rt_out || !d_P_out ||
        !d_fixed_out || !d_register_out || !d_report)
        return c ? fail(c, PGX_E_BADARG, "null pointer") : PGX_E_BADARG;
    Lock l(c);
    double cos2 = 0.0;
    int rc = init_args(c, M, stride, min_angle_deg, min_front_frac, min_points, &cos2);
    if (rc == PGX_OK) rc = geom_dev_args(c, F, stride, n_frames, d_frame_ids, 0);
    if (rc != PGX_OK) return rc;
    InitArgs a{};
    a.kp = d_kp; a.matches = d_matches; a.counts = d_counts; a.pairlist = d_pairlist; a.frame_ids = d_frame_ids;
    a.F = d_F; a.K = d_K;
    a.M = M; a.nslots = F; a.stride = stride; a.n_frames = n_frames;
    a.max_dist = max_dist; a.cos2 = cos2; a.min_front_frac = min_front_frac; a.min_points = min_points;
    a.Rt_pair = d_Rt_pair; a.pair_stats = d_pair_stats; a.sigma = d_sigma; a.cand_Rt = d_cand_Rt;
    a.Rt_out = d_Rt_out; a.P_out = d_P_out; a.fixed_out = d_fixed_out; a.register_out = d_register_out; a.report = d_report;
    return run_init_pair(c, a);
}

int pgx_relative_pose(pgx_ctx *c, const pgx_keypoint *kp1, int n1, const pgx_keypoint *kp2, int n2, const pgx_pair *matches, int max_dist,
                      const double *F, const double *K_a, const double *K_b, double min_angle_deg, double min_front_frac,
                      int min_points, double *Rt, int32_t *stats, double *sigma, double *cand_Rt)
{
    if (!c || !F || !K_a || !K_b || !Rt || !stats || !sigma || n1 < 0 || n2 < 0 || n1 > (1 << PGX_IDX_BITS) ||
        n2 > (1 << PGX_IDX_BITS) || (n1 > 0 && (!kp1 || !matches)) || (n2 > 0 && !kp2))
        return c ? fail(c, PGX_E_BADARG, "null pointer or bad size") : PGX_E_BADARG;
    Lock l(c);
    const int S = n1 > n2 ? n1 : (n2 > 0 ? n2 : 1);
    double cos2 = 0.0;
    const int rc = init_args(c, 1, S, min_angle_deg, min_front_frac, min_points, &cos2);
    if (rc != PGX_OK) return rc;
    // the pair (1, 2) of three frames, then F [9] and K [3][4] by frame (row 0 unused)
    HostImage in, ot;
    const PairIn i = pair_in(in, kp1, n1, kp2, n2, matches, S);
    const int i_F = in.add(F, 9, 8), i_K = in.add(nullptr, 0, 32, 3);
    in.put_at(32, K_a, 32);
    in.put_at(64, K_b, 32);
    // carved, not downloaded: the frames' Rt_out then P_out [3][12], fixed_out [3] then, 8 words in, register_out [3], the report
    const int o_Rt = ot.add(Rt, 12, 8), o_st = ot.add(stats, 8, 4), o_sg = ot.add(sigma, 1, 8), o_cand = ot.add(cand_Rt, 48, 8, 0, cand_Rt != nullptr),
              o_fr = ot.add(nullptr, 0, 96, 2 * 3), o_fi = ot.add(nullptr, 0, 4, 2 * 3 + 16), o_rep = ot.add(nullptr, 0, 4, 8);
    if (const int rs = stage_images(c, in, ot); rs != PGX_OK) return rs;
    InitArgs a{};
    a.kp = in.dev<pgx_keypoint>(i.kp); a.matches = in.dev<pgx_pair>(i.list);
    a.counts = in.dev<int32_t>(i.meta); a.pairlist = a.counts + 3;
    a.F = in.dev<double>(i_F); a.K = in.dev<double>(i_K);
    a.M = 1; a.nslots = a.n_frames = 3; a.stride = S;
    a.max_dist = max_dist; a.cos2 = cos2; a.min_front_frac = min_front_frac; a.min_points = min_points;
    a.Rt_pair = ot.dev<double>(o_Rt); a.pair_stats = ot.dev<int32_t>(o_st); a.sigma = ot.dev<double>(o_sg);
    a.cand_Rt = ot.dev<double>(o_cand);
    a.Rt_out = ot.dev<double>(o_fr); a.P_out = a.Rt_out + 3 * 12;
    a.fixed_out = ot.dev<int32_t>(o_fi); a.register_out = a.fixed_out + 8; a.report = ot.dev<int32_t>(o_rep);
    if (const int rq = run_init_pair(c, a); rq != PGX_OK) return rq;
    return download_images(c, ot);
}

// ---- dense depth maps by census plane sweep, and the cross-view filter ------------------------------------------------

int pgx_gray_batch_dev(pgx_ctx *c, const uint16_t *d_rgba, int F, int W, int H, float *d_gray)
{
    if (!c || !d_rgba || !d_gray) return c ? fail(c, PGX_E_BADARG, "null pointer") : PGX_E_BADARG;
    Lock l(c);
    if (F <= 0) return fail(c, PGX_E_BADARG, "F must be positive");
    if (dims_ok(c, W, H) != PGX_OK) return PGX_E_BADARG;
    if (c->map_set && (W != c->mapW || H != c->mapH))
        return fail(c, PGX_E_DIM_MISMATCH, "image %dx%d vs dewarp map %dx%d (ArgumentException)", W, H, c->mapW, c->mapH);
    {
        ProfScope ps(c, "dewarp_gray");
        pgx_launch_dewarp_gray(c->stream, d_rgba, c->src8, c->map_set ? c->d_map.as<int32_t>() : nullptr, F, W, H, d_gray, nullptr,
                               c->d_status);
    }
    HIPCHK(c, hipGetLastError());
    return PGX_OK;
}

namespace {
// what the device and the host form of a stage check alike
int depth_args(pgx_ctx *c, int F, int W, int H, int n_frames, bool has_ids, int R, int S, int D, int agg_radius, int min_views, int max_cost)
{
    if (dims_ok(c, W, H) != PGX_OK) return PGX_E_BADARG;
    if (F <= 0 || F > 65535 || n_frames <= 0) return fail(c, PGX_E_BADARG, "F must be in [1, 65535] and n_frames positive");
    if (!has_ids && n_frames != F) return fail(c, PGX_E_BADARG, "without d_frame_ids, n_frames must equal F");
    if (R < 0 || R > 65535) return fail(c, PGX_E_BADARG, "R must be in [0, 65535]");
    if (D < 3 || D > 256) return fail(c, PGX_E_BADARG, "D = %d, must be in [3, 256]", D);
    if (S < 1 || S > 8) return fail(c, PGX_E_BADARG, "S = %d, must be in [1, 8]", S);
    if (agg_radius < 0 || agg_radius > 3) return fail(c, PGX_E_BADARG, "agg_radius = %d, must be in [0, 3]", agg_radius);
    if (min_views < 1 || min_views > S) return fail(c, PGX_E_BADARG, "min_views = %d, must be in [1, S]", min_views);
    if (max_cost < 0) return fail(c, PGX_E_BADARG, "max_cost must be >= 0");
    if ((long long)(R > F ? R : F) * W * H > (1ll << 30)) return fail(c, PGX_E_BADARG, "max(F, R) * W * H must be <= 2^30");
    return PGX_OK;
}

int fuse_args(pgx_ctx *c, int R, int S, int W, int H, int n_frames, double rel_tol, int min_agree, int max_points)
{
    if (dims_ok(c, W, H) != PGX_OK) return PGX_E_BADARG;
    if (R < 0 || R > 65535 || n_frames <= 0) return fail(c, PGX_E_BADARG, "R must be in [0, 65535] and n_frames positive");
    if (S < 1 || S > 8) return fail(c, PGX_E_BADARG, "S = %d, must be in [1, 8]", S);
    if (!(rel_tol >= 0.0) || std::isinf(rel_tol)) return fail(c, PGX_E_BADARG, "rel_tol must be finite and >= 0");
    if (min_agree < 0 || max_points < 0) return fail(c, PGX_E_BADARG, "min_agree and max_points must be >= 0");
    if ((long long)R * W * H > (1ll << 30)) return fail(c, PGX_E_BADARG, "R * W * H must be <= 2^30");
    return PGX_OK;
}
} // namespace

int pgx_depth_maps_dev(pgx_ctx *c, const float *d_gray, int F, int W, int H, const int32_t *d_frame_ids, int n_frames, const double *d_P,
                       const int32_t *d_views, int R, int S, const double *d_range, int D, int agg_radius, int min_views, int max_cost,
                       int32_t *d_kq8, double *d_depth, int32_t *d_cost, int32_t *d_flags, double *d_warp, double *d_planes,
                       int32_t *d_summary)
{
    if (!c || !d_gray || !d_P || !d_views || !d_range || !d_kq8 || !d_depth || !d_flags || !d_summary)
        return c ? fail(c, PGX_E_BADARG, "null pointer") : PGX_E_BADARG;
    Lock l(c);
    const int rc = depth_args(c, F, W, H, n_frames, d_frame_ids != nullptr, R, S, D, agg_radius, min_views, max_cost);
    if (rc != PGX_OK) return rc;
    if (R == 0) return fail(c, PGX_E_BADARG, "R must be positive");
    DepArgs a{};
    a.gray = d_gray; a.F = F; a.W = W; a.H = H; a.frame_ids = d_frame_ids; a.n_frames = n_frames; a.P = d_P;
    a.views = d_views; a.R = R; a.S = S; a.range = d_range; a.D = D; a.min_views = min_views; a.max_cost = max_cost;
    a.kq8 = d_kq8; a.depth = d_depth; a.cost = d_cost; a.flags = d_flags; a.warp_out = d_warp; a.planes_out = d_planes;
    a.summary = d_summary;
    return run_depth_maps(c, a, agg_radius);
}

int pgx_depth_maps(pgx_ctx *c, const float *gray, int n_frames, int W, int H, const double *P, const int32_t *views, int R, int S,
                   const double *range, int D, int agg_radius, int min_views, int max_cost, int32_t *kq8, double *depth, int32_t *cost,
                   int32_t *flags, double *warp, double *planes, int32_t *summary)
{
    if (!c || !gray || !P || !summary || R < 0 || (R > 0 && (!views || !range || !kq8 || !depth || !flags)))
        return c ? fail(c, PGX_E_BADARG, "null pointer or bad size") : PGX_E_BADARG;
    Lock l(c);
    const int rc = depth_args(c, n_frames, W, H, n_frames, false, R, S, D, agg_radius, min_views, max_cost);
    if (rc != PGX_OK) return rc;
    for (int i = 0; i < 8; i++) summary[i] = 0;
    if (R == 0) return PGX_OK;
    const size_t npix = (size_t)W * H, n = (size_t)R * npix;
    HostImage in, out;
    const int i_g = in.add(gray, (size_t)n_frames * npix, 4), i_P = in.add(P, n_frames, 96), i_v = in.add(views, (size_t)R * (1 + S), 4),
              i_r = in.add(range, R, 16);
    const int o_kq = out.add(kq8, n, 4), o_d = out.add(depth, n, 8), o_c = out.add(cost, n, 4, 0, cost != nullptr),
              o_f = out.add(flags, n, 4), o_w = out.add(warp, (size_t)R * S * 12, 8, 0, warp != nullptr),
              o_p = out.add(planes, (size_t)R * D, 8, 0, planes != nullptr), o_s = out.add(summary, 8, 4, 64);
    int rs = stage_images(c, in, out);
    if (rs != PGX_OK) return rs;
    DepArgs a{};
    a.gray = in.dev<float>(i_g); a.F = a.n_frames = n_frames; a.W = W; a.H = H; a.P = in.dev<double>(i_P);
    a.views = in.dev<int32_t>(i_v); a.R = R; a.S = S; a.range = in.dev<double>(i_r); a.D = D;
    a.min_views = min_views; a.max_cost = max_cost;
    a.kq8 = out.dev<int32_t>(o_kq); a.depth = out.dev<double>(o_d); a.cost = out.dev<int32_t>(o_c); a.flags = out.dev<int32_t>(o_f);
    a.warp_out = out.dev<double>(o_w); a.planes_out = out.dev<double>(o_p); a.summary = out.dev<int32_t>(o_s);
    if ((rs = run_depth_maps(c, a, agg_radius)) != PGX_OK) return rs;
    return download_images(c, out);
}

int pgx_depth_fuse_dev(pgx_ctx *c, const double *d_depth, const int32_t *d_views, int R, int S, int W, int H, int n_frames,
                       const double *d_P, double rel_tol, int min_agree, int max_points, double *d_xyz, int32_t *d_src, int32_t *d_agree,
                       int32_t *d_summary)
{
    if (!c || !d_depth || !d_views || !d_P || !d_summary || (max_points > 0 && (!d_xyz || !d_src)))
        return c ? fail(c, PGX_E_BADARG, "null pointer") : PGX_E_BADARG;
    Lock l(c);
    const int rc = fuse_args(c, R, S, W, H, n_frames, rel_tol, min_agree, max_points);
    if (rc != PGX_OK) return rc;
    if (R == 0) return fail(c, PGX_E_BADARG, "R must be positive");
    FuseArgs a{};
    a.depth = d_depth; a.views = d_views; a.R = R; a.S = S; a.W = W; a.H = H; a.n_frames = n_frames; a.P = d_P;
    a.rel_tol = rel_tol; a.min_agree = min_agree; a.max_points = max_points;
    a.xyz = d_xyz; a.src = d_src; a.agree = d_agree; a.summary = d_summary;
    return run_depth_fuse(c, a);
}

int pgx_depth_fuse(pgx_ctx *c, const double *depth, const int32_t *views, int R, int S, int W, int H, int n_frames, const double *P,
                   double rel_tol, int min_agree, int max_points, double *xyz, int32_t *src, int32_t *agree, int32_t *summary)
{
    if (!c || !P || !summary || R < 0 || (R > 0 && (!depth || !views)) || (max_points > 0 && (!xyz || !src)))
        return c ? fail(c, PGX_E_BADARG, "null pointer or bad size") : PGX_E_BADARG;
    Lock l(c);
    const int rc = fuse_args(c, R, S, W, H, n_frames, rel_tol, min_agree, max_points);
    if (rc != PGX_OK) return rc;
    for (int i = 0; i < 4; i++) summary[i] = 0;
    if (R == 0) return PGX_OK;
    const size_t n = (size_t)R * W * H;
    HostImage in, out;
    const int i_d = in.add(depth, n, 8), i_v = in.add(views, (size_t)R * (1 + S), 4), i_P = in.add(P, n_frames, 96);
    // the summary first: its download tells how many points there are to fetch
    const int o_s = out.add(summary, 4, 4, 64), o_a = out.add(agree, n, 4, 0, agree != nullptr),
              o_x = out.add(nullptr, 0, 24, (size_t)max_points + 1), o_r = out.add(nullptr, 0, 8, (size_t)max_points + 1);
    int rs = stage_images(c, in, out);
    if (rs != PGX_OK) return rs;
    FuseArgs a{};
    a.depth = in.dev<double>(i_d); a.views = in.dev<int32_t>(i_v); a.R = R; a.S = S; a.W = W; a.H = H; a.n_frames = n_frames;
    a.P = in.dev<double>(i_P);
    a.rel_tol = rel_tol; a.min_agree = min_agree; a.max_points = max_points;
    a.xyz = out.dev<double>(o_x); a.src = out.dev<int32_t>(o_r); a.agree = out.dev<int32_t>(o_a); a.summary = out.dev<int32_t>(o_s);
    if ((rs = run_depth_fuse(c, a)) != PGX_OK) return rs;
    rs = download_images(c, out);   // summary and agree; waits for the stream
    const size_t np = (size_t)(summary[0] < max_points ? summary[0] : max_points);
    if (const int rf = fetch_rows(c, out, {{o_x, xyz, 24}, {o_r, src, 8}}, np); rf != PGX_OK) return rf;
    return rs;
}

// ---- the plan of the dense stage: sources and depth range per reference ----------------------------------------------

namespace {
// what the device and the host form check alike (R == 0 is the host form's to allow); the squared cosines of the two angles
int dvw_args(pgx_ctx *c, int R, int n_frames, int S, double min_angle_deg, double max_angle_deg, int min_shared, int min_points,
             int q_near_pm, int q_far_pm, double grow, double *cmin2, double *cmax2)
{
    if (S < 1 || S > 8) return fail(c, PGX_E_BADARG, "S = %d, must be in [1, 8]", S);
    if (R < 0 || R > 65535 || n_frames < 1 || n_frames > 65535) return fail(c, PGX_E_BADARG, "R and n_frames must be in [1, 65535]");
    if ((long long)R * n_frames > (1ll << 24)) return fail(c, PGX_E_BADARG, "R * n_frames must be <= 2^24");
    if (!std::isfinite(min_angle_deg) || !std::isfinite(max_angle_deg) || !(0.0 <= min_angle_deg && min_angle_deg < max_angle_deg && max_angle_deg < 90.0))
        return fail(c, PGX_E_BADARG, "the angles must satisfy 0 <= min_angle_deg < max_angle_deg < 90");
    if (min_shared < 0) return fail(c, PGX_E_BADARG, "min_shared must be >= 0");
    if (min_points < 1) return fail(c, PGX_E_BADARG, "min_points must be >= 1");
    if (q_near_pm < 0 || q_far_pm > 1000 || q_near_pm > q_far_pm)
        return fail(c, PGX_E_BADARG, "the quantiles must satisfy 0 <= q_near_pm <= q_far_pm <= 1000");
    if (!std::isfinite(grow) || grow < 1.0) return fail(c, PGX_E_BADARG, "grow must be finite and >= 1");
    const double c0 = std::cos(min_angle_deg * M_PI / 180.0), c1 = std::cos(max_angle_deg * M_PI / 180.0);
    *cmin2 = c0 * c0;
    *cmax2 = c1 * c1;
    return PGX_OK;
}

bool overlap(const void *p, size_t pn, const void *q, size_t qn)
{
    const char *a = static_cast<const char *>(p), *b = static_cast<const char *>(q);
    return p && q && pn && qn && a < b + qn && b < a + pn;
}

// a device form's arrays, each with its bytes: no output may overlap an input
struct Span {
    const void *p;
    size_t n;
};
int no_alias(pgx_ctx *c, const Span *in, size_t n_in, const Span *out, size_t n_out)
{
    for (size_t o = 0; o < n_out; o++)
        for (size_t i = 0; i < n_in; i++)
            if (overlap(out[o].p, out[o].n, in[i].p, in[i].n)) return fail(c, PGX_E_BADARG, "an output must not alias an input");
    return PGX_OK;
}
} // namespace

int pgx_dense_views_dev(pgx_ctx *c, const int32_t *d_offsets, const int32_t *d_nodes, const int32_t *d_track_summary, int max_tracks,
                        int max_nodes, const double *d_xyz, const int32_t *d_track_flags, int n_frames, const double *d_P,
                        const int32_t *d_refs, int R, int S, double min_angle_deg, double max_angle_deg, int min_shared,
                        int min_points, int q_near_pm, int q_far_pm, double grow, int32_t *d_views, double *d_range,
                        int32_t *d_pair_counts, int32_t *d_ref_stats, int32_t *d_report)
{
    if (!c || !d_offsets || !d_nodes || !d_track_summary || !d_xyz || !d_P || !d_views || !d_range || !d_ref_stats || !d_report)
        return c ? fail(c, PGX_E_BADARG, "null pointer") : PGX_E_BADARG;
    Lock l(c);
    double cmin2 = 0.0, cmax2 = 0.0;
    const int rc = dvw_args(c, R, n_frames, S, min_angle_deg, max_angle_deg, min_shared, min_points, q_near_pm, q_far_pm, grow, &cmin2, &cmax2);
    if (rc != PGX_OK) return rc;
    if (R == 0) return fail(c, PGX_E_BADARG, "R and n_frames must be in [1, 65535]");
    if (!d_refs && R != n_frames) return fail(c, PGX_E_BADARG, "without d_refs, R must equal n_frames");
    if (max_tracks < 0 || max_nodes < 0) return fail(c, PGX_E_BADARG, "max_tracks and max_nodes must be >= 0");
    const size_t mt = max_tracks, nf = n_frames;
    const Span in[] = {{d_offsets, (mt + 1) * 4}, {d_nodes, (size_t)max_nodes * 8}, {d_track_summary, 32},
                       {d_xyz, mt * 24}, {d_track_flags, mt * 4}, {d_P, nf * 96}, {d_refs, (size_t)R * 4}},
               out[] = {{d_views, (size_t)R * (1 + S) * 4}, {d_range, (size_t)R * 16},
                        {d_pair_counts, (size_t)R * nf * 8}, {d_ref_stats, (size_t)R * 16}, {d_report, 32}};
    if (const int ra = no_alias(c, in, std::size(in), out, std::size(out)); ra != PGX_OK) return ra;
    DvwArgs a{};
    a.tv.offsets = d_offsets; a.tv.nodes = d_nodes; a.tv.track_summary = d_track_summary;
    a.tv.n_frames = n_frames; a.tv.max_tracks = max_tracks; a.tv.node_cap = max_nodes;
    a.xyz = d_xyz; a.track_flags = d_track_flags; a.P = d_P; a.refs = d_refs;
    a.R = R; a.S = S; a.min_shared = min_shared; a.min_points = min_points; a.q_near_pm = q_near_pm; a.q_far_pm = q_far_pm;
    a.cmin2 = cmin2; a.cmax2 = cmax2; a.grow = grow;
    a.views = d_views; a.range = d_range; a.pair_counts = d_pair_counts; a.ref_stats = d_ref_stats; a.report = d_report;
    return run_dense_views(c, a);
}

int pgx_dense_views(pgx_ctx *c, const int32_t *track_offsets, const int32_t *nodes, int n_tracks, const double *xyz,
                    const int32_t *track_flags, int n_frames, const double *P, const int32_t *refs, int R, int S, double min_angle_deg,
                    double max_angle_deg, int min_shared, int min_points, int q_near_pm, int q_far_pm, double grow, int32_t *views,
                    double *range, int32_t *pair_counts, int32_t *ref_stats, int32_t *report)
{
    if (!c || !track_offsets || !P || !report || n_tracks < 0 || (n_tracks > 0 && !xyz) || (R > 0 && (!views || !range)))
        return c ? fail(c, PGX_E_BADARG, "null pointer or bad size") : PGX_E_BADARG;
    Lock l(c);
    double cmin2 = 0.0, cmax2 = 0.0;
    int rc = dvw_args(c, R, n_frames, S, min_angle_deg, max_angle_deg, min_shared, min_points, q_near_pm, q_far_pm, grow, &cmin2, &cmax2);
    if (rc != PGX_OK) return rc;
    if (track_offsets[0] != 0) return fail(c, PGX_E_BADARG, "track_offsets[0] must be 0");
    for (int t = 0; t < n_tracks; t++)
        if (track_offsets[t + 1] < track_offsets[t]) return fail(c, PGX_E_BADARG, "track_offsets decrease at track %d", t);
    const long long n_nodes = track_offsets[n_tracks];
    if (n_nodes > 0 && !nodes) return fail(c, PGX_E_BADARG, "null pointer (nodes)");
    for (long long o = 0; o < n_nodes; o++)
        if (nodes[2 * o] < 0 || nodes[2 * o] >= n_frames)
            return fail(c, PGX_E_BADARG, "node %lld names frame %d outside [0, n_frames)", o, nodes[2 * o]);
    for (int i = 0; i < 8; i++) report[i] = 0;
    if (R == 0) return PGX_OK;
    if (!refs && R != n_frames) return fail(c, PGX_E_BADARG, "without refs, R must equal n_frames");
    HostImage in, out;
    const int i_off = in.add(track_offsets, n_tracks + 1, 4), i_nd = in.add(nodes, n_nodes, 8, 1), i_xyz = in.add(xyz, n_tracks, 24, 1),
              i_fl = in.add(track_flags, n_tracks, 4, 1, track_flags != nullptr), i_P = in.add(P, n_frames, 96),
              i_refs = in.add(refs, R, 4, 0, refs != nullptr), i_ts = in.add_words({n_tracks, (int32_t)n_nodes}, 64);
    const int o_v = out.add(views, (size_t)R * (1 + S), 4), o_r = out.add(range, R, 16),
              o_pc = out.add(pair_counts, (size_t)R * n_frames, 8, 0, pair_counts != nullptr), o_st = out.add(ref_stats, R, 16),
              o_rep = out.add(report, 8, 4, 64);
    if ((rc = stage_images(c, in, out)) != PGX_OK) return rc;
    DvwArgs a{};
    a.tv.offsets = in.dev<int32_t>(i_off); a.tv.nodes = in.dev<int32_t>(i_nd); a.tv.track_summary = in.dev<int32_t>(i_ts);
    a.tv.n_frames = n_frames; a.tv.max_tracks = n_tracks; a.tv.node_cap = n_nodes;
    a.xyz = in.dev<double>(i_xyz); a.track_flags = in.dev<int32_t>(i_fl); a.P = in.dev<double>(i_P); a.refs = in.dev<int32_t>(i_refs);
    a.R = R; a.S = S; a.min_shared = min_shared; a.min_points = min_points; a.q_near_pm = q_near_pm; a.q_far_pm = q_far_pm;
    a.cmin2 = cmin2; a.cmax2 = cmax2; a.grow = grow;
    a.views = out.dev<int32_t>(o_v); a.range = out.dev<double>(o_r); a.pair_counts = out.dev<int32_t>(o_pc);
    a.ref_stats = out.dev<int32_t>(o_st); a.report = out.dev<int32_t>(o_rep);   // ref_stats is carved, and downloaded when given
    if ((rc = run_dense_views(c, a)) != PGX_OK) return rc;
    return download_images(c, out);
}

// ---- the fused points merged into one cloud with normals and colour --------------------------------------------------

namespace {
// what both forms of pgx_rgba8_batch check
int rgba8_args(pgx_ctx *c, int F, int W, int H)
{
    if (F <= 0) return fail(c, PGX_E_BADARG, "F must be positive");
    if (dims_ok(c, W, H) != PGX_OK) return PGX_E_BADARG;
    if (c->map_set && (W != c->mapW || H != c->mapH))
        return fail(c, PGX_E_DIM_MISMATCH, "image %dx%d vs dewarp map %dx%d (ArgumentException)", W, H, c->mapW, c->mapH);
    return PGX_OK;
}

int run_rgba8_batch(pgx_ctx *c, const void *d_rgba, int F, int W, int H, uint32_t *d_rgba8)
{
    {
        ProfScope ps(c, "dewarp_rgba8");
        pgx_launch_dewarp_rgba8(c->stream, d_rgba, c->src8, c->map_set ? c->d_map.as<int32_t>() : nullptr, F, W, H, d_rgba8, c->d_status);
    }
    HIPCHK(c, hipGetLastError());
    return PGX_OK;
}

// what the device and the host form of the merge check alike
int cloud_args(pgx_ctx *c, int max_in, int R, int S, int W, int H, int n_frames, bool has_rgba8, int F, bool has_ids, double cell,
               double ox, double oy, double oz, int normal_step, double disc_tol, int min_support, int max_points)
{
    if (dims_ok(c, W, H) != PGX_OK) return PGX_E_BADARG;
    if (R < 1 || R > 65535 || n_frames <= 0) return fail(c, PGX_E_BADARG, "R must be in [1, 65535] and n_frames positive");
    if (S < 1 || S > 8) return fail(c, PGX_E_BADARG, "S = %d, must be in [1, 8]", S);
    if ((long long)R * W * H > (1ll << 30)) return fail(c, PGX_E_BADARG, "R * W * H must be <= 2^30");
    if (max_in < 0 || max_in > (1 << 28) || max_points < 0 || max_points > (1 << 28))
        return fail(c, PGX_E_BADARG, "max_in and max_points must be in [0, 2^28]");
    if (has_rgba8) {
        if (F < 1 || F > 65535) return fail(c, PGX_E_BADARG, "F must be in [1, 65535]");
        if (!has_ids && n_frames != F) return fail(c, PGX_E_BADARG, "without d_frame_ids, n_frames must equal F");
        if ((long long)F * W * H > (1ll << 30)) return fail(c, PGX_E_BADARG, "F * W * H must be <= 2^30");
    }
    if (!std::isfinite(cell) || !(cell > 0.0)) return fail(c, PGX_E_BADARG, "cell must be finite and > 0");
    if (!std::isfinite(ox) || !std::isfinite(oy) || !std::isfinite(oz)) return fail(c, PGX_E_BADARG, "the origin must be finite");
    if (normal_step < 1 || normal_step > 8) return fail(c, PGX_E_BADARG, "normal_step = %d, must be in [1, 8]", normal_step);
    if (!std::isfinite(disc_tol) || !(disc_tol >= 0.0)) return fail(c, PGX_E_BADARG, "disc_tol must be finite and >= 0");
    if (min_support < 1) return fail(c, PGX_E_BADARG, "min_support must be >= 1");
    return PGX_OK;
}
} // namespace

int pgx_rgba8_batch_dev(pgx_ctx *c, const uint16_t *d_rgba, int F, int W, int H, uint32_t *d_rgba8)
{
    if (!c || !d_rgba || !d_rgba8) return c ? fail(c, PGX_E_BADARG, "null pointer") : PGX_E_BADARG;
    Lock l(c);
    if (const int rc = rgba8_args(c, F, W, H); rc != PGX_OK) return rc;
    return run_rgba8_batch(c, d_rgba, F, W, H, d_rgba8);
}

int pgx_rgba8_batch(pgx_ctx *c, const void *rgba, int F, int W, int H, uint32_t *rgba8)
{
    if (!c || !rgba || !rgba8) return c ? fail(c, PGX_E_BADARG, "null pointer") : PGX_E_BADARG;
    Lock l(c);
    if (const int rc = rgba8_args(c, F, W, H); rc != PGX_OK) return rc;
    const size_t n = (size_t)F * W * H;
    HostImage in, out;
    const int i_s = in.add(rgba, n, c->src8 ? 4 : 8), o_d = out.add(rgba8, n, 4);
    int rs = stage_images(c, in, out);
    if (rs != PGX_OK) return rs;
    if ((rs = run_rgba8_batch(c, in.dev<void>(i_s), F, W, H, out.dev<uint32_t>(o_d))) != PGX_OK) return rs;
    return download_images(c, out);
}

int pgx_cloud_merge_dev(pgx_ctx *c, const double *d_xyz, const int32_t *d_src, const int32_t *d_count, int max_in,
                        const double *d_depth, const int32_t *d_views, int R, int S, int W, int H, int n_frames, const double *d_P,
                        const uint32_t *d_rgba8, int F, const int32_t *d_frame_ids, double cell, double ox, double oy, double oz,
                        int normal_step, double disc_tol, int min_support, int max_points, double *d_out_xyz, float *d_out_normal,
                        uint32_t *d_out_rgba8, int32_t *d_out_info, int32_t *d_pt_normal, int32_t *d_cell_of, int32_t *d_report)
{
    if (!c || !d_depth || !d_views || !d_P || !d_report || (max_in > 0 && (!d_xyz || !d_src)) ||
        (max_points > 0 && (!d_out_xyz || !d_out_normal || !d_out_rgba8 || !d_out_info)))
        return c ? fail(c, PGX_E_BADARG, "null pointer") : PGX_E_BADARG;
    Lock l(c);
    const int rc = cloud_args(c, max_in, R, S, W, H, n_frames, d_rgba8 != nullptr, F, d_frame_ids != nullptr, cell, ox, oy, oz,
                              normal_step, disc_tol, min_support, max_points);
    if (rc != PGX_OK) return rc;
    const size_t ni = max_in, no = max_points, npix = (size_t)W * H;
    const Span in[] = {{d_xyz, ni * 24}, {d_src, ni * 8}, {d_count, 4}, {d_depth, (size_t)R * npix * 8},
                       {d_views, (size_t)R * (1 + S) * 4}, {d_P, (size_t)n_frames * 96},
                       {d_rgba8, d_rgba8 ? (size_t)F * npix * 4 : 0},
                       {d_frame_ids, d_rgba8 ? (size_t)F * 4 : 0}},
               out[] = {{d_out_xyz, no * 24}, {d_out_normal, no * 12}, {d_out_rgba8, no * 4}, {d_out_info, no * 16},
                        {d_pt_normal, ni * 12}, {d_cell_of, ni * 4}, {d_report, 32}};
    if (const int ra = no_alias(c, in, std::size(in), out, std::size(out)); ra != PGX_OK) return ra;
    CloudArgs a{};
    a.xyz = d_xyz; a.src = d_src; a.count = d_count; a.max_in = max_in; a.depth = d_depth; a.views = d_views;
    a.R = R; a.S = S; a.W = W; a.H = H; a.n_frames = n_frames; a.P = d_P;
    a.rgba8 = d_rgba8; a.F = d_rgba8 ? F : 0; a.frame_ids = d_rgba8 ? d_frame_ids : nullptr;
    a.cell = cell; a.ox = ox; a.oy = oy; a.oz = oz; a.disc_tol = disc_tol;
    a.normal_step = normal_step; a.min_support = min_support; a.max_points = max_points;
    a.out_xyz = d_out_xyz; a.out_normal = d_out_normal; a.out_rgba8 = d_out_rgba8; a.out_info = d_out_info;
    a.pt_normal = d_pt_normal; a.cell_of = d_cell_of; a.report = d_report;
    return run_cloud_merge(c, a);
}

int pgx_cloud_merge(pgx_ctx *c, const double *xyz, const int32_t *src, int n_in, const double *depth, const int32_t *views, int R, int S,
                    int W, int H, int n_frames, const double *P, const uint32_t *rgba8, double cell, double ox, double oy, double oz,
                    int normal_step, double disc_tol, int min_support, int max_points, double *out_xyz, float *out_normal,
                    uint32_t *out_rgba8, int32_t *out_info, int32_t *pt_normal, int32_t *cell_of, int32_t *report)
{
    if (!c || !depth || !views || !P || !report || (n_in > 0 && (!xyz || !src)) ||
        (max_points > 0 && (!out_xyz || !out_normal || !out_rgba8 || !out_info)))
        return c ? fail(c, PGX_E_BADARG, "null pointer") : PGX_E_BADARG;
    Lock l(c);
    int rs = cloud_args(c, n_in, R, S, W, H, n_frames, rgba8 != nullptr, n_frames, false, cell, ox, oy, oz, normal_step, disc_tol,
                        min_support, max_points);
    if (rs != PGX_OK) return rs;
    const size_t ni = n_in, no = max_points, npix = (size_t)W * H;
    HostImage in, out;
    const int i_x = in.add(xyz, ni, 24, 1), i_s = in.add(src, ni, 8, 1), i_d = in.add(depth, (size_t)R * npix, 8),
              i_v = in.add(views, (size_t)R * (1 + S), 4), i_P = in.add(P, n_frames, 96),
              i_c = in.add(rgba8, (size_t)n_frames * npix, 4, 0, rgba8 != nullptr);
    // the report first: its download tells how many cells there are to fetch
    const int o_r = out.add(report, 8, 4, 64), o_pn = out.add(pt_normal, ni * 3, 4, 0, pt_normal != nullptr),
              o_co = out.add(cell_of, ni, 4, 0, cell_of != nullptr), o_x = out.add(nullptr, 0, 24, no + 1),
              o_n = out.add(nullptr, 0, 12, no + 1), o_c = out.add(nullptr, 0, 4, no + 1), o_i = out.add(nullptr, 0, 16, no + 1);
    if ((rs = stage_images(c, in, out)) != PGX_OK) return rs;
    CloudArgs a{};
    a.xyz = in.dev<double>(i_x); a.src = in.dev<int32_t>(i_s); a.count = nullptr; a.max_in = n_in;
    a.depth = in.dev<double>(i_d); a.views = in.dev<int32_t>(i_v); a.R = R; a.S = S; a.W = W; a.H = H; a.n_frames = n_frames;
    a.P = in.dev<double>(i_P); a.rgba8 = in.dev<uint32_t>(i_c); a.F = rgba8 ? n_frames : 0; a.frame_ids = nullptr;
    a.cell = cell; a.ox = ox; a.oy = oy; a.oz = oz; a.disc_tol = disc_tol;
    a.normal_step = normal_step; a.min_support = min_support; a.max_points = max_points;
    a.out_xyz = out.dev<double>(o_x); a.out_normal = out.dev<float>(o_n); a.out_rgba8 = out.dev<uint32_t>(o_c);
    a.out_info = out.dev<int32_t>(o_i); a.pt_normal = out.dev<int32_t>(o_pn); a.cell_of = out.dev<int32_t>(o_co);
    a.report = out.dev<int32_t>(o_r);
    if ((rs = run_cloud_merge(c, a)) != PGX_OK) return rs;
    rs = download_images(c, out);   // the report and the per-point outputs; waits for the stream
    if (rs != PGX_OK && rs != PGX_E_CAPACITY) return rs;   // the report was not downloaded: nothing tells how many rows there are
    const size_t np = (size_t)(report[6] < max_points ? report[6] : max_points);
    if (const int rf = fetch_rows(c, out, {{o_x, out_xyz, 24}, {o_n, out_normal, 12}, {o_c, out_rgba8, 4}, {o_i, out_info, 16}}, np); rf != PGX_OK)
        return rf;
    return rs;
}

// ---- a triangle mesh from the depth maps: TSDF grid and surface nets ----------------------------------------------------

namespace {
// what the device and the host form of the mesh check alike: the cloud's refusals for the arguments the calls share, then its own
int mesh_args(pgx_ctx *c, int max_in, int R, int S, int W, int H, int n_frames, int min_agree, bool has_rgba8, int F, bool has_ids,
              double cell, double ox, double oy, double oz, int band, int trunc_cells, int min_weight, int max_voxels, int max_vertices,
              int max_tris)
{
    if (const int rc = cloud_args(c, max_in, R, S, W, H, n_frames, has_rgba8, F, has_ids, cell, ox, oy, oz, 1, 0.0, 1, 0); rc != PGX_OK)
        return rc;
    if (band < 1 || band > 3) return fail(c, PGX_E_BADARG, "band = %d, must be in [1, 3]", band);
    if (trunc_cells < 1 || trunc_cells > 8) return fail(c, PGX_E_BADARG, "trunc_cells = %d, must be in [1, 8]", trunc_cells);
    if (min_weight < 1) return fail(c, PGX_E_BADARG, "min_weight must be >= 1");
    if (min_agree < 0) return fail(c, PGX_E_BADARG, "min_agree must be >= 0");
    for (const int cap : {max_voxels, max_vertices, max_tris})
        if (cap < 0 || cap > (1 << 28)) return fail(c, PGX_E_BADARG, "max_voxels, max_vertices and max_tris must be in [0, 2^28]");
    return PGX_OK;
}
} // namespace

int pgx_mesh_dev(pgx_ctx *c, const double *d_xyz, const int32_t *d_src, const int32_t *d_count, int max_in, const double *d_depth,
                 const int32_t *d_views, int R, int S, int W, int H, int n_frames, const double *d_P, const int32_t *d_agree,
                 int min_agree, const uint32_t *d_rgba8, int F, const int32_t *d_frame_ids, double cell, double ox, double oy, double oz,
                 int band, int trunc_cells, int min_weight, int max_voxels, int max_vertices, int max_tris, double *d_out_xyz,
                 float *d_out_normal, uint32_t *d_out_rgba8, int32_t *d_out_info, int32_t *d_out_tri, int32_t *d_report)
{
    if (!c || !d_depth || !d_views || !d_P || !d_report || (max_in > 0 && (!d_xyz || !d_src)) ||
        (max_vertices > 0 && (!d_out_xyz || !d_out_normal || !d_out_rgba8 || !d_out_info)) || (max_tris > 0 && !d_out_tri))
        return c ? fail(c, PGX_E_BADARG, "null pointer") : PGX_E_BADARG;
    Lock l(c);
    const int rc = mesh_args(c, max_in, R, S, W, H, n_frames, min_agree, d_rgba8 != nullptr, F, d_frame_ids != nullptr, cell, ox, oy, oz,
                             band, trunc_cells, min_weight, max_voxels, max_vertices, max_tris);
    if (rc != PGX_OK) return rc;
    const size_t ni = max_in, nv = max_vertices, nt = max_tris, npix = (size_t)W * H;
    const Span in[] = {{d_xyz, ni * 24}, {d_src, ni * 8}, {d_count, 4}, {d_depth, (size_t)R * npix * 8},
                       {d_views, (size_t)R * (1 + S) * 4}, {d_P, (size_t)n_frames * 96},
                       {d_agree, (size_t)R * npix * 4}, {d_rgba8, d_rgba8 ? (size_t)F * npix * 4 : 0},
                       {d_frame_ids, d_rgba8 ? (size_t)F * 4 : 0}},
               out[] = {{d_out_xyz, nv * 24}, {d_out_normal, nv * 12}, {d_out_rgba8, nv * 4}, {d_out_info, nv * 16},
                        {d_out_tri, nt * 12}, {d_report, 32}};
    if (const int ra = no_alias(c, in, std::size(in), out, std::size(out)); ra != PGX_OK) return ra;
    MeshArgs a{};
    a.xyz = d_xyz; a.src = d_src; a.count = d_count; a.max_in = max_in; a.depth = d_depth; a.views = d_views;
    a.R = R; a.S = S; a.W = W; a.H = H; a.n_frames = n_frames; a.P = d_P; a.agree = d_agree; a.min_agree = min_agree;
    a.rgba8 = d_rgba8; a.F = d_rgba8 ? F : 0; a.frame_ids = d_rgba8 ? d_frame_ids : nullptr;
    a.cell = cell; a.ox = ox; a.oy = oy; a.oz = oz; a.band = band; a.trunc_cells = trunc_cells; a.min_weight = min_weight;
    a.max_voxels = max_voxels; a.max_vertices = max_vertices; a.max_tris = max_tris;
    a.out_xyz = d_out_xyz; a.out_normal = d_out_normal; a.out_rgba8 = d_out_rgba8; a.out_info = d_out_info; a.out_tri = d_out_tri;
    a.report = d_report;
    return run_mesh(c, a);
}

int pgx_mesh(pgx_ctx *c, const double *xyz, const int32_t *src, int n_in, const double *depth, const int32_t *views, int R, int S, int W,
             int H, int n_frames, const double *P, const int32_t *agree, int min_agree, const uint32_t *rgba8, double cell, double ox,
             double oy, double oz, int band, int trunc_cells, int min_weight, int max_voxels, int max_vertices, int max_tris,
             double *out_xyz, float *out_normal, uint32_t *out_rgba8, int32_t *out_info, int32_t *out_tri, int32_t *report)
{
    if (!c || !depth || !views || !P || !report || (n_in > 0 && (!xyz || !src)) ||
        (max_vertices > 0 && (!out_xyz || !out_normal || !out_rgba8 || !out_info)) || (max_tris > 0 && !out_tri))
        return c ? fail(c, PGX_E_BADARG, "null pointer") : PGX_E_BADARG;
    Lock l(c);
    int rs = mesh_args(c, n_in, R, S, W, H, n_frames, min_agree, rgba8 != nullptr, n_frames, false, cell, ox, oy, oz, band, trunc_cells,
                       min_weight, max_voxels, max_vertices, max_tris);
    if (rs != PGX_OK) return rs;
    const size_t ni = n_in, nv = max_vertices, nt = max_tris, npix = (size_t)W * H;
    HostImage in, out;
    const int i_x = in.add(xyz, ni, 24, 1), i_s = in.add(src, ni, 8, 1), i_d = in.add(depth, (size_t)R * npix, 8),
              i_v = in.add(views, (size_t)R * (1 + S), 4), i_P = in.add(P, n_frames, 96),
              i_a = in.add(agree, (size_t)R * npix, 4, 0, agree != nullptr),
              i_c = in.add(rgba8, (size_t)n_frames * npix, 4, 0, rgba8 != nullptr);
    // the report first: its download tells how many vertices and triangles there are to fetch
    const int o_r = out.add(report, 8, 4, 64);
    const MeshOut o = mesh_out(out, nv, nt);
    if ((rs = stage_images(c, in, out)) != PGX_OK) return rs;
    MeshArgs a{};
    a.xyz = in.dev<double>(i_x); a.src = in.dev<int32_t>(i_s); a.count = nullptr; a.max_in = n_in;
    a.depth = in.dev<double>(i_d); a.views = in.dev<int32_t>(i_v); a.R = R; a.S = S; a.W = W; a.H = H; a.n_frames = n_frames;
    a.P = in.dev<double>(i_P); a.agree = in.dev<int32_t>(i_a); a.min_agree = min_agree;
    a.rgba8 = in.dev<uint32_t>(i_c); a.F = rgba8 ? n_frames : 0; a.frame_ids = nullptr;
    a.cell = cell; a.ox = ox; a.oy = oy; a.oz = oz; a.band = band; a.trunc_cells = trunc_cells; a.min_weight = min_weight;
    a.max_voxels = max_voxels; a.max_vertices = max_vertices; a.max_tris = max_tris;
    const MeshRows r = mesh_dev(out, o);
    a.out_xyz = r.xyz; a.out_normal = r.normal; a.out_rgba8 = r.rgba8; a.out_info = r.info; a.out_tri = r.tri; a.report = out.dev<int32_t>(o_r);
    if ((rs = run_mesh(c, a)) != PGX_OK) return rs;
    rs = download_images(c, out);   // the report; waits for the stream
    if (rs != PGX_OK && rs != PGX_E_CAPACITY) return rs;   // the report was not downloaded: nothing tells how many rows there are
    const int rf = fetch_mesh(c, out, o, {out_xyz, out_normal, out_rgba8, out_info, out_tri}, report, max_vertices, max_tris);
    return rf != PGX_OK ? rf : rs;
}

// ---- what the stages that take a mesh list and write one share (the clean stage, the decimation) ------------------------------

namespace {
// the refusals of both stages, device and host form
int mesh_list_args(pgx_ctx *c, int max_vertices, int max_tris, double cell, double ox, double oy, double oz, int max_out_vertices,
                   int max_out_tris)
{
    for (const int cap : {max_vertices, max_tris, max_out_vertices, max_out_tris})
        if (cap < 0 || cap > (1 << 28))
            return fail(c, PGX_E_BADARG, "max_vertices, max_tris, max_out_vertices and max_out_tris must be in [0, 2^28]");
    if (!std::isfinite(cell) || !(cell > 0.0)) return fail(c, PGX_E_BADARG, "cell must be finite and > 0");
    if (!std::isfinite(ox) || !std::isfinite(oy) || !std::isfinite(oz)) return fail(c, PGX_E_BADARG, "the origin must be finite");
    return PGX_OK;
}

// a device form's lists, read from the filled arguments: aux is the stage's own per-vertex output (comp, level)
extern "C++" template <class A> int mesh_list_no_alias(pgx_ctx *c, const A &a, const int32_t *aux)
{
    const size_t nv = a.max_vertices, nt = a.max_tris, mv = a.max_out_vertices, mt = a.max_out_tris;
    const Span in[] = {{a.xyz, nv * 24}, {a.normal, nv * 12}, {a.rgba8, nv * 4}, {a.info, nv * 16}, {a.tri, nt * 12}, {a.counts, 32}},
               out[] = {{a.out_xyz, mv * 24}, {a.out_normal, mv * 12}, {a.out_rgba8, mv * 4}, {a.out_info, mv * 16},
                        {a.out_tri, mt * 12}, {a.vertex_map, nv * 4}, {aux, nv * 4}, {a.report, 32}};
    return no_alias(c, in, std::size(in), out, std::size(out));
}

// the pointers that MeshCleanArgs and MeshDecimateArgs name alike; the scalars are assigned by name where the form stands
extern "C++" template <class A>
void mesh_list_fill(A &a, const MeshList &i, const int32_t *counts, const MeshRows &o, int32_t *vertex_map, int32_t *report)
{
    a.xyz = i.xyz; a.normal = i.normal; a.rgba8 = i.rgba8; a.info = i.info; a.tri = i.tri; a.counts = counts;
    a.out_xyz = o.xyz; a.out_normal = o.normal; a.out_rgba8 = o.rgba8; a.out_info = o.info; a.out_tri = o.tri;
    a.vertex_map = vertex_map; a.report = report;
}
} // namespace

// ---- the mesh cleaned: small components dropped, smoothed, normals again ----------------------------------------------------

namespace {
// what the device and the host form of the clean stage check alike
int mesh_clean_args(pgx_ctx *c, int max_vertices, int max_tris, double cell, double ox, double oy, double oz, int min_tris, int min_frac_pm,
                    int iters, double lambda, double mu, int max_out_vertices, int max_out_tris)
{
    if (const int rc = mesh_list_args(c, max_vertices, max_tris, cell, ox, oy, oz, max_out_vertices, max_out_tris); rc != PGX_OK) return rc;
    if (min_tris < 1) return fail(c, PGX_E_BADARG, "min_tris must be >= 1");
    if (min_frac_pm < 0 || min_frac_pm > 1000) return fail(c, PGX_E_BADARG, "min_frac_pm = %d, must be in [0, 1000]", min_frac_pm);
    if (iters < 0 || iters > 64) return fail(c, PGX_E_BADARG, "iters = %d, must be in [0, 64]", iters);
    if (!std::isfinite(lambda) || !(lambda > 0.0) || lambda > 1.0) return fail(c, PGX_E_BADARG, "lambda must be in (0, 1]");
    if (!std::isfinite(mu) || mu < -1.5 || mu > 0.0) return fail(c, PGX_E_BADARG, "mu must be in [-1.5, 0]");
    return PGX_OK;
}
} // namespace

int pgx_mesh_clean_dev(pgx_ctx *c, const double *d_xyz, const float *d_normal, const uint32_t *d_rgba8, const int32_t *d_info,
                       const int32_t *d_tri, const int32_t *d_counts, int max_vertices, int max_tris, double cell, double ox, double oy,
                       double oz, int min_tris, int min_frac_pm, int iters, double lambda, double mu, int max_out_vertices,
                       int max_out_tris, double *d_out_xyz, float *d_out_normal, uint32_t *d_out_rgba8, int32_t *d_out_info,
                       int32_t *d_out_tri, int32_t *d_vertex_map, int32_t *d_comp, int32_t *d_report)
{
    if (!c || !d_report || (max_vertices > 0 && (!d_xyz || !d_normal || !d_rgba8 || !d_info)) || (max_tris > 0 && !d_tri) ||
        (max_out_vertices > 0 && (!d_out_xyz || !d_out_normal || !d_out_rgba8 || !d_out_info)) || (max_out_tris > 0 && !d_out_tri))
        return c ? fail(c, PGX_E_BADARG, "null pointer") : PGX_E_BADARG;
    Lock l(c);
    const int rc = mesh_clean_args(c, max_vertices, max_tris, cell, ox, oy, oz, min_tris, min_frac_pm, iters, lambda, mu, max_out_vertices,
                                   max_out_tris);
    if (rc != PGX_OK) return rc;
    MeshCleanArgs a{};
    mesh_list_fill(a, {d_xyz, d_normal, d_rgba8, d_info, d_tri}, d_counts, {d_out_xyz, d_out_normal, d_out_rgba8, d_out_info, d_out_tri}, d_vertex_map,
                   d_report);
    a.max_vertices = max_vertices; a.max_tris = max_tris; a.cell = cell; a.ox = ox; a.oy = oy; a.oz = oz;
    a.max_out_vertices = max_out_vertices; a.max_out_tris = max_out_tris;
    a.min_tris = min_tris; a.min_frac_pm = min_frac_pm; a.iters = iters; a.lambda = lambda; a.mu = mu; a.comp = d_comp;
    if (const int ra = mesh_list_no_alias(c, a, a.comp); ra != PGX_OK) return ra;
    return run_mesh_clean(c, a);
}

int pgx_mesh_clean(pgx_ctx *c, const double *xyz, const float *normal, const uint32_t *rgba8, const int32_t *info, const int32_t *tri,
                   int n_vertices, int n_tris, double cell, double ox, double oy, double oz, int min_tris, int min_frac_pm, int iters,
                   double lambda, double mu, int max_out_vertices, int max_out_tris, double *out_xyz, float *out_normal,
                   uint32_t *out_rgba8, int32_t *out_info, int32_t *out_tri, int32_t *vertex_map, int32_t *comp, int32_t *report)
{
    if (!c || !report || (n_vertices > 0 && (!xyz || !normal || !rgba8 || !info)) || (n_tris > 0 && !tri) ||
        (max_out_vertices > 0 && (!out_xyz || !out_normal || !out_rgba8 || !out_info)) || (max_out_tris > 0 && !out_tri))
        return c ? fail(c, PGX_E_BADARG, "null pointer") : PGX_E_BADARG;
    Lock l(c);
    int rs = mesh_clean_args(c, n_vertices, n_tris, cell, ox, oy, oz, min_tris, min_frac_pm, iters, lambda, mu, max_out_vertices,
                             max_out_tris);
    if (rs != PGX_OK) return rs;
    const size_t nv = n_vertices;
    HostImage in, out;
    const MeshIn i = mesh_in(in, xyz, normal, rgba8, info, tri, nv, n_tris);
    // the report first: its download tells how many vertices and triangles there are to fetch
    const int o_r = out.add(report, 8, 4, 64), o_vm = out.add(vertex_map, nv, 4, 1, vertex_map != nullptr),
              o_cp = out.add(comp, nv, 4, 1, comp != nullptr);
    const MeshOut o = mesh_out(out, max_out_vertices, max_out_tris);
    if ((rs = stage_images(c, in, out)) != PGX_OK) return rs;
    MeshCleanArgs a{};
    mesh_list_fill(a, mesh_dev(in, i), nullptr, mesh_dev(out, o), out.dev<int32_t>(o_vm), out.dev<int32_t>(o_r));
    a.max_vertices = n_vertices; a.max_tris = n_tris; a.cell = cell; a.ox = ox; a.oy = oy; a.oz = oz;
    a.max_out_vertices = max_out_vertices; a.max_out_tris = max_out_tris;
    a.min_tris = min_tris; a.min_frac_pm = min_frac_pm; a.iters = iters; a.lambda = lambda; a.mu = mu; a.comp = out.dev<int32_t>(o_cp);
    if ((rs = run_mesh_clean(c, a)) != PGX_OK) return rs;
    rs = download_images(c, out);   // the report and the per-vertex maps; waits for the stream
    if (rs != PGX_OK && rs != PGX_E_CAPACITY) return rs;   // the report was not downloaded: nothing tells how many rows there are
    const int rf = fetch_mesh(c, out, o, {out_xyz, out_normal, out_rgba8, out_info, out_tri}, report, max_out_vertices, max_out_tris);
    return rf != PGX_OK ? rf : rs;
}

// ---- the mesh decimated: adaptive vertex clustering over grid blocks ----------------------------------------------------------

namespace {
// what the device and the host form of the decimation check alike
int mesh_decimate_args(pgx_ctx *c, int max_vertices, int max_tris, double cell, double ox, double oy, double oz, int lmin, int lmax,
                       int flat_q, int max_out_vertices, int max_out_tris)
{
    if (const int rc = mesh_list_args(c, max_vertices, max_tris, cell, ox, oy, oz, max_out_vertices, max_out_tris); rc != PGX_OK) return rc;
    if (lmin < 0 || lmin > 6) return fail(c, PGX_E_BADARG, "lmin = %d, must be in [0, 6]", lmin);
    if (lmax < lmin || lmax > 6) return fail(c, PGX_E_BADARG, "lmax = %d, must be in [lmin, 6]", lmax);
    if (flat_q < 0 || flat_q > 1024) return fail(c, PGX_E_BADARG, "flat_q = %d, must be in [0, 1024]", flat_q);
    return PGX_OK;
}
} // namespace

int pgx_mesh_decimate_dev(pgx_ctx *c, const double *d_xyz, const float *d_normal, const uint32_t *d_rgba8, const int32_t *d_info,
                          const int32_t *d_tri, const int32_t *d_counts, int max_vertices, int max_tris, double cell, double ox, double oy,
                          double oz, int lmin, int lmax, int flat_q, int max_out_vertices, int max_out_tris, double *d_out_xyz,
                          float *d_out_normal, uint32_t *d_out_rgba8, int32_t *d_out_info, int32_t *d_out_tri, int32_t *d_vertex_map,
                          int32_t *d_level, int32_t *d_report)
{
    if (!c || !d_report || (max_vertices > 0 && (!d_xyz || !d_normal || !d_rgba8 || !d_info)) || (max_tris > 0 && !d_tri) ||
        (max_out_vertices > 0 && (!d_out_xyz || !d_out_normal || !d_out_rgba8 || !d_out_info)) || (max_out_tris > 0 && !d_out_tri))
        return c ? fail(c, PGX_E_BADARG, "null pointer") : PGX_E_BADARG;
    Lock l(c);
    const int rc = mesh_decimate_args(c, max_vertices, max_tris, cell, ox, oy, oz, lmin, lmax, flat_q, max_out_vertices, max_out_tris);
    if (rc != PGX_OK) return rc;
    MeshDecimateArgs a{};
    mesh_list_fill(a, {d_xyz, d_normal, d_rgba8, d_info, d_tri}, d_counts, {d_out_xyz, d_out_normal, d_out_rgba8, d_out_info, d_out_tri}, d_vertex_map,
                   d_report);
    a.max_vertices = max_vertices; a.max_tris = max_tris; a.cell = cell; a.ox = ox; a.oy = oy; a.oz = oz;
    a.max_out_vertices = max_out_vertices; a.max_out_tris = max_out_tris;
    a.lmin = lmin; a.lmax = lmax; a.flat_q = flat_q; a.level = d_level;
    if (const int ra = mesh_list_no_alias(c, a, a.level); ra != PGX_OK) return ra;
    return run_mesh_decimate(c, a);
}

int pgx_mesh_decimate(pgx_ctx *c, const double *xyz, const float *normal, const uint32_t *rgba8, const int32_t *info, const int32_t *tri,
                      int n_vertices, int n_tris, double cell, double ox, double oy, double oz, int lmin, int lmax, int flat_q,
                      int max_out_vertices, int max_out_tris, double *out_xyz, float *out_normal, uint32_t *out_rgba8, int32_t *out_info,
                      int32_t *out_tri, int32_t *vertex_map, int32_t *level, int32_t *report)
{
    if (!c || !report || (n_vertices > 0 && (!xyz || !normal || !rgba8 || !info)) || (n_tris > 0 && !tri) ||
        (max_out_vertices > 0 && (!out_xyz || !out_normal || !out_rgba8 || !out_info)) || (max_out_tris > 0 && !out_tri))
        return c ? fail(c, PGX_E_BADARG, "null pointer") : PGX_E_BADARG;
    Lock l(c);
    int rs = mesh_decimate_args(c, n_vertices, n_tris, cell, ox, oy, oz, lmin, lmax, flat_q, max_out_vertices, max_out_tris);
    if (rs != PGX_OK) return rs;
    const size_t nv = n_vertices;
    HostImage in, out;
    const MeshIn i = mesh_in(in, xyz, normal, rgba8, info, tri, nv, n_tris);
    // the report first: its download tells how many vertices and triangles there are to fetch
    const int o_r = out.add(report, 8, 4, 64), o_vm = out.add(vertex_map, nv, 4, 1, vertex_map != nullptr),
              o_lv = out.add(level, nv, 4, 1, level != nullptr);
    const MeshOut o = mesh_out(out, max_out_vertices, max_out_tris);
    if ((rs = stage_images(c, in, out)) != PGX_OK) return rs;
    MeshDecimateArgs a{};
    mesh_list_fill(a, mesh_dev(in, i), nullptr, mesh_dev(out, o), out.dev<int32_t>(o_vm), out.dev<int32_t>(o_r));
    a.max_vertices = n_vertices; a.max_tris = n_tris; a.cell = cell; a.ox = ox; a.oy = oy; a.oz = oz;
    a.max_out_vertices = max_out_vertices; a.max_out_tris = max_out_tris;
    a.lmin = lmin; a.lmax = lmax; a.flat_q = flat_q; a.level = out.dev<int32_t>(o_lv);
    if ((rs = run_mesh_decimate(c, a)) != PGX_OK) return rs;
    rs = download_images(c, out);   // the report and the per-vertex maps; waits for the stream
    if (rs != PGX_OK && rs != PGX_E_CAPACITY) return rs;   // the report was not downloaded: nothing tells how many rows there are
    const int rf = fetch_mesh(c, out, o, {out_xyz, out_normal, out_rgba8, out_info, out_tri}, report, max_out_vertices, max_out_tris);
    return rf != PGX_OK ? rf : rs;
}

// ---- measurement hooks ---------------------------------------------------------------------

int pgx_profile_enable(pgx_ctx *c, int on)
{
    if (!c) return PGX_E_BADARG;
    Lock l(c);
    c->prof_on = on != 0;
    return PGX_OK;
}

int pgx_profile_filter(pgx_ctx *c, const char *name)
{
    if (!c) return PGX_E_BADARG;
    Lock l(c);
    c->prof_only = name ? name : "";
    return PGX_OK;
}

static void prof_drain(pgx_ctx *c)
{
    for (auto &kv : c->prof) {
        for (auto &ev : kv.second.pending) {
            float ms = 0.f;
            if (hipEventElapsedTime(&ms, ev.first, ev.second) == hipSuccess) {
                kv.second.total_ms += ms;
                kv.second.launches += 1;
            }
            c->ev_pool.push_back(ev.first);
            c->ev_pool.push_back(ev.second);
        }
        kv.second.pending.clear();
    }
}

int pgx_profile_get(pgx_ctx *c, const char *name, int *launches, double *total_ms)
{
    if (!c || !name) return PGX_E_BADARG;
    Lock l(c);
    HIPCHK(c, hipStreamSynchronize(c->stream));
    prof_drain(c);
    auto it = c->prof.find(name);
    if (launches) *launches = it == c->prof.end() ? 0 : it->second.launches;
    if (total_ms) *total_ms = it == c->prof.end() ? 0.0 : it->second.total_ms;
    return PGX_OK;
}

int pgx_profile_serialize(pgx_ctx *c, int on)
{
    if (!c) return PGX_E_BADARG;
    Lock l(c);
    c->prof_serial = on != 0;
    return PGX_OK;
}

int pgx_profile_reset(pgx_ctx *c)
{
    if (!c) return PGX_E_BADARG;
    Lock l(c);
    HIPCHK(c, hipStreamSynchronize(c->stream));
    prof_drain(c);
    c->prof.clear();
    return PGX_OK;
}

int pgx_debug_counters(pgx_ctx *c, int64_t *out8)
{
    if (!c || !out8) return PGX_E_BADARG;
    Lock l(c);
    HIPCHK(c, hipStreamSynchronize(c->stream));
    HIPCHK(c, hipMemcpy(out8, c->d_status + PGX_DBG_OFF, 64, hipMemcpyDeviceToHost));
    HIPCHK(c, hipMemset(c->d_status + PGX_DBG_OFF, 0, 64));
    return PGX_OK;
}

int pgx_match_stats(pgx_ctx *c, int *rounds_wide, int64_t *evaluations, int64_t *evaluations_round0)
{
    if (!c) return PGX_E_BADARG;
    Lock l(c);
    unsigned long long ev[PGX_MAX_WIDE_ROUNDS] = {0};
    HIPCHK(c, hipStreamSynchronize(c->stream));
    HIPCHK(c, hipMemcpy(ev, c->d_status + 4, sizeof ev, hipMemcpyDeviceToHost));
    long long tot = 0;
    for (int r = 0; r < c->last_rounds_mfma && r < PGX_MAX_WIDE_ROUNDS; r++) tot += (long long)ev[r];
    if (rounds_wide) *rounds_wide = c->last_rounds_mfma;
    if (evaluations) *evaluations = tot;
    if (evaluations_round0) *evaluations_round0 = c->last_rounds_mfma > 0 ? (long long)ev[0] : 0;
    return PGX_OK;
}

} // extern "C"
