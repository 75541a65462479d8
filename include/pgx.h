/*
 * pgx.h -- C ABI of libpgx.so: MI355X (gfx950) native dewarp -> FAST-like detect -> NMS ->
 * BRIEF -> all-pairs Hamming match with the reference's greedy one-to-one assignment.
 *
 * This is the drop-in boundary for the hot path of Takatsuka-Mark/Photogrammetry
 * (dotnet_src/ImageProcessing).  The reference has no FFI today; every entry
 * point below names the C# member it replaces, and INTEGRATION.md shows the [DllImport]
 * stubs a maintainer would add.  Plain pointers and sizes only; no C++ or torch types.
 *
 * Conventions
 *   - Images are row-major [H][W]; pixel (x, y) = column x, row y = the reference's
 *     Matrix<T>[x, y] (Math/LinearAlgebra/Matrix.cs:44-76).
 *   - Rgba64 pixel = 4 x uint16 {R,G,B,A} (Images.Abstractions/Pixels/Rgba64.cs:3-9).
 *   - A descriptor is ceil(P/32) little-endian uint32 words of the reference's BigInteger:
 *     bit b of the BigInteger is bit (b & 31) of word (b >> 5); BRIEF test pair p lands on
 *     bit P-1-p (ImageProcessing.Abstractions/Keypoint.cs:29-57).
 *   - Every function returns PGX_OK or a PGX_E_* code; pgx_last_error() gives the text.
 *     No C++ exception crosses this boundary.
 *   - "host" entry points take host pointers, copy in/out and return when the result is in
 *     the caller's buffer.  "_dev" entry points take DEVICE pointers, enqueue on the
 *     context's stream and return immediately; data errors surface in pgx_check_status().
 *   - The caller owns every buffer; the library keeps no caller pointer after a call returns.
 *   - One context per GPU.  Calls on one context are serialised by an internal mutex
 *     (the reference never re-enters a stage: TestService.cs:25,137-152), so a context may be called from several host
 *     threads -- the reference's pipeline runs ApplyDistortionMat on image k + 1 beside Detect on image k
 *     (TestService.cs:25,146-149) -- but its stages then run one after the other; one context per stage (each with its own
 *     configuration and workspaces) lets them overlap on the device.  tests/test_gpu_threads.py covers both.
 *   - pgx_last_error(ctx) is per calling thread: it returns the text of that thread's most recent failing call on ctx
 *     (valid until the thread's next failing call or next pgx_last_error); a thread that has not failed on ctx gets a copy
 *     of the most recent failure of any thread.
 */
#ifndef PGX_H
#define PGX_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PGX_OK               0
#define PGX_E_DIM_MISMATCH   1  /* ArgumentException            DeWarp.cs:22-23           */
#define PGX_E_OOB_SOURCE     2  /* IndexOutOfRangeException     Matrix.cs:63-66,204-209   */
#define PGX_E_EMPTY_SET      3  /* ArgumentOutOfRangeException  KeypointMatching.cs:61    */
#define PGX_E_CAPACITY       4  /* an output or workspace capacity was exceeded           */
#define PGX_E_BADARG         5  /* ArgumentException / null pointer / unsupported size    */
#define PGX_E_HIP            6  /* a HIP runtime call failed                              */
#define PGX_E_NOT_CONFIGURED 7  /* stage used before its pgx_set_* call                   */
#define PGX_E_RCCL           8  /* an RCCL call failed, or librccl could not be loaded    */

#define PGX_DIST_NONE 2147483647 /* int.MaxValue: tail entries when N1 > N2 (KeypointMatching.cs:40-42) */

typedef struct pgx_ctx pgx_ctx;

/* Keypoint{Coordinate, FastScore, Value} (ImageProcessing.Abstractions/Keypoint.cs:11-15);
 * the BriefDescriptor travels in a separate [N][words] array. */
typedef struct { int32_t x, y, fast_score; float value; } pgx_keypoint;

/* KeypointPair{Keypoint1, Keypoint2, Distance} as indices into the two input lists
 * (ImageProcessing.Abstractions/KeypointPair.cs:3-8). */
typedef struct { int32_t k1, k2, dist; } pgx_pair;

/* ---- context ------------------------------------------------------------------------ */
int  pgx_ctx_create(int device, pgx_ctx **out);
void pgx_ctx_destroy(pgx_ctx *ctx);
const char *pgx_last_error(pgx_ctx *ctx);
const char *pgx_version(void);
/* Use the caller's HIP stream (hipStream_t) for all work; NULL = the context's own stream. */
int  pgx_set_stream(pgx_ctx *ctx, void *hip_stream);
/* Wait for the stream and report the first data error of the "_dev" calls since the last check. */
int  pgx_check_status(pgx_ctx *ctx);

/* ---- init-time configuration (replaces DI-bound options, Program.cs:61-69) ----------- */
/* Pixel type of every `rgba` argument below (host and device): PGX_SRC_RGBA64 (default) = 4 x uint16 as
 * Rgba64 (Rgba64.cs:3-9); PGX_SRC_RGBA8 = 4 x uint8, widened on the device to c * 257 per channel, which is what an
 * 8-bit file becomes when LocalImageReader loads it as Rgba64 (LocalImageReader.cs:22; SURVEY 8f-4 "ingest"): half the
 * upload and half the gathered bytes, identical results.  pgx_dewarp's output stays Rgba64. */
enum { PGX_SRC_RGBA64 = 0, PGX_SRC_RGBA8 = 1 };
int pgx_set_source_format(pgx_ctx *ctx, int format);
/* DeWarpTransformStepFactory.Initialize (DeWarpTransformStepFactory.cs:26-31): the Matrix<Uv>
 * built by DeWarp.GetDistortionMatrix, as host int32 [H][W][2] = (U, V).  NULL = stage off.
 * Memory: the context keeps the table on the device (8 B per pixel) and, made from it once when it is installed (here or by
 * pgx_set_dewarp_coeffs), its gather plan: one 32-bit source offset per pixel, 4 B per pixel more -- 12 B per pixel in all, 25 MB
 * at 1920 x 1080.  The batched detect calls gather through the plan; it is rebuilt with every table and released with it. */
int pgx_set_dewarp_map(pgx_ctx *ctx, const int32_t *uv, int W, int H);
/* The same table built ON THE DEVICE from DeWarpOptions.DistortionCoefficients (DeWarp.GetDistortionMatrix,
 * DeWarp.cs:39-107; exactly 5 coefficients or PGX_E_BADARG like DeWarp.cs:46-48): no 8-66 MB upload, no host
 * loop.  Same float64 formulas as pgx_build_dewarp_map; the device's libm differs from the host's in the last
 * ulp, so isolated entries can differ by +-1 from the host-built table ("within +-1 px, unpinned"). */
int pgx_set_dewarp_coeffs(pgx_ctx *ctx, int W, int H, const double *coeffs, int ncoeffs);
/* Copy the context's current table back to the host, int32 [H][W][2] (inspection / caching by the host). */
int pgx_get_dewarp_map(pgx_ctx *ctx, int32_t *uv_out, int W, int H);
/* KeypointDetection ctor's _gaussianKeypairs (KeypointDetection.cs:35-39): host int32 [P][4] =
 * (x1, y1, x2, y2).  The table is an INPUT because the reference draws it unseeded. */
int pgx_set_brief_pairs(pgx_ctx *ctx, const int32_t *pairs, int P);
/* Steered BRIEF: rotation-invariant descriptors by patch orientation (k_steer.hip).  Not in the C# reference, whose BRIEF
 * applies one table upright at every keypoint; this is ORB's remedy for camera roll, stated in integers so that the mode is
 * bit-identical to a CPU restatement (tests/steered_ref.py) with no tolerance anywhere.  Off by default; with it off nothing
 * changes.
 *
 * A steering table has B directions, with 4 <= B <= 64 and B % 4 == 0.  It holds:
 *   - dirs int32 [B][2] = (cx, cy), every component in [-32767, 32767];
 *   - pairs_rot int32 [B][P][4] in the layout of pgx_set_brief_pairs, with P = the context's current P;
 *   - a disc radius R, 1 <= R <= 31.
 * Steps 1-4 apply to a keypoint at (x, y) on a float32 grey image:
 *   1. q(g).  NaN -> 0; clamp to [0, 1]; ONE float32 multiplication by 65535.0f; round to nearest even; convert to int.  In
 *      numpy: np.rint(np.float32(clipped) * np.float32(65535)).  For the pipeline's own grey (sum / 196605) this is the channel
 *      mean in 16 bits.
 *   2. Moments.  m10 = sum of dx * q(pixel(x+dx, y+dy)) and m01 = sum of dy * q(...), over all integer (dx, dy) with
 *      dx^2 + dy^2 <= R^2.  A pixel outside the image contributes 0.  Each moment is below 2^31 in magnitude for R <= 31: the
 *      sum over dx > 0 of dx * 65535 on the R = 31 disc is 1 290 253 080.  Every partial sum lies between the negative part
 *      and the positive part of the total.  int32 accumulation in any order is therefore exact.
 *   3. Direction.  s_k = (int64)m10 * dirs[k][0] + (int64)m01 * dirs[k][1], and |s_k| < 2^46.  bin = the smallest k with the
 *      largest s_k.  A flat patch, with all s_k = 0, gets bin 0.
 *   4. Descriptor.  Exactly the existing rule (bit order, the "either end point outside -> bit 0" rule, the < on the original
 *      float32 values) applied with the table pairs_rot[bin].
 *
 * pgx_set_brief_steering uploads the tables and, when P == 256, builds one row-sorted sample plan per direction.
 * pairs_rot == NULL turns the mode off.  It needs pgx_set_brief_pairs first (PGX_E_NOT_CONFIGURED), and a later
 * pgx_set_brief_pairs turns the mode off, because the turned tables belong to the old table.  Bad B, radius or dirs:
 * PGX_E_BADARG.  With the mode on, pgx_brief, pgx_detect, pgx_detect_batch_dev and pgx_sequence_step_dev write steered
 * descriptors; keypoints, counts and order are unchanged. */
int pgx_set_brief_steering(pgx_ctx *ctx, const int32_t *pairs_rot, const int32_t *dirs, int B, int radius);
/* Scale pyramid: scale-invariant keypoints by running the detect chain on a ladder of shrunk grey images (k_pyramid.hip).  Not
 * in the C# reference, whose chain is single-scale; this is ORB's remedy for a camera that moves toward or away from the
 * scene.  Everything below is integer arithmetic or single IEEE float32 operations, so the mode is bit-identical to a CPU
 * restatement (tests/pyramid_ref.py) with no tolerance anywhere.  Off by default; with it off nothing changes.
 *
 * pgx_set_pyramid(ctx, n_levels, step_q16): 1 <= n_levels <= 8; step_q16 is the scale step between neighbouring levels in
 * 16.16 fixed point, 69632 <= step_q16 <= 131072 (1.0625 ... 2.0; 78643 ~ 1.2, 92682 ~ sqrt 2).  Anything else is
 * PGX_E_BADARG.  n_levels == 1 turns the mode off.
 *
 *   1. Sizes.  W_0 = W, H_0 = H; W_l = (W_{l-1} * 65536) / step and H_l likewise, int64 floor division.  A level with
 *      W_l < 16 or H_l < 16 is empty (no keypoints), and so is every level after it; that is not an error.
 *   2. Scale back to level 0.  S_0 = 65536, S_l = (S_{l-1} * step + 32768) >> 16 in uint64.
 *   3. Resampling.  Level l is built from level l - 1; level 0 is the chain's grey.  For destination column x:
 *      q = ((2x + 1) * step - 65536) >> 1 in int64, x0 = q >> 16, x1 = min(x0 + 1, W_{l-1} - 1),
 *      fx = (float)(q & 65535) * 2^-16 (exact).  Rows alike give y0, y1, fy.  With a = src[y0][x0], b = src[y0][x1],
 *      c = src[y1][x0], d = src[y1][x1]:  t = a + fx * (b - a);  u = c + fx * (d - c);  out = t + fy * (u - t) -- nine
 *      float32 operations in that order, none contracted.  q >= 0 and x0 <= W_{l-1} - 1 hold for every size from 16 to
 *      65535 and every step in range.  At step 2.0 this is the 2 x 2 mean; at smaller steps it is the 2-tap bilinear filter
 *      ORB implementations use between neighbouring levels.
 *   4. Per level, on the level image of size (W_l, H_l), the existing chain runs unchanged: FAST at the context's
 *      threshold, NMS at the context's radius, then BRIEF or steered BRIEF.  pgx_set_capacity's raw limit and survivor
 *      limit apply to each level separately, with their usual meaning at that level.
 *   5. Merged list of a frame.  Levels follow each other in the order 0, 1, ..., each level's entries in its NMS order.
 *      An entry from level l at (x_l, y_l) carries pgx_keypoint.x = min(((2 x_l + 1) * S_l) >> 17, W - 1) and y likewise
 *      with H, so the geometry stages keep reading level-0 pixels; fast_score and value are the level image's, and the
 *      descriptor is evaluated on the level image.  d_counts[f] = min(total, capacity); a total above capacity raises
 *      PGX_E_CAPACITY at the next status check, with the first `capacity` entries intact.  d_nraw[f] is the sum over the
 *      levels.  Every entry's slot follows from the level counts alone: no atomic decides a placement.
 *
 * With the mode on, pgx_detect, pgx_detect_batch_dev, pgx_detect_batch_steered_dev (bins merged too) and
 * pgx_sequence_step_dev write the merged lists of rule 5. */
int pgx_set_pyramid(pgx_ctx *ctx, int n_levels, int step_q16);
/* Rules 1 and 2 on the host (no GPU work): dims_out [n_levels][2] = (W_l, H_l), (0, 0) for an empty level; scale_out
 * [n_levels] = S_l.  Either output may be NULL.  W or H outside [1, 65535], bad n_levels or step: PGX_E_BADARG. */
int pgx_pyramid_dims(int W, int H, int n_levels, int step_q16, int32_t *dims_out /*[n_levels][2]*/, int32_t *scale_out /*[n_levels]*/);
/* KeypointDetectionOptions.Threshold, RedundantKeypointEliminationOptions.SuppressionRadius. */
int pgx_set_detect_params(pgx_ctx *ctx, float threshold, int suppression_radius);
/* Per-frame limits of the fused detect path.  max_raw_per_frame: raw FAST hits kept for NMS.  A frame with more raises
 * PGX_E_CAPACITY at the next status check (which clears it); its d_nraw is still the true total, and its lists are those
 * of the first max_raw_per_frame hits in raster order (NMS, the survivors' order and the descriptors as if the later hits
 * did not exist), at every radius; the other frames of the call are unaffected, and rows at and beyond counts[f] are
 * not written.  max_keypoints_per_frame: survivor LIMIT -- a frame's list is cut to its first
 * max_keypoints_per_frame entries in NMS order without an error (a harness-side truncation: the reference has
 * no cap; default 2^20 = none).  Survivors beyond a call's own `capacity` still raise
 * PGX_E_CAPACITY. */
int pgx_set_capacity(pgx_ctx *ctx, int max_raw_per_frame, int max_keypoints_per_frame);
/* Image pairs per workspace chunk of pgx_match_batch_dev / pgx_sequence_step_dev (default 2048, [16, 4096]).  A job with
 * more pairs goes through in chunks; the chunk bounds the matcher's workspace (about 4.4 MiB per image pair at 4096 descriptors
 * a side -- 4 MiB of it the residual's distance matrix -- plus the allocator's 25 % slack: 11 GB at the default).  Chunks of 1024 pairs or more run one after the
 * other on the context's stream with ONE workspace; smaller chunks run their stages side by side on three streams with three
 * workspaces resident (the form for small-memory configurations: it hides nothing once a chunk fills the chip).
 * The per-pair finish is one workgroup per pair, so large chunks balance the CUs better.  Results do not depend on it. */
int pgx_set_match_chunk(pgx_ctx *ctx, int image_pairs_per_chunk);

/* ---- stage-granular host entry points (one reference function each) ------------------ */
/* DeWarp.ApplyDistortionMat<Rgba64> (DeWarp.cs:19-37) with the context's map. */
int pgx_dewarp(pgx_ctx *ctx, const uint16_t *rgba64, int W, int H, uint16_t *out_rgba64);
/* Matrix.Convert(Grayscale.FromRgba64) (Converters.cs:15-22, Grayscale.cs:19-23). */
int pgx_gray(pgx_ctx *ctx, const uint16_t *rgba64, int W, int H, float *out_gray);
/* KeypointDetection.Detect minus the BRIEF ctor work (KeypointDetection.cs:42-63): raster-order
 * hits.  *n_out = total hits; only min(*n_out, capacity) are written (PGX_E_CAPACITY if more). */
int pgx_fast(pgx_ctx *ctx, const float *gray, int W, int H,
             pgx_keypoint *out, int capacity, int *n_out);
/* Keypoint.GetBriefDescriptor (Keypoint.cs:29-57) for n keypoints -> desc [n][ceil(P/32)]. */
int pgx_brief(pgx_ctx *ctx, const float *gray, int W, int H,
              const pgx_keypoint *kps, int n, uint32_t *desc_out);
/* Steps 1-3 of steered BRIEF for n keypoints -> bins_out [n] (not in the C# reference); PGX_E_NOT_CONFIGURED when the mode
 * is off.  A keypoint may lie anywhere: pixels outside the image contribute 0. */
int pgx_orient(pgx_ctx *ctx, const float *gray, int W, int H,
               const pgx_keypoint *kps, int n, int32_t *bins_out);
/* Level `level` of a host grey image under the context's pyramid step (rule 3 of pgx_set_pyramid, applied `level` times;
 * level 0 is a copy).  out [H_l][W_l], sized by the caller from pgx_pyramid_dims.  Not in the C# reference.
 * PGX_E_NOT_CONFIGURED when the mode is off; PGX_E_BADARG when level is negative, at or beyond n_levels, or names an
 * empty level. */
int pgx_pyramid_level(pgx_ctx *ctx, const float *gray, int W, int H, int level, float *out);
/* RedundantKeypointEliminator.EliminateRedundantKeypoints (:16-35): order_out[k] = index into
 * kps of the k-th accepted keypoint; *n_out = accepted count (order_out holds n entries). */
int pgx_nms(pgx_ctx *ctx, const pgx_keypoint *kps, int n, int W, int H,
            int32_t *order_out, int *n_out);
/* KeypointMatching.MatchKeypoints (KeypointMatching.cs:14-69): exactly n1 entries in the
 * reference's emission order; (0, 0, PGX_DIST_NONE) tail when n1 > n2; PGX_E_EMPTY_SET when
 * n2 == 0 < n1.  words = uint32 words per descriptor. */
int pgx_match(pgx_ctx *ctx, const uint32_t *desc1, int n1, const uint32_t *desc2, int n2,
              int words, pgx_pair *out);

/* KeypointMatching.MatchKeypoints for n_pairs image pairs in ONE call, host buffers ("Call sites": the batched
 * form a P/Invoke host with managed arrays calls instead of n_pairs x pgx_match -- one upload, one enqueue of the batched
 * matcher, one download).  descs[f] = frame f's descriptors [counts[f]][words] (may be NULL when counts[f] == 0);
 * pair_list [n_pairs][2] = (frame_a, frame_b).  out receives the lists back to back in pair order: list m has counts[a_m]
 * entries and starts at out_offsets[m] (out_offsets [n_pairs + 1], optional; the caller sizes out as the sum of counts[a_m]).
 * A pair with counts[b] == 0 < counts[a] gets counts[a] entries (0, 0, PGX_DIST_NONE) and the call returns PGX_E_EMPTY_SET
 * after all lists are written (the reference would have thrown at that pair, KeypointMatching.cs:61). */
int pgx_match_batch(pgx_ctx *ctx, const uint32_t *const *descs, const int32_t *counts, int n_frames, int words,
                    const int32_t *pair_list, int n_pairs, pgx_pair *out, int64_t *out_offsets);

/* ---- fused host entry point: dewarp -> gray -> detect -> NMS -> BRIEF for one image ---- */
/* The chain of TestService.BuildKeypointDetectorPipeline (TestService.cs:137-152).
 * kp_out [capacity], desc_out [capacity][ceil(P/32)]; *n_out survivors in NMS order,
 * *n_raw raw FAST hits. */
int pgx_detect(pgx_ctx *ctx, const uint16_t *rgba64, int W, int H,
               pgx_keypoint *kp_out, uint32_t *desc_out, int capacity, int *n_out, int *n_raw);

/* ---- device-resident batched entry points (asynchronous on the context's stream) ------ */
/* Stream hand-off contract: the context's own stream is NON-BLOCKING (it does not order against the null stream
 * or any other stream).  Every "_dev" input must be complete, and every output buffer free to be written, on the
 * context's stream when the call is made: either hand the library the stream that produced them
 * (pgx_set_stream) or synchronise the producer first.  Results are defined after pgx_check_status() (or after
 * the caller synchronises that stream). */
/* F frames [F][H][W][4] uint16 in HBM -> per frame up to `capacity` survivors.
 * d_kp [F][capacity], d_desc [F][capacity][words], d_counts [F], d_nraw [F] (all device). */
int pgx_detect_batch_dev(pgx_ctx *ctx, const uint16_t *d_rgba64, int F, int W, int H,
                         pgx_keypoint *d_kp, uint32_t *d_desc, int32_t *d_counts,
                         int32_t *d_nraw, int capacity);
/* The same chain in steered mode (PGX_E_NOT_CONFIGURED when it is off); it also writes each survivor's direction bin,
 * d_bins [F][capacity].  Not in the C# reference. */
int pgx_detect_batch_steered_dev(pgx_ctx *ctx, const uint16_t *d_rgba64, int F, int W, int H,
                                 pgx_keypoint *d_kp, uint32_t *d_desc, int32_t *d_counts,
                                 int32_t *d_nraw, int capacity, int32_t *d_bins);
/* The same chain in pyramid mode (PGX_E_NOT_CONFIGURED when it is off), with where every entry of the merged lists came
 * from: d_origin [F][capacity][3] = (level, x_l, y_l) on the level image; d_level_stats [F][n_levels][2] = (entries of the
 * level in the frame's list, raw FAST hits of the level), (0, 0) for an empty level.  d_bins [F][capacity] or NULL; a
 * non-NULL d_bins needs steering on (PGX_E_NOT_CONFIGURED).  Not in the C# reference. */
int pgx_detect_batch_pyramid_dev(pgx_ctx *ctx, const uint16_t *d_rgba64, int F, int W, int H,
                                 pgx_keypoint *d_kp, uint32_t *d_desc, int32_t *d_counts,
                                 int32_t *d_nraw, int capacity, int32_t *d_origin, int32_t *d_level_stats, int32_t *d_bins);
/* M image pairs: d_pairlist [M][2] = (frame_a, frame_b) indexes descriptor sets
 * d_desc [F][stride][words] with d_counts [F].  d_out [M][stride]: the first counts[a] entries of
 * row m are the reference's match list for (a, b).  Pairs with counts[b] == 0 < counts[a] raise
 * PGX_E_EMPTY_SET in pgx_check_status and leave their row filled with (0,0,PGX_DIST_NONE).
 * max_count = an upper bound of every d_counts entry used (<= stride; pass stride if unknown):
 * it only sizes the launch grids, counts above it are clamped to it. */
int pgx_match_batch_dev(pgx_ctx *ctx, const uint32_t *d_desc, const int32_t *d_counts,
                        int stride, int words, const int32_t *d_pairlist, int M, int max_count,
                        pgx_pair *d_out);
/* Stage ordering between TWO contexts on one GPU (consecutive jobs kept in flight, each context on its own stream): `ctx`'s
 * stream waits until stage `stage` of `other`'s most recent call of that kind has finished on the device (no wait if it has
 * run none): PGX_STAGE_DETECT = the detect chain of pgx_detect_batch_dev; PGX_STAGE_MATCH_WIDE / _ROWS / _DONE = the whole-chip
 * distance rounds / the residual distance rows / everything of pgx_match_batch_dev (the stages of pgx_sequence_step_dev count
 * the same way).  What the measurements say ("Two jobs in flight"; bench.py --gate): the productive overlap is job
 * k + 1's detect chain BESIDE job k's distance kernel -- that kernel's 256-thread workgroups mix with the detect chain's -- so job
 * k + 1's pgx_detect_batch_dev needs NO wait at all, and its matcher is held back with
 * pgx_gate_match(ctx, other, PGX_STAGE_MATCH_ROWS) until job k's residual distance rows are written: the next distance kernel
 * then runs beside job k's per-pair finish (round 5: 7.13 ms per bench step; waiting for PGX_STAGE_MATCH_DONE 7.21, for
 * PGX_STAGE_MATCH_WIDE only -- the rows kernel beside the next distance kernel, both on the matrix pipe -- 7.49; no gate at all:
 * two distance kernels at once, slower still).  pgx_wait_stage remains for hosts that want another order.  The
 * reference has the same shape on the CPU: ApplyDistortionMat of image k + 1 runs beside Detect of image k
 * (TestService.cs:25,146-149).  Ordering only: results do not depend on it.
 * Memory: every context owns its workspaces.  The matcher's is about 5.5 MiB per image pair of a chunk at 4096 descriptors a
 * side (4 MiB of it the residual's byte matrix; allocations carry 25 % slack): 11 GB at the default chunk of 2048 pairs, so two
 * contexts in flight hold 22 GB plus their own output buffers -- sized for the 288 GB of an MI355X; pgx_set_match_chunk
 * lowers it.  Each context also holds its own dewarp table and gather plan (12 B per pixel, pgx_set_dewarp_map). */
enum { PGX_STAGE_DETECT = 0, PGX_STAGE_MATCH_WIDE = 1, PGX_STAGE_MATCH_ROWS = 2, PGX_STAGE_MATCH_DONE = 3 };
int pgx_wait_stage(pgx_ctx *ctx, pgx_ctx *other, int stage);
/* The same wait, placed INSIDE ctx's next matcher call (pgx_match_batch_dev / pgx_sequence_step_dev; one shot): between its
 * init kernel -- which touches ctx's own workspace only and so runs ahead, beside whatever `other` still has on the chip -- and
 * its first whole-chip distance round, which then starts the moment the gate opens (with pgx_wait_stage in front of the call the
 * init kernel sits on the critical path: 0.2 ms per step of the bench job).  `other` must outlive that call. */
int pgx_gate_match(pgx_ctx *ctx, pgx_ctx *other, int stage);

/* ---- exact nearest-neighbour matching (k_knn.hip) --------------------------------------------------------------------- */
/* A second matching mode beside the reference's greedy one-to-one assignment (pgx_match*): per image pair the nearest columns
 * of every row and the nearest row of every column, and from them a match list with a distance gate, Lowe's ratio test and a
 * mutual (cross) check.  Not in the C# reference; the reference's Python matcher (keypoint_matching.py) keeps a row's nearest
 * column under --match-threshold.
 * Inputs as for pgx_match_batch_dev: d_desc [F][stride][words], d_counts [F], d_pairlist [M][2] = (a, b), max_count (counts
 * above it are clamped to it).  For image pair m = (a, b), row i < counts[a], column j < counts[b]:
 * d(i, j) = popcount(desc_a[i] ^ desc_b[j]).  Every result is exact and does not depend on launch configuration or run.
 *   row neighbours  the k in {1, 2} columns with the smallest (d, j), ascending in (d, j): a tie goes to the smaller index.
 *                   Missing entries (counts[b] < k) are (-1, PGX_DIST_NONE).
 *   column nearest  for every column j < counts[b] the row with the smallest (d, i); -1 when counts[a] == 0.
 *   NN list         one pgx_pair per row, entry i for row i: (i, j1, d1) when the row is accepted, else (i, -1, PGX_DIST_NONE)
 *                   (pgx_tracks_dev / pgx_tracks_add_pair never link such an entry).  Accepted when d1 <= max_dist; and,
 *                   with ratio > 0, there is no second neighbour or (double)d1 < (double)ratio * (double)d2 (exact: d <= 4064;
 *                   two equal nearest distances are rejected); and, with cross_check != 0, column-nearest(j1) == i.
 *                   ratio <= 0: no ratio test; ratio > 1 or NaN: PGX_E_BADARG.
 * counts[b] == 0 < counts[a] is NOT an error here: every row of the pair is rejected.  Rows >= counts[a] (columns >= counts[b]
 * of the column output) are not written.  Limits: stride <= 2^20, 1 <= words <= 127; k other than 1, 2 -> PGX_E_BADARG.
 * 256-bit descriptors (words == 8) run on the FP4 matrix instruction with the top-2 and the column argmin fused into the tile
 * loop (no distance matrix in memory); other lengths on a plain xor + popcount path. */
/* Asynchronous on the context's stream, stream hand-off contract as above.  d_idx, d_dist [M][stride][k]; d_col_nn [M][stride]
 * or NULL. */
int pgx_knn_batch_dev(pgx_ctx *ctx, const uint32_t *d_desc, const int32_t *d_counts, int stride, int words, const int32_t *d_pairlist,
                      int M, int max_count, int k, int32_t *d_idx, int32_t *d_dist, int32_t *d_col_nn);
/* The NN lists (k = 2 and the column nearest, then the selection above): d_out [M][stride], the first counts[a] entries of row m
 * are pair m's list, ready for pgx_tracks_dev as they are.  Workspace: 20 bytes per slot of a chunk of pgx_set_match_chunk pairs. */
int pgx_match_nn_batch_dev(pgx_ctx *ctx, const uint32_t *d_desc, const int32_t *d_counts, int stride, int words,
                           const int32_t *d_pairlist, int M, int max_count, int max_dist, float ratio, int cross_check,
                           pgx_pair *d_out);
/* Host buffers, one pair (the form a C# host with managed arrays calls, like pgx_match): idx_out, dist_out [n1][k],
 * col_nn_out [n2] or NULL.  Returns when the results are in the caller's buffers. */
int pgx_knn(pgx_ctx *ctx, const uint32_t *desc1, int n1, const uint32_t *desc2, int n2, int words, int k, int32_t *idx_out,
            int32_t *dist_out, int32_t *col_nn_out);

/* ---- epipolar-guided exact matching (k_guided.hip) -------------------------------------------------------------------- */
/* The nearest-neighbour mode above restricted, per image pair, to the columns that lie near each row's epipolar line, so that
 * a descriptor repeated elsewhere in the image no longer spoils the ratio test.  Inputs as for pgx_knn_batch_dev, plus
 * d_kp [F][stride] (the pgx_detect_batch_dev layout, same stride as the descriptors), d_F [M][9] float32 row-major with
 * h_a^T F h_b = 0, h = (x, y, 1) -- the convention of pgx_fundamental_ransac_dev's score -- and band, in pixels.  Its d_F is
 * accepted as it is, but its estimate keeps the reference's column-major fill: the matrix it fits to true correspondences
 * satisfies h_b^T F h_a = 0, so pass its transpose (or the pair swapped) to guide by it.
 * For image pair m = (a, b), row i at (x, y) = kp_a[i], column j at (u, v) = kp_b[j], every value converted to double and every
 * operation one IEEE double operation rounded to nearest, in the order written, none contracted into an FMA:
 *   l0 = (F[0][0]*x + F[1][0]*y) + F[2][0]      (the products are exact in double)
 *   l1 = (F[0][1]*x + F[1][1]*y) + F[2][1]
 *   l2 = (F[0][2]*x + F[1][2]*y) + F[2][2]
 *   n2 = l0*l0 + l1*l1;  e = (l0*u + l1*v) + l2;  T = (double)band * (double)band
 *   admissible(i, j)  <=>  all nine F entries finite  and  n2 > 0  and  e*e <= T*n2
 * (numpy float64 reproduces this bit for bit.)
 *   row neighbours  the k in {1, 2} ADMISSIBLE columns with the smallest (d, j); missing entries are (-1, PGX_DIST_NONE).
 *   column nearest  the admissible row with the smallest (d, i), -1 when there is none (the row's line decides on both sides).
 *   NN list         the selection rules of pgx_match_nn_batch_dev (distance gate, ratio, cross-check) on these neighbours.
 * Errors: band NaN, infinite or negative, and every argument pgx_knn_batch_dev rejects -> PGX_E_BADARG.  A keypoint coordinate
 * outside [-2^20, 2^20) in a used slot (index < counts) of frame a or b rejects all rows of that pair and reports
 * PGX_E_BADARG through pgx_check_status.  A pair with a non-finite F is not an error: all its rows are rejected.  Results do
 * not depend on pgx_set_match_chunk, the launch configuration or the run.  Rows >= counts[a] (columns >= counts[b]) are not
 * written.  The kernel buckets every frame of a chunk once into a grid and walks only the cells the band crosses.
 * Asynchronous on the context's stream.  d_idx, d_dist [M][stride][k]; d_col_nn [M][stride] or NULL.  Workspace: the grids
 * of the frames of one chunk of image pairs, about 10 bytes per keypoint slot (max_count) of 2 * chunk frames. */
int pgx_knn_guided_batch_dev(pgx_ctx *ctx, const uint32_t *d_desc, const pgx_keypoint *d_kp, const int32_t *d_counts, int stride,
                             int words, const int32_t *d_pairlist, int M, int max_count, const float *d_F, float band, int k,
                             int32_t *d_idx, int32_t *d_dist, int32_t *d_col_nn);
/* The guided NN lists: d_out [M][stride] as pgx_match_nn_batch_dev's, ready for pgx_tracks_dev. */
int pgx_match_guided_batch_dev(pgx_ctx *ctx, const uint32_t *d_desc, const pgx_keypoint *d_kp, const int32_t *d_counts, int stride,
                               int words, const int32_t *d_pairlist, int M, int max_count, const float *d_F, float band,
                               int max_dist, float ratio, int cross_check, pgx_pair *d_out);
/* Host buffers, one pair (frame a = 1, frame b = 2): F [9]; idx_out, dist_out [n1][k], col_nn_out [n2] or NULL.  Returns when
 * the results are in the caller's buffers (PGX_E_BADARG for an out-of-range coordinate). */
int pgx_knn_guided(pgx_ctx *ctx, const uint32_t *desc1, const pgx_keypoint *kp1, int n1, const uint32_t *desc2,
                   const pgx_keypoint *kp2, int n2, int words, const float *F, float band, int k, int32_t *idx_out,
                   int32_t *dist_out, int32_t *col_nn_out);

/* ---- RANSAC fundamental matrix and camera pose, batched over image pairs (asynchronous, device pointers) --- */
/* CameraPoseEstimation.GetFundamentalMatrix (CameraPoseEstimation.cs:26-94) for M image pairs at once: `keypointPairs` of
 * image pair m = the first counts[a] entries of d_matches[m] (indices into d_kp[a] / d_kp[b], (a, b) = d_pairlist[m]); per
 * sample a subset of pairs_per_sample DISTINCT list positions, the normalised 8-point estimate (EstimateFundamentalMatrix,
 * :204-250, incl. its always-1 scale and column-major fill), the signed score (F * p2) . p1 <= threshold over the whole list
 * (:67-77); the first sample with the most inliers wins.  rank_check != 0 keeps only matrices of numerical rank 2 like
 * :46-51 (with noisy pairs that rejects nearly every sample -- the reference then throws; here d_inliers[m] = -1).
 * The reference draws subsets from an unseeded System.Random and singular vectors from MathNet's SVD: `seed` replaces the
 * former, a Jacobi eigen-solver with a fixed sign rule the latter (parity unpinned).  d_F [M][9] row-major;
 * d_inliers[m] = -1 when the list is shorter than pairs_per_sample (:31-32) or no sample qualified (:88-89).
 * pairs_per_sample < 8 -> PGX_E_BADARG (:28-29). */
int pgx_fundamental_ransac_dev(pgx_ctx *ctx, const pgx_keypoint *d_kp /* [F][stride] */, const pgx_pair *d_matches /* [M][stride] */,
                               const int32_t *d_counts /* [F] */, const int32_t *d_pairlist /* [M][2] */, int M, int stride,
                               int n_samples, int pairs_per_sample, float threshold, int rank_check, uint64_t seed,
                               float *d_F, int32_t *d_inliers, int32_t *d_best_sample);
/* CameraPoseEstimation.EstimateCameraPose (:96-202): E = K^T F K with the reference's hard-coded K, the four (R, t)
 * candidates, linear triangulation of every keypoint pair, vote on z >= 0.  d_Rt [M][12] = R row-major then t of the
 * winning candidate, d_votes [M][4], d_best [M]; d_points [M][stride][3] (or NULL) = the winner's point cloud (the input of
 * Utils.CreatePointCloud, :199). */
int pgx_pose_dev(pgx_ctx *ctx, const pgx_keypoint *d_kp, const pgx_pair *d_matches, const int32_t *d_counts,
                 const int32_t *d_pairlist, int M, int stride, const float *d_F, float *d_Rt, int32_t *d_votes,
                 int32_t *d_best, float *d_points);

/* ---- multi-GPU: one process and one context per GPU; the context owns the RCCL communicator -------- */
/* The reference handles one image pair in one process (TestService.cs:80-96) and nothing couples image pairs, so the
 * path shards with no collective inside detect or match: frame f -> rank f mod G, image pair p -> rank p mod G, and two
 * exchanges of FIXED-SIZE records (per-frame {count, descriptors}; per-pair match lists -- always exactly N1 entries,
 * KeypointMatching.cs:38), both in-place all-gathers over a rank-major buffer [G][slots][...]: global item k sits in
 * block k mod G at place k / G.  librccl is loaded on first use; without it these calls return PGX_E_RCCL. */
#define PGX_COMM_ID_BYTES 128
/* Rank 0 makes the id (ncclGetUniqueId); the host hands the 128 bytes to every rank (socket, file, MPI, ...). */
int pgx_comm_unique_id(void *id_out /* [PGX_COMM_ID_BYTES] */);
/* Collective over all ranks (ncclCommInitRank on the context's device). */
int pgx_comm_init(pgx_ctx *ctx, int rank, int world, const void *id /* [PGX_COMM_ID_BYTES] */);
int pgx_comm_destroy(pgx_ctx *ctx);
int pgx_comm_info(pgx_ctx *ctx, int *rank, int *world);   /* (0, 1) without a communicator */
/* In-place all-gather on the context's stream: this rank's record is bytes [rank * bytes_per_rank, +bytes_per_rank) of
 * d_buf [world * bytes_per_rank].  world == 1: no-op. */
int pgx_allgather_dev(pgx_ctx *ctx, void *d_buf, size_t bytes_per_rank);
/* The four phases of one job, enqueued on the context's stream: detect this rank's n_local_frames frames into its block
 * of d_desc_all [world * frame_slots][capacity][words] / d_counts_all [world * frame_slots]; all-gather both; match this
 * rank's n_local_pairs image pairs (d_pairlist_local [n][2] = SLOT indices into the gathered buffers) into its block of
 * d_out_all [world * pair_slots][capacity]; all-gather the lists.  Lists are cut to `capacity` by pgx_set_capacity's
 * survivor limit (set it <= capacity).  world == 1: the same without the collectives.
 * Errors at world > 1: every rank-local check and allocation happens before the first collective, and the first call with a
 * given set of arguments ends that part with a status exchange among the ranks: if any rank fails there, EVERY rank returns
 * (the failing one its own code, the others PGX_E_RCCL naming it) and nothing has been exchanged.  A HIP / RCCL failure later
 * in the step aborts this rank's communicator (best effort: peers blocked in a collective may not notice on one node -- the
 * host must put a time limit on its ranks) and leaves the context without one. */
int pgx_sequence_step_dev(pgx_ctx *ctx, const uint16_t *d_frames_local, int n_local_frames, int frame_slots, int W, int H,
                          pgx_keypoint *d_kp_local, uint32_t *d_desc_all, int32_t *d_counts_all, int32_t *d_nraw_local,
                          int capacity, const int32_t *d_pairlist_local, int n_local_pairs, int pair_slots,
                          pgx_pair *d_out_all);

/* ---- the track graph over the gathered match lists -------------------------------------------------- */
/* Not in the reference (TestService.cs:80-96 handles one image pair); north_star names it as the consumer of the
 * gathered lists.  What the reference does hold is the distance gate: python_src/scripts/match_keypoints.py:23,127
 * (`--match-threshold`), `new KeypointMatching(100)` in the commented code of Photogrammetry/Program.cs:165,224.
 * Semantics -- order-independent, so the device build and the sequential host build below give the same result bit for bit:
 *   nodes   (frame, keypoint) with keypoint < counts[frame]
 *   edges   entry e < counts[a] of image pair (a, b)'s list links (a, k1) with (b, k2) when dist <= max_dist; the
 *           (0, 0, PGX_DIST_NONE) tail entries (KeypointMatching.cs:40-42) never link, whatever max_dist is
 *   tracks  connected components with at least min_len nodes; a component that holds two keypoints of ONE frame is
 *           inconsistent and dropped as a whole (counted, its nodes marked -2)
 *   order   tracks by their first (frame, keypoint), nodes inside a track ascending.
 *
 * Device form (asynchronous on the context's stream, device pointers): the lists are used where the matcher / the all-gather
 * left them.  d_matches [M][stride], d_counts [F], d_pairlist [M][2] exactly as for pgx_match_batch_dev (pair m's frames are
 * SLOT indices into d_counts).  d_frame_ids [F] (or NULL = identity, n_frames = F) maps a slot to the frame NUMBER the graph
 * uses, in [0, n_frames), distinct; -1 = this slot is not part of the graph (padding slots of the rank-major gathered buffers;
 * frames of sequences another rank builds the graph for): image pairs that touch such a slot are skipped.  Outputs:
 *   d_track_of [n_frames][stride]   track index of every node; -1 = no track (beyond counts, or a component below min_len),
 *                                   -2 = dropped with its inconsistent component
 *   d_offsets  [n_frames*stride+1]  the first n_tracks + 1 entries: track t's nodes are d_nodes[d_offsets[t] .. d_offsets[t+1])
 *   d_nodes    [n_frames*stride][2] (frame, keypoint)
 *   d_summary  [8]                  n_tracks, n_nodes, dropped components, nodes in them, edges used, longest track,
 *                                   largest dropped component, 0
 * n_frames * stride <= 2^30.  min_len < 1 counts as 1. */
int pgx_tracks_dev(pgx_ctx *ctx, const pgx_pair *d_matches, const int32_t *d_counts, const int32_t *d_pairlist, int M, int F,
                   int stride, const int32_t *d_frame_ids, int n_frames, int max_dist, int min_len,
                   int32_t *d_track_of, int32_t *d_offsets, int32_t *d_nodes, int32_t *d_summary);

/* Split mode: inconsistent components are split at tighter gates instead of dropped whole.
 * Inputs: the same as pgx_tracks_dev, plus n_gates refinement gates with max_dist > gates[0] > gates[1] > ... > gates[n-1] >= 0
 * and 0 <= n_gates <= 7.  Write g_0 = max_dist and g_l = gates[l-1].
 *   E_l     the match entries that pgx_tracks_dev would use as edges at gate g_l.  These are the same filters as today:
 *           e < counts[a], k1 and k2 in range, never the PGX_DIST_NONE tail and never k2 = -1 rows of NN lists.  The only
 *           change is dist <= g_l.  So E_0 ⊇ E_1 ⊇ ... ⊇ E_n.
 *   C_l(x)  the connected component of node x in (nodes, E_l).  Components nest: C_l(x) ⊆ C_{l-1}(x).
 *   level   the level of x is the smallest l for which C_l(x) is consistent, meaning it has at most one keypoint per frame.
 *           If x has a level, its group is C_level(x).  Every node of that group has the same level and the same group, so
 *           the groups partition the nodes that have a level.
 *   tracks  the groups with at least min_len nodes.  Nodes of smaller groups get -1.  Nodes with no level (C_n(x) is still
 *           inconsistent) get -2 and count as dropped.
 *   order   the same as today: tracks are sorted by first (frame, keypoint), and nodes inside a track ascend.
 * This is a cut of the single-linkage hierarchy at the coarsest consistent level among the given gates.  It does not depend
 * on the order in which edges are processed.  With n_gates = 0 it is exactly pgx_tracks_dev.
 * gates is a HOST array [n_gates].  Unordered gates, a gate at or above max_dist, a negative gate or n_gates outside [0, 7]:
 * PGX_E_BADARG.  Layouts and argument checks as pgx_tracks_dev; asynchronous on the context's stream.  In this mode the slots
 * of d_frame_ids must name distinct frames: two slots naming one frame are reported as PGX_E_BADARG by pgx_check_status.
 *   d_summary [16]  [0..7] as pgx_tracks_dev: [2], [3] and [6] are the components still inconsistent at the last gate, [4]
 *                   counts the edges of E_0, [7] is 0.  [8 + l] = nodes in tracks whose level is l (unused slots 0);
 *                   [8] + ... + [15] = [1]. */
int pgx_tracks_split_dev(pgx_ctx *ctx, const pgx_pair *d_matches, const int32_t *d_counts, const int32_t *d_pairlist, int M, int F,
                         int stride, const int32_t *d_frame_ids, int n_frames, int max_dist, const int32_t *gates, int n_gates,
                         int min_len, int32_t *d_track_of, int32_t *d_offsets, int32_t *d_nodes, int32_t *d_summary);

/* Host form, no GPU work (small inputs; a host that holds the lists in managed memory): the same semantics, sequential.
 * counts [n_frames] = keypoints per frame. */
typedef struct pgx_tracks pgx_tracks;
int  pgx_tracks_create(const int32_t *counts, int n_frames, pgx_tracks **out);
void pgx_tracks_destroy(pgx_tracks *t);
/* matches: the first n entries of one image pair's list (n = counts[frame_a]).  The gated edges (node a, node b, dist) are
 * kept in the object, so that pgx_tracks_finish_split can recompute the levels. */
int  pgx_tracks_add_pair(pgx_tracks *t, int frame_a, int frame_b, const pgx_pair *matches, int n, int max_dist);
/* Closes the graph: *n_tracks consistent components of at least min_len nodes with *n_nodes nodes in all. */
int  pgx_tracks_finish(pgx_tracks *t, int min_len, int *n_tracks, int *n_nodes);
/* After either finish call. */
int  pgx_tracks_get(pgx_tracks *t, int32_t *track_offsets /* [n_tracks + 1] */, int32_t *nodes /* [n_nodes][2] = (frame, keypoint) */);
/* The split mode's host form (the rule of pgx_tracks_split_dev; level 0 = the edges as added).  gates [n_gates], strictly
 * decreasing, >= 0, n_gates in [0, 7], else PGX_E_BADARG.  An edge that was added with a per-pair max_dist smaller than
 * gates[l] enters level l only if its distance is also within that pair's max_dist: g_l of a pair is min(its max_dist, g_l).
 * (This follows from pgx_tracks_add_pair keeping only the entries within the pair's max_dist.)
 * summary [16] as d_summary of pgx_tracks_split_dev (or NULL).  Closes the graph like pgx_tracks_finish; more edges may be
 * added and either finish call made again. */
int  pgx_tracks_finish_split(pgx_tracks *t, const int32_t *gates, int n_gates, int min_len, int *n_tracks, int *n_nodes,
                             int32_t *summary /* [16] */);
/* After either finish call: inconsistent components (at the last gate) and the nodes in them (what d_summary[2], [3] report
 * on the device). */
int  pgx_tracks_dropped(pgx_tracks *t, int *n_components, int *n_nodes);

/* ---- multi-view triangulation of tracks ------------------------------------------------ */
/* The reference's end product is a point cloud: CameraPoseEstimation.EstimateCameraPose (CameraPoseEstimation.cs:96-202)
 * triangulates every keypoint pair of ONE image pair and hands the points to Utils.CreatePointCloud.  This is the same step
 * for the tracks of the graph above, over any number of views, with the caller's cameras.
 * Inputs:
 *   d_offsets, d_nodes, d_track_summary   the outputs of pgx_tracks_dev / pgx_tracks_split_dev, unchanged.  Only
 *           d_track_summary[0] = n_tracks is read, and on the device, so the call can follow the graph on the same stream.
 *   d_kp [F][stride]     the keypoints in the pgx_detect_batch_dev layout.
 *   d_frame_ids [F]      the array the graph call took (NULL = identity, n_frames = F): nodes name frame NUMBERS, keypoints
 *           sit in SLOTS.  Two slots naming one frame: PGX_E_BADARG through pgx_check_status.
 *   d_P [n_frames][12]   float64, row-major 3x4, by frame number: world point -> pixels in the keypoint convention, column
 *           u = pgx_keypoint.x, row v = pgx_keypoint.y (exact doubles).  Write M = P[:, 0:3], p4 = P[:, 3], m3 = M's 3rd row.
 *           A camera is UNKNOWN if an entry is not finite or det(M) == 0; observations in its frame are skipped (pass NaN rows
 *           for the frames that have no pose yet).
 * Per track, over its used observations i = (u_i, v_i, P_i) in d_nodes order, with C_i = -M_i^-1 p4_i (the adjugate over
 * det) and S = the mean of the used C_i:
 *   1 linear  in the frame shifted to S, P'_i = [M_i | p4_i + M_i S].  Rows u_i P'_i[2] - P'_i[0] and v_i P'_i[2] - P'_i[1],
 *             each divided by its Euclidean norm; v = the unit null vector of the 2n x 4 system (smallest eigenvector of its
 *             Gram matrix).  |v[3]| <= 1e-12 or a non-finite v: DEGENERATE.  Else X' = v[0:3] / v[3].
 *   2 refine  refine_iters in [0, 32] Gauss-Newton steps on cost(X') = sum_i e_i^2, each from the 3x3 normal equations
 *             J^T J d = -J^T r.  Before a step: stop if ||d|| <= 1e-12 (1 + ||S + X'||).  A step is kept only if the cost
 *             strictly decreases; otherwise X' stays and refinement stops.  X = S + X'.
 *   3 quality e_i = the pixel distance between (u_i, v_i) and the projection of X; depth_i = sign(det M_i) (P_i[2].(X, 1)) /
 *             ||m3_i||; parallax = the largest angle in degrees between C_i - X and C_j - X over pairs of used observations.
 *   4 flags   (PGX_TRI_*, bits; 0 = a valid point)
 *             FEWVIEWS    fewer than 2 used observations: no point, xyz, quality and the track's node errors are NaN
 *             DEGENERATE  step 1 found the point at infinity: xyz, quality and node errors NaN
 *             BEHIND      some depth_i <= 0
 *             PARALLAX    parallax < min_parallax_deg
 *             REPROJ      not (max e_i <= max_reproj_px)  (+inf disables it)
 * Outputs, for t < min(n_tracks, max_tracks):
 *   d_xyz [max_tracks][3], d_quality [max_tracks][3] = (rms e, max e, parallax) float64, d_flags [max_tracks] int32;
 *   d_node_err [n_frames * stride] float64 or NULL: e_i in d_nodes order, NaN for a skipped observation;
 *   d_summary [8] int32: tracks processed, tracks with flags 0, tracks carrying each of the five bits (FEWVIEWS first),
 *           observations used.
 * Errors through pgx_check_status: n_tracks > max_tracks (PGX_E_CAPACITY; the first max_tracks are written); a node whose
 * frame is outside [0, n_frames), whose keypoint is outside [0, stride) or whose frame no slot names (PGX_E_BADARG; the node is
 * skipped).  Returned at once (PGX_E_BADARG): refine_iters outside [0, 32], min_parallax_deg < 0 or NaN, max_reproj_px <= 0
 * or NaN, null required pointers, F, stride or n_frames not positive, n_frames * stride > 2^30, max_tracks < 0.
 * Results depend on the inputs only: the same bits for any max_tracks >= n_tracks, any slot layout of the same frames, from
 * run to run, and from the host form below.  Asynchronous on the context's stream. */
#define PGX_TRI_FEWVIEWS   1
#define PGX_TRI_DEGENERATE 2
#define PGX_TRI_BEHIND     4
#define PGX_TRI_PARALLAX   8
#define PGX_TRI_REPROJ     16
int pgx_triangulate_tracks_dev(pgx_ctx *ctx, const pgx_keypoint *d_kp, int F, int stride, const int32_t *d_frame_ids, int n_frames,
                               const double *d_P, const int32_t *d_offsets, const int32_t *d_nodes, const int32_t *d_track_summary,
                               int max_tracks, double min_parallax_deg, double max_reproj_px, int refine_iters, double *d_xyz,
                               double *d_quality, int32_t *d_flags, double *d_node_err, int32_t *d_summary);
/* Host form (what a host calls after pgx_tracks_get): the same kernels on host arrays, returns when the results are in the
 * caller's buffers.  kps = every frame's keypoints one after another (frame f's counts[f] entries start at counts[0] + ... +
 * counts[f-1]); P [n_frames][12]; track_offsets [n_tracks + 1], nodes [track_offsets[n_tracks]][2] as pgx_tracks_get writes
 * them.  A node outside [0, n_frames) x [0, counts[frame]) or offsets that are not non-decreasing from 0: PGX_E_BADARG before
 * any GPU work.  xyz [n_tracks][3], quality [n_tracks][3], flags [n_tracks], node_err [n_nodes] (or NULL), summary [8]. */
int pgx_triangulate_tracks(pgx_ctx *ctx, const pgx_keypoint *kps, const int32_t *counts, int n_frames, const double *P,
                           const int32_t *track_offsets, const int32_t *nodes, int n_tracks, double min_parallax_deg,
                           double max_reproj_px, int refine_iters, double *xyz, double *quality, int32_t *flags, double *node_err,
                           int32_t *summary);

/* ---- bundle adjustment of cameras and track points -------------------------------------- */
/* The stage after the triangulation: refines the free cameras and the points of the tracks together by minimising the
 * reprojection error (Levenberg-Marquardt), on the same stream, with no host sync.  It also writes P_out, so the caller can
 * triangulate again with the refined cameras.
 * Inputs: d_kp, F, stride, d_frame_ids, n_frames, d_offsets, d_nodes, d_track_summary and max_tracks as for
 * pgx_triangulate_tracks_dev (nodes name frame numbers, keypoints sit in slots; n_tracks = d_track_summary[0], read on the
 * device), and by frame number:
 *   d_K [n_frames][4]     fx, fy, cx, cy (float64): pinhole, fixed intrinsics
 *   d_Rt_in [n_frames][12] R row-major, then t (the layout of pgx_pose_dev's d_Rt, in float64).  With (x, y, z) = R X + t a
 *           point projects to u = fx (x / z) + cx, v = fy (y / z) + cy; u is pgx_keypoint.x, v is pgx_keypoint.y.
 *   d_fixed [n_frames]    != 0: the frame is held
 *   d_xyz_in [max_tracks][3], d_track_flags [max_tracks] (or NULL: all 0), e.g. pgx_triangulate_tracks_dev's xyz and flags
 * Frames.  UNKNOWN if an entry of its K or Rt is not finite or fx or fy is 0: its observations are skipped, its rows are
 * copied.  A finite R with max |R R^T - I| > 1e-9 or det R <= 0 is PGX_E_BADARG through pgx_check_status and the frame is
 * unknown.  A known frame with d_fixed != 0 is FIXED, the other known frames are FREE, numbered in frame order.  More than
 * 128 free frames: PGX_E_CAPACITY through pgx_check_status; no known fixed frame: PGX_E_BADARG the same way; in both cases no
 * iteration runs (stop reason 0).  One fixed frame leaves the scale free (the damping keeps the solves definite); two fix it.
 * Tracks.  Track t takes part if t < min(n_tracks, max_tracks), its flag is 0, xyz_in[t] is finite and it has >= 2 USED
 * observations (nodes in known frames).  The others are copied.  A node outside [0, n_frames) x [0, stride), in a frame no
 * slot names, or malformed offsets: PGX_E_BADARG through pgx_check_status, the node is skipped.  A track with two nodes in
 * one frame: PGX_E_BADARG the same way, the track does not take part.
 * Cost.  Per used observation r = projection - (u, v), s = |r|^2, rho(s) = s for s <= d^2 and 2 d sqrt(s) - d^2 above, with
 * d = huber_px (+inf: least squares); C = sum rho.  IRLS weights w = 1 or d / sqrt(s); A = sum w J^T J, g = sum w J^T r.
 * Parameters.  Free camera: (omega, tau), R' = Exp(omega) R (Rodrigues), t' = t + tau, so d(R X + t)/d omega = -[R X]x.
 * Point: X' = X + dX.
 * Levenberg-Marquardt.  Solve (A + lambda D) delta = -g, D = diag(clamp(diag A, 1e-6, 1e32)), by eliminating the 3x3 point
 * blocks (Schur complement), a Cholesky factorisation of the reduced camera system (<= 768 unknowns) and back-substitution.
 * Start: C = C0, lambda = lambda0, trace[0] = (C0, lambda0).  The stop test (first match wins) runs at the start and after
 * every attempted step: the call had an error or no track takes part (reason 0); C == 0, or the last step was accepted with
 * C_old - C_new <= 1e-12 C_old (reason 2); lambda > 1e16 (reason 4); max_iters steps attempted (reason 1).  An attempt:
 *   1 a point block or pivot of the damped system that is not positive definite: rejected, lambda *= 10, non-PD count + 1;
 *   2 else ||delta|| <= 1e-12 (1 + ||x||), x the stacked t of the free cameras and X of the points that take part: stop with
 *     reason 3, the step is not applied;
 *   3 else C_new = C at the trial state; C_new < C: accepted (lambda = max(lambda / 10, 1e-12), re-linearise); else
 *     rejected (lambda *= 10, the next attempt re-solves at the same linearisation).
 *   trace[i] = (C, lambda) after attempt i.
 * Outputs (out arrays may alias their in arrays):
 *   d_Rt_out [n_frames][12]  refined free cameras; fixed and unknown frames copied bit for bit
 *   d_P_out [n_frames][12]   K [R | t] of Rt_out for known frames (rows (fx r0 + cx r2, fy r1 + cy r2, r2)), NaN for unknown
 *   d_xyz_out [max_tracks][3] for t < min(n_tracks, max_tracks): the refined point, or xyz_in[t] for a track not taking part
 *   d_node_err [n_frames * stride] or NULL: the final |r| in d_nodes order, NaN for a node not used in a track taking part
 *   d_trace [max_iters + 1][2] (C, lambda); rows after the stop are NaN
 *   d_report [8] int32: attempted steps, accepted steps, stop reason, free frames, tracks taking part, used observations of
 *           those tracks, of them with z <= 0 at the end, non-PD solves
 * Returned at once (PGX_E_BADARG): max_iters outside [0, 100], huber_px <= 0 or NaN, lambda0 <= 0 or not finite, null
 * required pointers, and the size checks of pgx_triangulate_tracks_dev.
 * Results depend on the inputs only: the same bits for any max_tracks >= n_tracks, any slot layout, from run to run, and from
 * the host form below.  Asynchronous on the context's stream. */
int pgx_bundle_adjust_dev(pgx_ctx *ctx, const pgx_keypoint *d_kp, int F, int stride, const int32_t *d_frame_ids, int n_frames,
                          const double *d_K, const double *d_Rt_in, const int32_t *d_fixed, const int32_t *d_offsets,
                          const int32_t *d_nodes, const int32_t *d_track_summary, int max_tracks, const double *d_xyz_in,
                          const int32_t *d_track_flags, int max_iters, double huber_px, double lambda0, double *d_Rt_out,
                          double *d_P_out, double *d_xyz_out, double *d_node_err, double *d_trace, int32_t *d_report);
/* Host form: the same kernels on host arrays (the conventions of pgx_triangulate_tracks: kps concatenated by frame, tracks
 * as pgx_tracks_get writes them; a node outside [0, n_frames) x [0, counts[frame]) or offsets that are not non-decreasing
 * from 0: PGX_E_BADARG before any GPU work).  xyz_in / xyz_out [n_tracks][3], track_flags [n_tracks] or NULL, node_err
 * [n_nodes] or NULL; returns when the outputs are in the caller's buffers. */
int pgx_bundle_adjust(pgx_ctx *ctx, const pgx_keypoint *kps, const int32_t *counts, int n_frames, const double *K,
                      const double *Rt_in, const int32_t *fixed, const int32_t *track_offsets, const int32_t *nodes, int n_tracks,
                      const double *xyz_in, const int32_t *track_flags, int max_iters, double huber_px, double lambda0,
                      double *Rt_out, double *P_out, double *xyz_out, double *node_err, double *trace, int32_t *report);

/* ---- frame registration (absolute pose) by P3P RANSAC against track points ------------- */
/* Places frames that have no pose yet into the frame and scale of the existing reconstruction: the stage between two
 * triangulations of the incremental loop (known frames -> pgx_triangulate_tracks_dev -> this -> triangulate again on P_out
 * -> pgx_bundle_adjust_dev), on the same stream, with no host sync.
 * Inputs: d_kp, F, stride, d_frame_ids, n_frames, d_offsets, d_nodes, d_track_summary and max_tracks as for
 * pgx_bundle_adjust_dev (nodes name frame numbers, keypoints sit in slots; n_tracks = d_track_summary[0], read on the
 * device); d_K [n_frames][4] (fx, fy, cx, cy) and d_Rt_in [n_frames][12] (R row-major, then t; float64) in BA's
 * conventions: with (x, y, z) = R X + t a point projects to u = fx x / z + cx, v = fy y / z + cy (u = pgx_keypoint.x,
 * v = pgx_keypoint.y); d_register [n_frames]; d_xyz [max_tracks][3] and d_track_flags [max_tracks] (or NULL: all 0), e.g.
 * pgx_triangulate_tracks_dev's xyz and flags.
 * Targets.  Frame f is a target if d_register[f] != 0; d_Rt_in of a target is not read.  A target whose K has an entry
 * that is not finite or fx or fy == 0 is failed with PGX_REG_BADK and has no correspondences.  Every other frame is copied
 * bit for bit into Rt_out, with P_out = K [R | t] if its K passes that test and its Rt is finite, NaN otherwise.
 * Correspondences of target f, position j in this order: tracks t < min(n_tracks, max_tracks) in order, then the nodes of
 * each track in order; a node (f, k) is one if the track's flag is 0 and xyz[t] is finite: (u, v) = (kp.x, kp.y), X = xyz[t].
 * A track with two nodes in one target frame: PGX_E_BADARG through pgx_check_status, those nodes are skipped.  A node
 * outside [0, n_frames) x [0, stride), in a frame no slot names, malformed offsets, or two slots naming one frame:
 * PGX_E_BADARG through pgx_check_status, as in the triangulation (the node or track is skipped).
 * Shift.  S_f = the mean of the correspondences' X (a fixed-order sum), X' = X - S_f; the pose (R, t_S) is found in the
 * shifted world, and Rt_out's t = t_S - R S_f (each entry t_S[i] - ((R[i][0] S0 + R[i][1] S1) + R[i][2] S2)).
 * Samples.  For s in [0, n_samples): state = seed ^ ((uint64)f << 32) ^ (uint64)s * 0xD1B54A32D192ED03 (f the frame
 * number); draw splitmix64(state) % n (n = correspondences) until there are 3 distinct positions (k_pose.hip's generator).
 * Minimal solver.  P3P by Lambda Twist (Persson and Nordberg, ECCV 2018) on the unit bearings of ((u - cx) / fx,
 * (v - cy) / fy, 1) and the three X': the cubic's root by monotone Newton, the degenerate conic's eigenvectors by cross
 * products, up to 3 Newton steps on the depths, R = [Y1 - Y2, Y1 - Y3, (Y1 - Y2) x (Y1 - Y3)] [X'1 - X'2, X'1 - X'3, ...]^-1.
 * Every real solution with positive depth at its 3 points and finite entries is a hypothesis (at most 4 per sample); a
 * sample's solutions are ranked by ascending |t_S|^2 (ties: the solver's order), hypothesis h = 4 s + rank.
 * Inlier predicate (no division, evaluated in this order): x = ((R00 X'0 + R01 X'1) + R02 X'2) + tS0, y and z alike;
 * a = fx * x + (cx - u) * z, b = fy * y + (cy - v) * z, e = inlier_px * z; inlier iff z > 0 and a * a + b * b <= e * e.
 * Winner: the most inliers, ties to the smallest h (integers only: the grid and the summation order do not matter).
 * Refinement: up to refine_iters Gauss-Newton steps on the winner's inlier set with pixel residuals r = (fx (x / z) +
 * (cx - u), fy (y / z) + (cy - v)), R' = Exp(omega) R, t_S' = t_S + tau (BA's parameterisation), a 6x6 Cholesky solve.  A
 * step is kept only if the sum of r^2 over that set strictly falls; the refinement stops at the first step not kept, when
 * ||delta|| <= 1e-12 (1 + ||t_S||), or when the Cholesky solve is not positive definite.  The final inlier set is the
 * predicate at the refined pose.
 * Failure: fewer than 3 correspondences PGX_REG_FEWPOINTS; no hypothesis at all PGX_REG_NOSOLUTION; fewer than min_inliers
 * final inliers PGX_REG_FEWINLIERS.  A failed target has NaN rows in Rt_out and P_out (the triangulation and BA treat it as
 * unknown).
 * Outputs:
 *   d_Rt_out, d_P_out [n_frames][12]  P rows (fx r0 + cx r2, fy r1 + cy r2, r2) of [R | t], as BA writes them
 *   d_frame_stats [n_frames][4] int32: correspondences, final inliers, winning sample or -1, PGX_REG_* flags;
 *           (-1, -1, -1, -1) for a frame that is not a target
 *   d_frame_err [n_frames][2]   rms and max of |r| over the final inliers; NaN when there are none
 *   d_node_inlier [n_frames * stride] or NULL, in d_nodes order for the nodes of tracks t < min(n_tracks, max_tracks): 1 a
 *           final inlier, 0 an outlier correspondence, -1 not a correspondence of a target
 *   d_report [8] int32: targets, registered targets, targets carrying each flag bit (BADK first), correspondences of all
 *           targets, final inliers of all targets
 * Returned at once (PGX_E_BADARG): n_samples outside [1, 65536], inlier_px <= 0 or not finite, min_inliers < 3,
 * refine_iters outside [0, 32], null required pointers, and the size checks of pgx_triangulate_tracks_dev.
 * n_tracks > max_tracks: PGX_E_CAPACITY through pgx_check_status, the first max_tracks tracks are used.
 * Results depend on the inputs only: the same bits for any max_tracks >= n_tracks, any slot layout, from run to run, and
 * from the host form below.  Asynchronous on the context's stream. */
#define PGX_REG_BADK       1
#define PGX_REG_FEWPOINTS  2
#define PGX_REG_NOSOLUTION 4
#define PGX_REG_FEWINLIERS 8
int pgx_register_frames_dev(pgx_ctx *ctx, const pgx_keypoint *d_kp, int F, int stride, const int32_t *d_frame_ids, int n_frames,
                            const double *d_K, const double *d_Rt_in, const int32_t *d_register, const int32_t *d_offsets,
                            const int32_t *d_nodes, const int32_t *d_track_summary, int max_tracks, const double *d_xyz,
                            const int32_t *d_track_flags, int n_samples, double inlier_px, int min_inliers, int refine_iters,
                            uint64_t seed, double *d_Rt_out, double *d_P_out, int32_t *d_frame_stats, double *d_frame_err,
                            int32_t *d_node_inlier, int32_t *d_report);
/* Host form: the same kernels on host arrays (the conventions of pgx_bundle_adjust: kps concatenated by frame, tracks as
 * pgx_tracks_get writes them; a node outside [0, n_frames) x [0, counts[frame]) or offsets that are not non-decreasing
 * from 0: PGX_E_BADARG before any GPU work).  xyz [n_tracks][3], track_flags [n_tracks] or NULL, node_inlier [n_nodes] or
 * NULL; returns when the outputs are in the caller's buffers. */
int pgx_register_frames(pgx_ctx *ctx, const pgx_keypoint *kps, const int32_t *counts, int n_frames, const double *K,
                        const double *Rt_in, const int32_t *reg, const int32_t *track_offsets, const int32_t *nodes, int n_tracks,
                        const double *xyz, const int32_t *track_flags, int n_samples, double inlier_px, int min_inliers,
                        int refine_iters, uint64_t seed, double *Rt_out, double *P_out, int32_t *frame_stats, double *frame_err,
                        int32_t *node_inlier, int32_t *report);

/* ---- track consensus: drop outlier observations from tracks ----------------------------- */
/* A track with one wrong observation is otherwise lost whole: the triangulation can only flag it (PGX_TRI_REPROJ), and bundle
 * adjustment and registration skip flagged tracks.  This stage sits between either graph call and the triangulation (tracks
 * -> consensus -> triangulate -> BA -> register -> triangulate -> consensus -> ...), needs cameras but no points, and
 * writes a graph with fewer nodes: per track a small deterministic RANSAC over pairs of views, then an ordered compaction.
 * Not in the reference.
 * Inputs: d_kp, F, stride, d_frame_ids, n_frames, d_P, d_offsets, d_nodes, d_track_summary and max_tracks as for
 * pgx_triangulate_tracks_dev (n_tracks = d_track_summary[0], read on the device).
 * Values.  Every value is a double, every operation one IEEE double operation in the order written; a sum of three terms is
 * ((a + b) + c), a dot product ((x0 y0 + x1 y1) + x2 y2); nothing is contracted into a fused multiply-add.
 * Frames.  A frame is KNOWN by the triangulation's test: all 12 entries finite and det M != 0, det M = (m00 k00 + m01 k01) +
 * m02 k02 over the cofactors k of M's first row.  Per known frame Minv = adj(M) / det (every entry divided), C = -(Minv p4),
 * each component -((Minv[r][0] p4[0] + Minv[r][1] p4[1]) + Minv[r][2] p4[2]), and sgn = +1 for det M > 0, else -1.
 * Observations.  The known observations of a track are its nodes in known frames, in d_nodes order, at positions
 * 0 .. n_k - 1.  The ray of observation i = (u, v) is d_i = sgn * ((Minv[:,0] u + Minv[:,1] v) + Minv[:,2]).  Nodes in unknown
 * frames are never judged and always carried over (registration needs them later).
 * Hypotheses.  n_p = n_k (n_k - 1) / 2.  If n_p <= max_hyp, hypothesis h is the h-th pair (i, j), i < j, in lexicographic
 * order (exhaustive).  Otherwise, for h < max_hyp: state = seed ^ ((uint64)(uint32)t << 32) ^ (uint64)(uint32)h *
 * 0xD1B54A32D192ED03 (t the track's index in the input), draw splitmix64(state) % n_k until there are 2 distinct positions
 * (registration's generator); i is the smaller, j the larger.  With w0 = C_i - C_j, a = d_i.d_i, b = d_i.d_j, c = d_j.d_j,
 * dd = d_i.w0, e = d_j.w0, den = a c - b b, a hypothesis is VALID unless it is rejected, in this order:
 *   1 b > 0 and b b >= cos2 (a c), cos2 = the square of cos(min_parallax_deg pi / 180), computed once on the host;
 *   2 not den > 0;
 *   3 s = (b e - c dd) / den, tt = (a e - b dd) / den: not (s > 0 and tt > 0).
 * Its point relative to C_i is X' = 0.5 (s d_i + (tt d_j - w0)): the midpoint of the two rays' closest points.
 * Score.  Known observation m = (u, v) is an inlier of a hypothesis with y = X' + (C_i - C_m), h = M_m y (rows in order),
 * w = h2, a' = h0 - u w, b' = h1 - v w, e' = inlier_px w: inlier iff sgn_m w > 0 and a' a' + b' b' <= e' e'.  No division and
 * no p4: a translated scene decides the same way.  A camera with det M < 0 is read as the negative of a proper camera, as the
 * triangulation's depth does: -P decides exactly as P, and a mirrored K (fx < 0) has its points behind it.
 * Winner: the valid hypothesis with the most inliers, ties to the smallest h (an integer key: the grid, the lane mapping and
 * the summation order cannot matter).
 * Per track (PGX_CNS_* bits in d_track_stats):
 *   FEWVIEWS     n_k < 2: the track passes through unchanged
 *   LOWPARALLAX  no valid hypothesis: passes through unchanged (a track that cannot be judged yet is not a wrong track)
 *   NOCONSENSUS  the winner has fewer than min_inliers inliers: the whole track is removed
 *   otherwise    every known observation that is not an inlier of the winner is removed.
 *   SHORT        (with any of the above but NOCONSENSUS) fewer than min_len nodes are left, counting the nodes in unknown
 *                frames: the track is removed.  min_len < 1 counts as 1.
 * Order.  Surviving tracks keep their relative order, surviving nodes theirs.  Once a track's first node is removed the
 * output is NO LONGER SORTED by first node (pgx_tracks_dev's order); the triangulation, bundle adjustment and registration
 * walk tracks by index and nodes by position and do not rely on it.
 * Outputs (none may alias an input: d_offsets_out == d_offsets, d_nodes_out == d_nodes or d_summary_out == d_track_summary
 * is PGX_E_BADARG), for t < min(n_tracks, max_tracks):
 *   d_offsets_out [max_tracks + 1], d_nodes_out [n_frames * stride][2], d_summary_out [8]  the layout of pgx_tracks_dev, so the
 *           triangulation, BA and registration take them unchanged: [0] tracks, [1] nodes, [5] the longest track; [2], [3],
 *           [4], [6] copied from d_track_summary; [7] = 0
 *   d_track_map [max_tracks]     old index -> new index, or -1
 *   d_xyz_out [max_tracks][3], d_flags_out [max_tracks]  by the NEW index: the winner's point in world coordinates, each
 *           component X' + C_i, and flag 0; NaN and PGX_TRI_FEWVIEWS for a track that passed through.  Registration or BA
 *           can follow directly without a triangulation in between
 *   d_track_stats [max_tracks][4] by the OLD index: known observations, the winner's inliers, the winning h or -1, PGX_CNS_*
 *   d_track_of [n_frames][stride] or NULL, in place, for the nodes of the processed tracks: a node of a removed track
 *           becomes -1, a removed node of a surviving track -3, any other node its track's new index
 *   d_report [8]  tracks in, tracks out, nodes in, nodes out, outlier observations removed (of the tracks that reached a
 *           consensus), NOCONSENSUS tracks, SHORT tracks, tracks that passed through undecided (FEWVIEWS or LOWPARALLAX)
 * Errors through pgx_check_status: n_tracks > max_tracks (PGX_E_CAPACITY; the first max_tracks tracks are processed); a node
 * outside [0, n_frames) x [0, stride) or in a frame no slot names (PGX_E_BADARG; the node is dropped from the output),
 * malformed offsets (the track counts as empty) or two slots naming one frame, as in the triangulation.  Returned at once
 * (PGX_E_BADARG): inlier_px not positive or not finite, min_parallax_deg outside [0, 90), min_inliers < 2, max_hyp outside
 * [1, 4096], null required pointers, aliased outputs, and the size checks of pgx_triangulate_tracks_dev.
 * Results depend on the inputs only: the same bits for any max_tracks >= n_tracks, any slot layout, from run to run, and
 * from the host form below.  Asynchronous on the context's stream. */
#define PGX_CNS_FEWVIEWS    1
#define PGX_CNS_LOWPARALLAX 2
#define PGX_CNS_NOCONSENSUS 4
#define PGX_CNS_SHORT       8
int pgx_track_consensus_dev(pgx_ctx *ctx, const pgx_keypoint *d_kp, int F, int stride, const int32_t *d_frame_ids, int n_frames,
                            const double *d_P, const int32_t *d_offsets, const int32_t *d_nodes, const int32_t *d_track_summary,
                            int max_tracks, double inlier_px, double min_parallax_deg, int min_inliers, int min_len, int max_hyp,
                            uint64_t seed, int32_t *d_offsets_out, int32_t *d_nodes_out, int32_t *d_summary_out,
                            int32_t *d_track_map, double *d_xyz_out, int32_t *d_flags_out, int32_t *d_track_stats,
                            int32_t *d_track_of, int32_t *d_report);
/* Host form (what a host calls after pgx_tracks_get): the same kernels on host arrays (the conventions of
 * pgx_triangulate_tracks: kps concatenated by frame, tracks as pgx_tracks_get writes them; a node outside [0, n_frames) x
 * [0, counts[frame]) or offsets that are not non-decreasing from 0: PGX_E_BADARG before any GPU work).  offsets_out
 * [n_tracks + 1], nodes_out [n_nodes][2], summary_out [8] (slots 2, 3, 4 and 6 are 0) and report [8] are required; track_map
 * [n_tracks], xyz_out [n_tracks][3], flags_out [n_tracks] and track_stats [n_tracks][4] may be NULL.  Returns when the
 * outputs are in the caller's buffers. */
int pgx_track_consensus(pgx_ctx *ctx, const pgx_keypoint *kps, const int32_t *counts, int n_frames, const double *P,
                        const int32_t *track_offsets, const int32_t *nodes, int n_tracks, double inlier_px, double min_parallax_deg,
                        int min_inliers, int min_len, int max_hyp, uint64_t seed, int32_t *offsets_out, int32_t *nodes_out,
                        int32_t *summary_out, int32_t *track_map, double *xyz_out, int32_t *flags_out, int32_t *track_stats,
                        int32_t *report);

/* ---- two-view geometric verification of match lists by epipolar RANSAC ----------------- */
/* The stage between a matcher and the track graph: per image pair a robust fundamental matrix, the match list with
 * everything but its inliers rejected (ready for pgx_tracks_dev), and F in the guided matcher's convention (d_F32 is
 * accepted by pgx_match_guided_batch_dev as it is).  Not in the C# reference.
 * Inputs: d_kp, d_matches, d_counts, d_pairlist, M, stride and max_dist as for pgx_tracks_dev; (a, b) = d_pairlist[m].
 * Values.  Every value is a double, every operation one IEEE double operation in the order written, nothing is contracted
 * into a fused multiply-add.
 * Candidates.  Entry e < clamp(counts[a], 0, stride) of list m is a candidate when 0 <= k1 < counts[a], 0 <= k2 < counts[b]
 * (both counts clamped to [0, stride]), dist <= max_dist and dist != PGX_DIST_NONE: pgx_tracks_dev's filters of an edge.
 * Candidates keep their list order and get positions 0 .. n-1; with (x, y) = kp_a[k1] and (u, v) = kp_b[k2] a candidate gives
 * h_a = (x, y, 1) and h_b = (u, v, 1).  n < 8: PGX_VER_FEWMATCHES (and no other flag).
 * Samples.  For s in [0, n_samples): state = seed ^ ((uint64)(uint32)a << 32) ^ (uint64)(uint32)b * 0x9E3779B97F4A7C15 ^
 * (uint64)s * 0xD1B54A32D192ED03; draw splitmix64(state) % n until there are 8 distinct positions (k_pose.hip's generator).
 * The stream depends on the pair's slots, not on its place in the list.
 * Fit: the normalised 8-point algorithm with rank 2 enforced, on a set S of correspondences.  Per image, c = the mean point
 * and dbar = the mean of sqrt((x - cx)^2 + (y - cy)^2) (sums in the set's order for a sample, in a fixed launch-independent
 * order for a refit); sc = sqrt(2) / dbar, dbar == 0 makes the set invalid; T = [[sc, 0, -sc cx], [0, sc, -sc cy], [0, 0, 1]],
 * hh = T h (hh0 = sc x + (-(sc cx))); the row of a correspondence is r = (hha0 hhb0, hha0 hhb1, hha0, hha1 hhb0, hha1 hhb1,
 * hha1, hhb0, hhb1, 1); G = sum r r^T; f = the eigenvector of G's smallest eigenvalue (cyclic Jacobi, sign: largest
 * component positive); Fh = f row-major; v3 = the same of Fh^T Fh; Fh' = Fh - (Fh v3) v3^T; F = Ta^T Fh' Tb divided by its
 * Frobenius norm.  A non-finite entry makes the fit invalid; an invalid sample has count -1 and a NaN F.
 * Inlier predicate (the Sampson distance with no division and no square root), evaluated in this order:
 *   m0 = (F00 u + F01 v) + F02;  m1 = (F10 u + F11 v) + F12;  m2 = (F20 u + F21 v) + F22;  e = (x m0 + y m1) + m2
 *   l0 = (F00 x + F10 y) + F20;  l1 = (F01 x + F11 y) + F21;  d = ((l0 l0 + l1 l1) + m0 m0) + m1 m1;  T = inlier_px inlier_px
 *   inlier iff d > 0 and e e <= T d
 * Winner: the valid sample with the most inliers over all n candidates, ties to the smallest s (integers only: the grid
 * does not matter).  No valid sample: PGX_VER_NOMODEL.
 * Refit, up to refit_iters times: the fit on the whole current inlier set if it has at least 8 members; the new F is kept
 * only if the fit is valid and its inlier count is strictly greater, otherwise the refits stop.
 * Final inliers < min_inliers: PGX_VER_FEWINLIERS.  A pair that carries any flag is rejected whole.
 * Outputs:
 *   d_out [M][stride]  for e < clamp(counts[a], 0, stride): the input entry if it is a candidate, a final inlier and the pair
 *           is accepted, (k1 of the input entry, -1, PGX_DIST_NONE) otherwise (never linked by the track graph); entries at
 *           and beyond that are not written.  d_out may alias d_matches.
 *   d_F [M][9]         the final F row-major: NaN for FEWMATCHES and NOMODEL, kept for FEWINLIERS
 *   d_F32 [M][9] or NULL  d_F rounded to float32
 *   d_stats [M][8] int32: n candidates, the winner's count, the final count, the winning sample or -1, the flags, refits
 *           kept, valid samples, 0 (counts are 0 without a winner)
 *   d_inlier [M][stride] or NULL, for the entries d_out writes: 1 candidate and final inlier (of the final F, also in a
 *           rejected pair), 0 candidate and outlier, -1 not a candidate
 *   d_sample_F [M][n_samples][9], d_sample_count [M][n_samples], each or NULL: every sample's F (NaN when invalid) and count
 *   d_report [8] int32: pairs, accepted pairs, pairs with FEWMATCHES, with NOMODEL, with FEWINLIERS, candidates of all
 *           pairs, final inliers of accepted pairs, 0
 * Returned at once (PGX_E_BADARG): n_samples outside [1, 65536], inlier_px <= 0 or not finite, min_inliers < 8, refit_iters
 * outside [0, 8], M < 0, stride outside [1, 2^20], a null required pointer.  A pair with counts[a] == 0 is FEWMATCHES.
 * Results depend on the inputs only: the same bits from run to run, for any order of the pair list, for any
 * pgx_set_match_chunk, and from the host form below.  Asynchronous on the context's stream. */
#define PGX_VER_FEWMATCHES 1   /* fewer than 8 candidate entries */
#define PGX_VER_NOMODEL    2   /* no sample gave a finite F */
#define PGX_VER_FEWINLIERS 4   /* final inliers < min_inliers */
int pgx_verify_pairs_dev(pgx_ctx *ctx, const pgx_keypoint *d_kp, const pgx_pair *d_matches, const int32_t *d_counts,
                         const int32_t *d_pairlist, int M, int stride, int max_dist, int n_samples, double inlier_px,
                         int min_inliers, int refit_iters, uint64_t seed, pgx_pair *d_out, double *d_F, float *d_F32,
                         int32_t *d_stats, int32_t *d_inlier, double *d_sample_F, int32_t *d_sample_count, int32_t *d_report);
/* Host form: one pair on host arrays, the same kernels with frame a in slot 1 and frame b in slot 2 (so the bits are those
 * of the device form for the pair (1, 2)).  matches, out and inlier hold n1 entries; F [9], stats [8]; inlier may be NULL.
 * n1 or n2 < 0 or above 2^20: PGX_E_BADARG.  Returns when the outputs are in the caller's buffers. */
int pgx_verify_pair(pgx_ctx *ctx, const pgx_keypoint *kp1, int n1, const pgx_keypoint *kp2, int n2, const pgx_pair *matches,
                    int max_dist, int n_samples, double inlier_px, int min_inliers, int refit_iters, uint64_t seed, pgx_pair *out,
                    double *F, int32_t *stats, int32_t *inlier);

/* ---- relative pose per image pair and the choice of the initial pair ------------------- */
/* The start of a reconstruction: turns verification's F and the intrinsics into the first two cameras, so that the chain
 * pgx_verify_pairs_dev -> pgx_tracks_dev -> this -> pgx_triangulate_tracks_dev -> pgx_bundle_adjust_dev ->
 * pgx_register_frames_dev runs on one stream with no host round trip.  No RANSAC of its own (verification ran one) and no
 * refinement (bundle adjustment with one fixed frame does that).  Not in the C# reference.
 * Inputs: d_kp [F][stride], d_matches [M][stride] (meant: verification's d_out), d_counts [F], d_pairlist [M][2] (slots), M,
 * F, stride, d_frame_ids [F] or NULL, n_frames and max_dist as for pgx_tracks_dev; (a, b) = d_pairlist[m];
 *   d_F [M][9]          float64, verification's d_F: h_a^T F h_b = 0
 *   d_K [n_frames][4]   fx, fy, cx, cy by frame NUMBER, as pgx_bundle_adjust_dev takes it
 *   min_angle_deg in [0, 90), min_front_frac in (0, 1], min_points >= 1.
 * Values.  Every value is a double, every operation one IEEE double operation in the order written, nothing is contracted
 * into a fused multiply-add; dot products are summed as ((.0 + .1) + .2).
 * Per pair m:
 *   1 flags   (PGX_INIT_*, bits; 0 = eligible)
 *             SKIPPED     a slot outside [0, F), a == b, or a slot whose frame number is -1 (or otherwise outside
 *                         [0, n_frames)); no other flag is set with it and nothing else of the pair is read
 *             BADINPUT    an entry of F, K_a or K_b is not finite, or some fx or fy is 0; no other flag is set with it
 *             DEGENERATE  step 4 failed; no other flag is set with it
 *             FEWFRONT, FEWPOINTS  step 6; both can be set on one pair
 *   2 candidates  exactly pgx_verify_pairs_dev's: entry e < clamp(counts[a], 0, stride) with 0 <= k1 < counts[a], 0 <= k2 <
 *             counts[b] (both clamped to [0, stride]), dist <= max_dist and dist != PGX_DIST_NONE, in list order; there are n.
 *             With (x, y) = kp_a[k1], (u, v) = kp_b[k2] the unnormalised bearings are g_a = ((x - cx_a) fy_a, (y - cy_a) fx_a,
 *             fx_a fy_a) with s_a = fx_a fy_a, and g_b, s_b alike: no division.
 *   3 E = K_a^T F K_b: the rows of A = K_a^T F are fx_a F[0], fy_a F[1], (cx_a F[0] + cy_a F[1]) + F[2]; the columns of E are
 *             A[:,0] fx_b, A[:,1] fy_b, (A[:,0] cx_b + A[:,1] cy_b) + A[:,2].  G = E^T, so that g_b^T G g_a = 0 and G is
 *             proportional to [t]x R for x_b = R x_a + t.  Gh = G / sqrt(the sum of its squares, row-major from 0).
 *   4 decomposition  B = Gh^T Gh (B[i][j] = the dot product of columns i and j); its eigenpairs by cyclic Jacobi
 *             (pgx_verify_pairs_dev's solver, N = 3), ordered by eigenvalue descending, ties to the lower column;
 *             sigma_i = sqrt(max(lambda_i, 0)).  DEGENERATE if an entry of Gh, an eigenvalue or an entry of a candidate is not
 *             finite, or sigma_2 <= 1e-6 sigma_1.  u1 = (Gh v1) / sigma_1; w = Gh v2, u2 = (w - (u1 . w) u1) / its norm;
 *             v3 = v1 x v2, u3 = u1 x u2.  R1[i][j] = (u2[i] v1[j] - u1[i] v2[j]) + u3[i] v3[j] (= U W V^T, W = [[0, -1, 0],
 *             [1, 0, 0], [0, 0, 1]]), R2[i][j] = (u1[i] v2[j] - u2[i] v1[j]) + u3[i] v3[j] (= U W^T V^T), t = u3, |t| = 1.
 *             Candidates c = 0..3 = (R1, t), (R1, -t), (R2, t), (R2, -t).
 *   5 score of a candidate (R, t) on one match, with no division and no square root:
 *             p = R g_a;  a11 = p . p;  c = p . g_b;  a12 = -c;  a22 = g_b . g_b;  r1 = -(p . t);  r2 = g_b . t
 *             det = a11 a22 - a12 a12;  na = r1 a22 - a12 r2;  nb = a11 r2 - a12 r1
 *             front  iff det > 0 and na s_a > 0 and nb s_b > 0 (both depths positive)
 *             wide   iff front and ((c s_a) s_b <= 0 or c c <= cos2 (a11 a22)): the angle between the two rays is at least
 *                    min_angle_deg; cos2 = the square of the host C library's cos(min_angle_deg * (M_PI / 180)).
 *             The ray angle does not depend on t: a pair related by a pure rotation has no wide point, whatever its t.
 *   6 winner  the candidate with the most front points, ties to the smallest c.  FEWFRONT if (double)front <
 *             min_front_frac * (double)n; FEWPOINTS if the winner's wide count < min_points.  Only integers are summed: the
 *             grid and the order of the sums do not matter.
 * Choice.  Among the pairs with flags 0 the largest wide count; ties to the smaller frame number of a, then of b, then the
 * smaller m (integer keys; with distinct pairs the choice does not depend on the order of the pair list).  Call it m*, its
 * frames a*, b*.
 * Outputs, per pair:
 *   d_Rt_pair [M][12]      the winner, R row-major then t; NaN for SKIPPED, BADINPUT and DEGENERATE
 *   d_pair_stats [M][8]    int32: n, front[0..3], the winner's wide count, the winner c or -1, the flags.  n is counted for
 *                          every pair but a SKIPPED one; the other counts are 0 without a winner
 *   d_sigma [M] or NULL    sigma_2 / sigma_1; NaN when it was not computed (SKIPPED, BADINPUT, a non-finite Gh or eigenvalue)
 *   d_cand_Rt [M][4][12] or NULL  the four candidates; NaN where d_Rt_pair is
 * per frame number, ready for the next calls (NaN and 0 throughout when no pair is eligible, which is no error):
 *   d_Rt_out, d_P_out [n_frames][12]  frame a* = [I | 0], frame b* = [R | t] of m*, every other frame NaN; P = K [R | t] with
 *                          the rows (fx r0 + cx r2, fy r1 + cy r2, r2), as pgx_bundle_adjust_dev writes them
 *   d_fixed_out [n_frames]     int32: 1 for a*, else 0
 *   d_register_out [n_frames]  int32: 1 for every frame that some slot names other than a* and b*, else 0
 *   d_report [8] int32: pairs, pairs with flags 0, SKIPPED or BADINPUT, DEGENERATE, FEWFRONT, FEWPOINTS, m* or -1, the wide
 *                          count of m* (0 without one)
 * Returned at once (PGX_E_BADARG): min_angle_deg outside [0, 90), min_front_frac outside (0, 1], either NaN, min_points < 1,
 * M < 0, stride outside [1, 2^20], F or n_frames not positive, no d_frame_ids and n_frames != F, n_frames * stride > 2^30, a
 * null required pointer.
 * Results depend on the inputs only: the same bits from run to run, for any order of the pair list (the choice then names the
 * same pair), any slot layout of the same frames, any n_frames that holds them, and from the host form below.  The workspace
 * is 304 bytes per pair, so pgx_set_match_chunk plays no part.  Asynchronous on the context's stream, no host sync. */
#define PGX_INIT_SKIPPED    1
#define PGX_INIT_BADINPUT   2
#define PGX_INIT_DEGENERATE 4
#define PGX_INIT_FEWFRONT   8
#define PGX_INIT_FEWPOINTS  16
int pgx_init_pair_dev(pgx_ctx *ctx, const pgx_keypoint *d_kp, const pgx_pair *d_matches, const int32_t *d_counts,
                      const int32_t *d_pairlist, int M, int F, int stride, const int32_t *d_frame_ids, int n_frames, int max_dist,
                      const double *d_F, const double *d_K, double min_angle_deg, double min_front_frac, int min_points,
                      double *d_Rt_pair, int32_t *d_pair_stats, double *d_sigma, double *d_cand_Rt, double *d_Rt_out,
                      double *d_P_out, int32_t *d_fixed_out, int32_t *d_register_out, int32_t *d_report);
/* Host form: one pair on host arrays, the same kernels with frame a in slot 1 and frame b in slot 2, like pgx_verify_pair (so
 * the bits are those of the device form).  matches holds n1 entries; F [9]; K_a, K_b [4]; Rt [12], stats [8], sigma [1],
 * cand_Rt [48] or NULL.  n1 or n2 < 0 or above 2^20: PGX_E_BADARG.  Returns when the outputs are in the caller's buffers. */
int pgx_relative_pose(pgx_ctx *ctx, const pgx_keypoint *kp1, int n1, const pgx_keypoint *kp2, int n2, const pgx_pair *matches,
                      int max_dist, const double *F, const double *K_a, const double *K_b, double min_angle_deg,
                      double min_front_frac, int min_points, double *Rt, int32_t *stats, double *sigma, double *cand_Rt);

/* ---- image-pair selection on a binary visual vocabulary ------------------------------ */
/* Which pairs of an unordered collection are worth matching: every matcher, verification and the track graph take
 * d_pairlist [M][2] from the caller, and all pairs stop scaling at a few dozen frames.  This is image retrieval as SfM
 * packages do it (quantise the descriptors against a vocabulary, score frames by their word histograms, match the best
 * partners), stated in integers so that it is bit-identical to a CPU restatement (tests/pairs_ref.py).  Not in the C#
 * reference.  k_vocab.hip.
 * Shared definitions.  Descriptors are 256-bit: 8 words each, descriptor bit t = bit t % 32 of word t / 32.
 *   d_desc [F][stride][8], d_counts [F]; slots f < F, n_f = clamp(d_counts[f], 0, stride); 1 <= stride <= 65535,
 *   1 <= F <= 4096, 1 <= V <= 65536, anything else PGX_E_BADARG.  A slot with n_f == 0 takes part in nothing.
 *   d(x, y) = popcount(x ^ y) over the 8 words.
 *   word(f, i) = argmin over j < V of (d(desc[f][i], vocab[j]), j): a tie goes to the smaller j.
 *
 * pgx_vocab_quantize_dev: d_word[f][i] = word(f, i) and, with d_wdist not NULL, d_wdist[f][i] = its distance, for i < n_f;
 * entries i >= n_f are not written.  The exact Hamming argmin on the block-scaled FP4 matrix instruction; no workspace. */
int pgx_vocab_quantize_dev(pgx_ctx *ctx, const uint32_t *d_desc, const int32_t *d_counts, int F, int stride,
                           const uint32_t *d_vocab /*[V][8]*/, int V, int32_t *d_word /*[F][stride]*/,
                           int32_t *d_wdist /*[F][stride] or NULL*/);
/* pgx_vocab_train_dev: k-majority, the Hamming form of k-means; integers only, deterministic.
 *   N = the sum of n_f; rank g enumerates the valid descriptors by (f, i) ascending.
 *   Initialisation, in uint64: lo_j = (j N) / V, hi_j = ((j + 1) N) / V, state = seed ^ (uint64_t)j * 0xD1B54A32D192ED03,
 *     r_j = lo_j + splitmix64(state) % (hi_j - lo_j) (the splitmix64 of the RANSAC stages: state += 0x9E3779B97F4A7C15, then
 *     the two multiply-xorshift rounds); vocab[j] = the descriptor of rank r_j.
 *   One iteration: every valid descriptor gets its word by the rule above; for word j with c_j members of which ones_j[t]
 *     have bit t set, the new bit t is 1 if 2 ones > c, 0 if 2 ones < c, the old bit on equality; c_j == 0 leaves the word
 *     as it is.  All `iters` iterations run: no early stop, no host round trip.
 *   d_report [4] int32: N; words without a member in the last assignment (-1 at iters == 0); bits changed by the last
 *     iteration (-1 at iters == 0); 0.
 * iters outside [0, 64]: PGX_E_BADARG at once.  N < V is known on the device only: d_report[0] = N, d_vocab is not written
 * and pgx_check_status reports PGX_E_BADARG.  Workspace: 8 bytes per descriptor slot (F * stride) + 8 bytes per word.
 * The same bits for any stride layout of the same descriptors. */
int pgx_vocab_train_dev(pgx_ctx *ctx, const uint32_t *d_desc, const int32_t *d_counts, int F, int stride, int V, int iters,
                        uint64_t seed, uint32_t *d_vocab /*out [V][8]*/, int32_t *d_report /*[4]*/);
/* pgx_select_pairs_dev: the pair list of a collection.
 * Histograms and weights.  h_f[w] = the number of entries i < n_f with word(f, i) == w; Fv = the slots with n_f > 0;
 *   df[w] = the slots with h_f[w] > 0.  weighting == 0: q[w] = 1.  weighting == 1, an integer log2 of the inverse document
 *   frequency with a linear mantissa: q[w] = 0 where df[w] == 0, else x = (Fv 2^16) / df[w] in 64 bits, e = the index of the
 *   highest set bit of x, m = (x 2^8) / 2^e - 256, q[w] = 256 (e - 16) + m (a word in every frame weighs 0).  Any other
 *   weighting: PGX_E_BADARG.
 * Scores, in int64: self_f = sum_w q[w] h_f[w]; s(a, b) = sum_w q[w] min(h_a[w], h_b[w]);
 *   sn(a, b) = (s(a, b) 2^20) / max(1, min(self_a, self_b)), in [0, 2^20], symmetric.
 *   d_scores[a][b] = sn(a, b) for non-empty a != b, -1 on the diagonal and wherever a slot is empty.
 * Selection.  Slot a nominates the first min(top_k, .) of its candidates: the b != a with n_b > 0 and sn >= min_score, in
 *   (sn descending, b ascending) order.  A pair a < b of non-empty slots is selected when a nominates b, or b nominates a,
 *   or b - a <= window.  top_k >= 0, window >= 0 (else PGX_E_BADARG); top_k = 0 with window = w is the sliding-window list.
 * Output.  The selected pairs in lexicographic (a, b) order in d_pairlist [max_pairs][2], each with its sn in d_pair_score
 *   [max_pairs]; rows from the count to max_pairs hold (-1, -1) and -1.  More than max_pairs pairs: the first max_pairs are
 *   written and pgx_check_status reports PGX_E_CAPACITY.  A prefix of the list is what every d_pairlist consumer takes.
 *   d_summary [8] int32: pairs selected (the full count); Fv; words with df == 0; words with df == Fv; pairs selected by
 *   the window alone; the smallest sn among nominated pairs (-1: none); 0; 0.
 * Workspace: per slot 4 stride + 2 V + 32 bytes, per word 4 bytes, 8 F^2 bytes of raw scores, and 4 F^2 more when d_scores is
 * NULL. */
int pgx_select_pairs_dev(pgx_ctx *ctx, const uint32_t *d_desc, const int32_t *d_counts, int F, int stride,
                         const uint32_t *d_vocab, int V, int weighting, int top_k, int window, int min_score, int max_pairs,
                         int32_t *d_pairlist /*[max_pairs][2]*/, int32_t *d_pair_score /*[max_pairs]*/,
                         int32_t *d_scores /*[F][F] or NULL*/, int32_t *d_summary /*[8]*/);
/* Host forms: host arrays in the layouts above in, host arrays out, the same kernels; they return when the results are in the
 * caller's buffers.  pgx_vocab_train answers N < V with PGX_E_BADARG at once.  scores may be NULL. */
int pgx_vocab_train(pgx_ctx *ctx, const uint32_t *desc, const int32_t *counts, int F, int stride, int V, int iters,
                    uint64_t seed, uint32_t *vocab, int32_t *report);
int pgx_select_pairs(pgx_ctx *ctx, const uint32_t *desc, const int32_t *counts, int F, int stride, const uint32_t *vocab,
                     int V, int weighting, int top_k, int window, int min_score, int max_pairs, int32_t *pairlist,
                     int32_t *pair_score, int32_t *scores, int32_t *summary);

/* ---- dense depth maps by census plane sweep, and a cross-view filter ------------------ */
/* The sparse stages end with one point per track.  These three calls make a surface-dense cloud from the same frames and the
 * cameras those stages estimated: grey images, one depth map per reference frame, and the pixels that other maps confirm as a
 * point list.  Integer rules wherever a rule can be an integer, float64 in a stated order elsewhere (the library is built
 * without contraction): bit-identical to a numpy restatement (tests/depth_ref.py).  Not in the C# reference.  k_depth.hip.
 *
 * pgx_gray_batch_dev: d_gray [F][H][W] float32 = the grey image of every frame of d_rgba [F][H][W] (the context's source
 * format), gathered through the context's dewarp map when one is set (then W x H must be the map's: PGX_E_DIM_MISMATCH).
 * Per frame the bits of pgx_gray (of pgx_gray on pgx_dewarp's output, with a map).  Asynchronous. */
int pgx_gray_batch_dev(pgx_ctx *ctx, const uint16_t *d_rgba, int F, int W, int H, float *d_gray /* [F][H][W] */);
/* pgx_depth_maps_dev.  Frames, slots, d_frame_ids and d_P as for pgx_triangulate_tracks_dev: d_gray holds F SLOTS, slot s shows
 * frame d_frame_ids[s] (NULL: identity, n_frames = F; of two slots naming one frame the lower is used), d_P [n_frames][12] by
 * frame NUMBER, u = column, v = row; M = P[:, 0:3], p4 = P[:, 3], m3 = M's third row, adj(M) the adjugate (cofactors
 * transposed, each cofactor a b - c d), det M = (m00 adj00 + m01 adj10) + m02 adj20.  A camera is UNKNOWN if an entry is not
 * finite or det M == 0.  Row r of d_views [R][1 + S] names the reference frame, then S source frames; -1 = no source there.
 * d_range [R][2] = (z_near, z_far).  Everything is read on the device: the call can follow pgx_bundle_adjust_dev's P_out on the
 * same stream.  a . b + c . d + e . f below always means (a b + c d) + e f.
 *   1 census  per slot and pixel, the 9 wide x 7 high window in raster order without the centre: bit t (t = 0 .. 61) =
 *             g(neighbour) < g(centre) in float32 (a NaN on either side gives 0), neighbour coordinates clamped to the image.
 *   2 planes  for k < D: iz_k = 1/z_far + (k / (D - 1)) (1/z_near - 1/z_far); w_k = (sign(det M_r) ||m3_r||) (1 / iz_k), with
 *             ||m3|| = sqrt(m20^2 + m21^2 + m22^2).  A reference with an unknown camera, a range that is not 0 < z_near < z_far
 *             finite, or a frame that no slot shows is flagged NOCAMERA at every pixel.
 *   3 warp    per (r, s): A_ij = (M_s[i] . adj(M_r)[:, j]) / det M_r, b_i = p4_s[i] - (A[i] . p4_r).  A source that is -1, has an
 *             unknown camera or no slot is invalid everywhere.
 *   4 cost    of reference pixel (u, v), plane k, source s: y_i = (A_i0 u + A_i1 v) + A_i2, q_i = w_k y_i + b_i.  The source is
 *             valid iff q_2 > 0 and 0 <= q_0 / q_2 + 0.5 < W and 0 <= q_1 / q_2 + 0.5 < H (IEEE float64, correctly rounded
 *             division; NaN fails); the source pixel is the floor of those two values.  cost = popcount(census_r(u, v) xor
 *             census_s(pixel)) where valid, 31 where not.  raw(u, v, k) = the sum over the S sources, nvalid(u, v, k) = the
 *             number of valid ones.  A consequence, here and in pgx_depth_fuse_dev: a source with det M_s < 0 (-P for a
 *             camera P) has q_2 < 0 at every point in front of it, so q_2 > 0 passes over it there as over a source that is
 *             -1 (its warp is finite all the same), while as a reference such a camera is as good as P (w_k < 0).
 *   5 box     agg(u, v, k) = the sum of raw over the (2 agg_radius + 1)^2 box, box coordinates clamped to the image.
 *   6 choice  k* = the argmin of agg over k, ties to the smallest k.  Flags (PGX_DEP_*, bits): NOCAMERA (step 2); NOVIEWS
 *             nvalid(u, v, k*) < min_views; EDGE k* is 0 or D - 1; HIGHCOST agg(k*) > max_cost.
 *   7 sub-plane position, in integers: n = agg(k* - 1) - agg(k* + 1), den = agg(k* - 1) - 2 agg(k*) + agg(k* + 1) >= 0;
 *             off = 0 if den == 0, else sign(n) ((|n| 128) / den) truncated (|off| <= 128); kq8 = 256 k* + off;
 *             depth = 1 / (1/z_far + ((kq8 / 256.0) / (D - 1)) (1/z_near - 1/z_far)).  With any flag set kq8 = -1, depth = NaN.
 * Outputs: d_kq8, d_flags int32 and d_depth float64 [R][H][W]; d_cost [R][H][W] int32 or NULL = agg(k*), written unless
 * NOCAMERA; d_warp [R][S][12] float64 or NULL = A row-major then b (NaN for an invalid source); d_planes [R][D] float64 or
 * NULL = w_k (NaN for a NOCAMERA reference); d_summary [8] int32: pixels processed, pixels with flags 0, pixels carrying
 * NOCAMERA, NOVIEWS, EDGE, HIGHCOST, reference maps with NOCAMERA, 0.
 * Returned at once (PGX_E_BADARG): D outside [3, 256], S outside [1, 8], agg_radius outside [0, 3], min_views outside [1, S],
 * max_cost < 0, R outside [1, 65535], F outside [1, 65535], W or H outside [1, 65535], max(F, R) W H > 2^30, n_frames != F
 * without d_frame_ids, null required pointers.  Workspace: 8 bytes per pixel and slot.
 * Results depend on the inputs only: the same bits from run to run, for any slot layout of the same frames, and from the host
 * form.  Asynchronous on the context's stream. */
#define PGX_DEP_NOCAMERA 1
#define PGX_DEP_NOVIEWS  2
#define PGX_DEP_EDGE     4
#define PGX_DEP_HIGHCOST 8
int pgx_depth_maps_dev(pgx_ctx *ctx, const float *d_gray /* [F][H][W] */, int F, int W, int H,
                       const int32_t *d_frame_ids /* [F] or NULL */, int n_frames, const double *d_P /* [n_frames][12] */,
                       const int32_t *d_views /* [R][1 + S] */, int R, int S, const double *d_range /* [R][2] = (z_near, z_far) */,
                       int D, int agg_radius, int min_views, int max_cost,
                       int32_t *d_kq8 /* [R][H][W] */, double *d_depth /* [R][H][W] */, int32_t *d_cost /* [R][H][W] or NULL */,
                       int32_t *d_flags /* [R][H][W] */, double *d_warp /* [R][S][12] or NULL */, double *d_planes /* [R][D] or NULL */,
                       int32_t *d_summary /* [8] */);
/* pgx_depth_fuse_dev: the pixels of the maps that other maps of the same call confirm, as a point list.  d_depth, d_views as
 * above (the frames of d_views are frame NUMBERS into d_P; no slots here: map r is row r).  A map whose reference frame is
 * outside [0, n_frames) or has an unknown camera is skipped.  For pixel (u, v) of map r with finite depth z:
 *   w = (sign(det M_r) ||m3_r||) z; t = (w u - p4_r[0], w v - p4_r[1], w - p4_r[2]); X_i = (adj(M_r)[i] . t) / det M_r.
 *   For each source j of r's row, in the row's order, that is the reference of a row of this call with a known camera (the
 *   first such row; -1 and other frames are passed over; a frame named twice counts twice; r's own frame counts if it is
 *   named): q_i = (P_j[i][0:3] . X) + P_j[i][3]; pixel validity and the nearest pixel as in rule 4 above;
 *   d = (sign(det M_j) q_2) / ||m3_j||; z_j = the depth of map j at that pixel; the view agrees iff z_j is finite and
 *   |d - z_j| <= rel_tol z_j.
 *   agree = the number of agreeing views; the pixel is kept iff agree >= min_agree.
 * The kept pixels in (r, v, u) order: d_xyz [max_points][3] float64 = X, d_src [max_points][2] int32 = (r, v W + u).  More than
 * max_points kept: the first max_points are written and pgx_check_status reports PGX_E_CAPACITY.  d_agree [R][H][W] int32 or
 * NULL = agree, -1 for a pixel without a depth or of a skipped map.  d_summary [4] int32: pixels kept (the full count), pixels
 * with a depth, those of them with at least one source of the kind above that they project into validly, maps skipped.
 * Returned at once (PGX_E_BADARG): S outside [1, 8], R outside [1, 65535], R W H > 2^30, rel_tol negative or not finite,
 * min_agree or max_points < 0, null required pointers (d_xyz and d_src may be NULL with max_points == 0).
 * The same bit-identity properties as the depth maps.  Asynchronous on the context's stream. */
int pgx_depth_fuse_dev(pgx_ctx *ctx, const double *d_depth /* [R][H][W] */, const int32_t *d_views /* [R][1 + S] */, int R, int S,
                       int W, int H, int n_frames, const double *d_P, double rel_tol, int min_agree, int max_points,
                       double *d_xyz /* [max_points][3] */, int32_t *d_src /* [max_points][2] = (r, v * W + u) */,
                       int32_t *d_agree /* [R][H][W] or NULL */, int32_t *d_summary /* [4] */);
/* Host forms: host arrays in the layouts above, the same kernels; they return when the results are in the caller's buffers.
 * gray [n_frames][H][W] by frame number (no slots).  cost, warp, planes and agree may be NULL.  R == 0: the summary is zeroed and
 * nothing else is written.  pgx_depth_fuse writes min(summary[0], max_points) rows of xyz and src. */
int pgx_depth_maps(pgx_ctx *ctx, const float *gray, int n_frames, int W, int H, const double *P, const int32_t *views, int R, int S,
                   const double *range, int D, int agg_radius, int min_views, int max_cost, int32_t *kq8, double *depth,
                   int32_t *cost, int32_t *flags, double *warp, double *planes, int32_t *summary);
int pgx_depth_fuse(pgx_ctx *ctx, const double *depth, const int32_t *views, int R, int S, int W, int H, int n_frames,
                   const double *P, double rel_tol, int min_agree, int max_points, double *xyz, int32_t *src, int32_t *agree,
                   int32_t *summary);

/* ---- the plan of the dense stage from the sparse model: sources and depth range per reference -------- */
/* pgx_depth_maps_dev takes d_views and d_range from the caller.  This call derives both from the track graph, the track points
 * and the cameras, on the device, so that tracks -> (consensus) -> triangulate -> bundle-adjust -> triangulate -> this ->
 * pgx_gray_batch_dev -> pgx_depth_maps_dev -> pgx_depth_fuse_dev runs on one stream with no host round trip.  View selection by
 * shared points at a usable triangulation angle and a depth range from the depths of the sparse points, as multi-view stereo
 * packages do both; stated so that it is bit-identical to a numpy restatement (tests/dense_views_ref.py).  Not in the C#
 * reference.  k_denseviews.hip.
 * Inputs.  d_offsets, d_nodes, d_track_summary and max_tracks as for pgx_triangulate_tracks_dev; n_tracks = d_track_summary[0] is
 * read on the device.  max_nodes = the entries of d_nodes that an offset may reach (n_frames * stride for a graph of
 * pgx_tracks_dev or pgx_track_consensus_dev).  d_xyz [max_tracks][3] and d_track_flags [max_tracks] or NULL as for
 * pgx_bundle_adjust_dev.  d_P [n_frames][12] by frame NUMBER.  d_refs [R] frame numbers, or NULL: reference r is frame r, and R must
 * be n_frames.  Only the frame of a node is read: the call takes no keypoints and no slots.
 * Values.  Every value is a double, every operation one IEEE double operation in the order written, nothing is contracted into
 * a fused multiply-add; a dot product x . y is ((x0 y0 + x1 y1) + x2 y2).
 * Frames.  A frame is KNOWN by the triangulation's test (all 12 entries finite and det M != 0).  Per known frame Minv,
 * C = -(Minv p4) and sgn are exactly pgx_track_consensus_dev's; nrm = sqrt((m20 m20 + m21 m21) + m22 m22).
 * Used tracks.  Track t is used iff t < min(n_tracks, max_tracks), d_track_flags[t] == 0 (or the pointer is NULL) and X = d_xyz[t]
 * has three finite components.  Nothing else of an unused track is read.
 * Used nodes.  Node i of a used track, in frame f, is USED iff f is in [0, n_frames) and known, and
 *   z_i = (sgn_f ((P_f[2][0:3] . X) + P_f[2][3])) / nrm_f
 * satisfies z_i > 0 (NaN fails).  This is the triangulation's depth_i and the z of the depth maps.
 * Pairs.  For used nodes i < j (positions in d_nodes) of one track, in frames a and b: a pair with a == b is passed over.
 * Otherwise r_i = C_a - X, r_j = C_b - X (componentwise), d = r_i . r_j, na = r_i . r_i, nb = r_j . r_j; the pair counts 1 in
 * shared[a][b] and in shared[b][a], and 1 in good[a][b] and good[b][a] iff d > 0 and d d <= cmin2 (na nb) and
 * d d >= cmax2 (na nb): the angle at X between the two centres lies in [min_angle_deg, max_angle_deg].  cmin2 and cmax2 are the
 * squares of the host C library's cos(min_angle_deg * M_PI / 180.0) and cos(max_angle_deg * M_PI / 180.0), computed once.  No
 * division and no p4 beyond C: a translated scene decides the same way, and -P decides exactly as P.  A track that names a
 * frame twice counts each of its two nodes there against every other frame.  The counts are int32.
 * Sources of reference a (a known frame).  The candidates are the known frames b != a with shared[a][b] >= min_shared (with
 * min_shared = 0 every other known frame).  Ordered by good descending, then shared descending, then frame number ascending
 * (an integer key: the grid and the order of the sums cannot matter), the first S are the row's sources; missing ones are -1.
 * Range of reference a.  Z_a = the multiset of the z_i of the used nodes in frame a, n_a its size, z_(0) <= ... <= z_(n_a - 1)
 * its order.  In 64-bit integers i_near = ((n_a - 1) q_near_pm) / 1000 and i_far = ((n_a - 1) q_far_pm + 999) / 1000;
 * z_near = z_(i_near) / grow, z_far = z_(i_far) * grow: exact order statistics of the exact doubles (numpy.sort's), no
 * histogram approximation.  n_a < min_points: the range is (NaN, NaN), and pgx_depth_maps_dev flags that map NOCAMERA by its
 * rule 2.
 * Outputs, per row r of d_refs:
 *   d_views [R][1 + S] int32  the reference frame as given, then the sources
 *   d_range [R][2] float64    (z_near, z_far)
 *   d_pair_counts [R][n_frames][2] int32 or NULL  (shared[a][b], good[a][b]) for every frame b
 *   d_ref_stats [R][4] int32  n_a, the candidates, the sources chosen, PGX_DVW_* bits: FEWPOINTS n_a < min_points; FEWVIEWS
 *           fewer than S sources chosen; NARROW the range is finite but not z_near < z_far.  A reference that is outside
 *           [0, n_frames) or not known has -1 for every source, a NaN range, zero counts and NOCAMERA alone.
 *   d_report [8] int32: tracks processed, tracks used, nodes used, pairs counted (once each, whatever d_refs names), references
 *           with a finite range, references with S sources, references with at least one source, 0.
 * A frame named twice in d_refs gives two equal rows.
 * Errors through pgx_check_status: n_tracks > max_tracks (PGX_E_CAPACITY; the first max_tracks tracks are processed); a node
 * of a used track whose frame is outside [0, n_frames) (PGX_E_BADARG; the node is skipped); malformed offsets (o0 < 0,
 * o1 < o0 or o1 > max_nodes: PGX_E_BADARG, the track counts as empty, as in the triangulation).  Only where malformed offsets make
 * tracks overlap can there be more used nodes than max_nodes; the ranges are then unspecified (no access leaves the buffers).
 * Returned at once (PGX_E_BADARG), with nothing written: S outside [1, 8], R or n_frames outside [1, 65535],
 * R n_frames > 2^24, max_tracks or max_nodes < 0, angles that are not finite or not 0 <= min_angle_deg < max_angle_deg < 90,
 * min_shared < 0, min_points < 1, R != n_frames without d_refs, q_near_pm or q_far_pm outside [0, 1000] or q_near_pm > q_far_pm, grow not finite or < 1, null
 * required pointers, an output that overlaps an input.
 * Workspace: 8 bytes per cell of R x n_frames, 8 bytes per entry of max_nodes, 112 bytes per frame.
 * Results depend on the inputs only: the same bits from run to run, for any max_tracks >= n_tracks, on a used workspace and
 * from the host form below.  Asynchronous on the context's stream. */
#define PGX_DVW_NOCAMERA  1
#define PGX_DVW_FEWPOINTS 2
#define PGX_DVW_FEWVIEWS  4
#define PGX_DVW_NARROW    8
int pgx_dense_views_dev(pgx_ctx *ctx, const int32_t *d_offsets, const int32_t *d_nodes, const int32_t *d_track_summary,
                        int max_tracks, int max_nodes, const double *d_xyz, const int32_t *d_track_flags, int n_frames,
                        const double *d_P, const int32_t *d_refs /* [R] or NULL */, int R, int S, double min_angle_deg,
                        double max_angle_deg, int min_shared, int min_points, int q_near_pm, int q_far_pm, double grow,
                        int32_t *d_views /* [R][1 + S] */, double *d_range /* [R][2] */,
                        int32_t *d_pair_counts /* [R][n_frames][2] or NULL */, int32_t *d_ref_stats /* [R][4] */,
                        int32_t *d_report /* [8] */);
/* Host form: host arrays in the layouts above, the same kernels (tracks as pgx_tracks_get writes them; offsets that are not
 * non-decreasing from 0, or a node whose frame is outside [0, n_frames): PGX_E_BADARG before any GPU work).  nodes
 * [n_nodes][2]; xyz [n_tracks][3]; track_flags [n_tracks] or NULL; refs [R] or NULL (then R = n_frames);
 * pair_counts and ref_stats may be NULL.  R == 0: the report is zeroed and nothing else is written.  Returns when the
 * outputs are in the caller's buffers. */
int pgx_dense_views(pgx_ctx *ctx, const int32_t *track_offsets, const int32_t *nodes, int n_tracks, const double *xyz,
                    const int32_t *track_flags, int n_frames, const double *P, const int32_t *refs, int R, int S,
                    double min_angle_deg, double max_angle_deg, int min_shared, int min_points, int q_near_pm, int q_far_pm,
                    double grow, int32_t *views, double *range, int32_t *pair_counts, int32_t *ref_stats, int32_t *report);

/* ---- the fused points merged into one cloud, with normals and colour ------------------------------ */
/* pgx_depth_fuse_dev ends with one list entry per kept pixel and map: a surface point seen by five references appears five
 * times, without a normal and without a colour.  These calls make the cloud a user writes to a file and meshes: one point per
 * occupied cell of a grid, its normal from the depth maps and its colour from the frames, on the same stream with no host
 * round trip.  Integers wherever a rule can be an integer (every sum is one, so no order of execution changes a bit), float64
 * elsewhere, one IEEE operation at a time in the order written, nothing contracted: bit-identical to a numpy restatement
 * (tests/cloud_ref.py).  Not in the C# reference.  k_image.hip, k_cloud.hip.
 *
 * pgx_rgba8_batch_dev: d_rgba8 [F][H][W] uint32 = per frame and pixel the pixel that pgx_dewarp writes (the context's source
 * format, gathered through the context's dewarp map when one is set: then W x H must be the map's, PGX_E_DIM_MISMATCH, and a map
 * entry outside the image gives the zero pixel and PGX_E_OOB_SOURCE from pgx_check_status), channel c in bits 8 c .. 8 c + 7 in the
 * source's channel order: the high byte of each 16-bit channel; an RGBA8 source's bytes as they are.  Asynchronous. */
int pgx_rgba8_batch_dev(pgx_ctx *ctx, const uint16_t *d_rgba, int F, int W, int H, uint32_t *d_rgba8 /* [F][H][W] */);
/* pgx_cloud_merge_dev.
 * Inputs.  d_xyz [max_in][3] float64 and d_src [max_in][2] int32 = (r, v W + u) as pgx_depth_fuse_dev writes them; any list in
 * that layout, in any order.  d_count int32 on the device or NULL (the filter's d_summary fits):
 * n = min(max(d_count[0], 0), max_in), or max_in with NULL; n is read on the device.  d_depth [R][H][W], d_views [R][1 + S] (only
 * column 0 is read), n_frames and d_P as for the filter.  d_rgba8 [F][H][W] (pgx_rgba8_batch_dev's) or NULL; F slots and
 * d_frame_ids [F] or NULL as for pgx_depth_maps_dev: the lowest slot that shows a frame is used.  F and d_frame_ids are not read
 * without d_rgba8.
 *   1 used    point i < n is USED iff its three coordinates are finite, r = src[i][0] is in [0, R), pix = src[i][1] is in
 *             [0, W H), and for every axis a, t_a = (X_a - o_a) / cell and g_a = floor(t_a) satisfy -2^20 <= g_a < 2^20
 *             (o = (ox, oy, oz)).  key = (g_0 + 2^20) << 42 | (g_1 + 2^20) << 21 | (g_2 + 2^20).  The position in the cell:
 *             p_a = (int) floor((t_a - g_a) 65536.0), 0 <= p_a <= 65535; the subtraction and the scaling are exact.
 *   2 normal  of a used point, from its own map alone.  (u, v) = (pix % W, pix / W), z = depth[r][v][u].  No normal when map r is
 *             skipped by the filter's rule (its frame outside [0, n_frames) or its camera unknown) or z is not finite.
 *             X_c = the filter's back-projection of (u, v, z).  A neighbour (u', v') COUNTS iff it is inside the image, its
 *             depth z' is finite and |z' - z| <= disc_tol z; its point is the same back-projection of (u', v', z').  Along u,
 *             with the neighbours at u +- k (k = normal_step): d_u = X+ - X- when both count, X+ - X_c when only the forward
 *             one does, X_c - X- when only the backward one does; no normal when neither counts.  d_v the same along v.
 *             n = d_u x d_v, each component a b - c d: n_0 = d_u1 d_v2 - d_u2 d_v1, n_1 = d_u2 d_v0 - d_u0 d_v2,
 *             n_2 = d_u0 d_v1 - d_u1 d_v0.  The ray: e_i = (adj(M_r)[i][0] u + adj(M_r)[i][1] v) + adj(M_r)[i][2];
 *             dX/dz = (sign(det) ||m3|| / det) e has the direction of e for either sign of det, so the normal faces the camera
 *             iff n . e < 0.  s = (n_0 e_0 + n_1 e_1) + n_2 e_2, L = sqrt((n_0 n_0 + n_1 n_1) + n_2 n_2).  No normal when L is not
 *             finite, L == 0, s is not finite or s == 0.  Otherwise m = (s > 0 ? -n : n) / L and
 *             q_a = (int) floor(m_a 32767.0 + 0.5).
 *   3 colour  of a used point: word pix of the slot that shows frame views[r][0], its low three bytes.  No colour when d_rgba8
 *             is NULL or no slot shows the frame.
 *   4 cells   per key, over its used points, in int64 or int32: cnt; the three sums sp of p; nn and the three sums sn of q over
 *             the points with a normal; nc and the three channel sums sc over the points with a colour; first = the smallest i.
 *   5 output  a cell is KEPT iff cnt >= min_support.  The kept cells in ascending first, the order of first appearance in the
 *             list:
 *             d_out_xyz [max_points][3] float64 = o_a + ((double) g_a + ((double)(2 sp_a + cnt) / (double)(2 cnt)) / 65536.0) cell:
 *               the mean of the points' positions to cell / 65536 (each point stands at the middle of its 1/65536 of the cell);
 *             d_out_normal [max_points][3] float32 = (float)(s_a / L), s_a = (double) sn_a, L = sqrt((s_0 s_0 + s_1 s_1) + s_2 s_2);
 *               zeros when nn == 0 or L == 0;
 *             d_out_rgba8 [max_points] uint32: channel c = (2 sc_c + nc) / (2 nc) in integers in bits 8 c .. 8 c + 7, alpha 255;
 *               0 when nc == 0;
 *             d_out_info [max_points][4] int32 = (cnt, nn, nc, first).
 * Optional: d_pt_normal [max_in][3] int32 = q, zeros for a point without a normal; d_cell_of [max_in] int32 = the output index
 * of the point's cell (the full index, also at or past max_points), -1 for a point that is not used, -2 for a point of a dropped
 * cell.  Rows i >= n of both are not written.
 * d_report [8] int32: n, used, not used, points with a normal, points with a colour, cells, cells kept (the full count), 0.
 * More than max_points cells kept: the first max_points are written and pgx_check_status reports PGX_E_CAPACITY.
 * Returned at once (PGX_E_BADARG), with nothing written: S outside [1, 8], R outside [1, 65535], W or H outside [1, 65535],
 * R W H > 2^30, n_frames < 1, max_in or max_points outside [0, 2^28]; with d_rgba8: F outside [1, 65535], F W H > 2^30, n_frames != F
 * without d_frame_ids; cell not finite or <= 0, an origin that is not finite, normal_step outside [1, 8], disc_tol not finite or
 * < 0, min_support < 1, null required pointers (d_xyz and d_src may be NULL with max_in == 0, the four outputs with
 * max_points == 0), an output that overlaps an input.
 * Workspace: 20 bytes per entry of a table of the power of two >= max(2 max_in, 256) entries, 20 bytes per entry of max_in,
 * 84 bytes per entry of max_points.
 * Results depend on the inputs only: the same bits from run to run, for any slot layout of the same frames, on a used
 * workspace and from the host form; a permuted list gives the same cells with the same sums, in the order of their new first.
 * Asynchronous on the context's stream. */
int pgx_cloud_merge_dev(pgx_ctx *ctx, const double *d_xyz /* [max_in][3] */, const int32_t *d_src /* [max_in][2] */,
                        const int32_t *d_count /* [1] or NULL */, int max_in, const double *d_depth /* [R][H][W] */,
                        const int32_t *d_views /* [R][1 + S] */, int R, int S, int W, int H, int n_frames, const double *d_P,
                        const uint32_t *d_rgba8 /* [F][H][W] or NULL */, int F, const int32_t *d_frame_ids /* [F] or NULL */,
                        double cell, double ox, double oy, double oz, int normal_step, double disc_tol, int min_support,
                        int max_points, double *d_out_xyz /* [max_points][3] */, float *d_out_normal /* [max_points][3] */,
                        uint32_t *d_out_rgba8 /* [max_points] */, int32_t *d_out_info /* [max_points][4] */,
                        int32_t *d_pt_normal /* [max_in][3] or NULL */, int32_t *d_cell_of /* [max_in] or NULL */,
                        int32_t *d_report /* [8] */);
/* Host forms: host arrays in the layouts above, the same kernels; they return when the results are in the caller's buffers.
 * pgx_rgba8_batch: rgba [F][H][W] in the context's source format.  pgx_cloud_merge: the list has n_in entries (no d_count);
 * rgba8 [n_frames][H][W] by frame number (no slots) or NULL; pt_normal and cell_of may be NULL; the report is downloaded first,
 * then min(report[6], max_points) rows of the four outputs. */
int pgx_rgba8_batch(pgx_ctx *ctx, const void *rgba, int F, int W, int H, uint32_t *rgba8);
int pgx_cloud_merge(pgx_ctx *ctx, const double *xyz, const int32_t *src, int n_in, const double *depth, const int32_t *views, int R,
                    int S, int W, int H, int n_frames, const double *P, const uint32_t *rgba8, double cell, double ox, double oy,
                    double oz, int normal_step, double disc_tol, int min_support, int max_points, double *out_xyz,
                    float *out_normal, uint32_t *out_rgba8, int32_t *out_info, int32_t *pt_normal, int32_t *cell_of,
                    int32_t *report);

/* ---- a triangle mesh from the depth maps: TSDF grid and surface nets -------------------------------- */
/* The cloud above is points with normals; these calls make the surface, on the same stream with no host round trip: a truncated
 * signed distance (TSDF) on the lattice nodes round the filter's points, in which the maps that see a node are averaged, and
 * naive surface nets: one vertex in every cube of eight nodes with a sign change, one quad on every lattice edge with a sign
 * change.  No case table.  Integers wherever a rule can be an integer (every sum over maps and nodes is one, so no order of
 * execution changes a bit), float64 elsewhere, one IEEE operation at a time in the order written, a dot product as
 * (a b + c d) + e f, nothing contracted: bit-identical to a numpy restatement (tests/mesh_ref.py).  Not in the C# reference.
 * k_mesh.hip.
 *
 * pgx_mesh_dev.
 * Inputs.  The list d_xyz, d_src, d_count, max_in, the maps d_depth, d_views (column 0 alone), n_frames, d_P and the colour
 * d_rgba8, F, d_frame_ids exactly as for pgx_cloud_merge_dev.  d_agree [R][H][W] int32 (pgx_depth_fuse_dev's optional output) or
 * NULL, with min_agree.  The grid cell, o = (ox, oy, oz).  band B in [1, 3], trunc_cells T in [1, 8]:
 * trunc = (double) T * cell.  min_weight >= 1.
 *   1 seeds     point i < n is USED by rule 1 of pgx_cloud_merge_dev (the same test, the same g and key) and, further,
 *               -2^20 + 4 <= g_a < 2^20 - 4 on every axis.
 *   2 voxels    a lattice node c (an integer triple) stands at X_a = o_a + (double) c_a * cell.  It is a VOXEL iff some used point
 *               has g_a - B + 1 <= c_a <= g_a + B on every axis (B = 1: the eight corners of the point's own cell).  With
 *               d = c - g + (B - 1): nb = (d_2 2B + d_1) 2B + d_0, and ord(c) = the minimum of 256 i + nb over all such
 *               (point, node) incidences, a 64-bit integer; it equals the minimum over the occupied cells of
 *               256 first(cell) + nb.
 *   3 TSDF      per voxel over the maps r = 0 .. R - 1; a map is skipped by the filter's rule (its frame outside [0, n_frames) or
 *               its camera unknown).  q = P_r (X, 1) row by row as ((p_0 X_0 + p_1 X_1) + p_2 X_2) + p_3; the projection is
 *               VALID iff q_2 > 0 and the nearest pixel (u, v) = ((int)(q_0 / q_2 + 0.5), (int)(q_1 / q_2 + 0.5)) is inside the
 *               image, as in the filter; d = (sign(det M_r) q_2) / ||m3_r||.  The observation COUNTS iff the projection is valid,
 *               z = depth[r][v][u] is finite, and d_agree is NULL or agree[r][v][u] >= min_agree.  s = z - d.  If s < -trunc (or s
 *               is NaN) the map is passed over: the voxel is hidden behind the surface.  t = s > trunc ? trunc : s,
 *               tq = (int) floor((t / trunc) * 32767.0 + 0.5); in integers w += 1, st += tq; if s <= trunc and a slot shows frame
 *               views[r][0] (the lowest, as in the cloud): nc += 1 and the three channel sums sc take the pixel's low three bytes.
 *               A voxel is VALID iff w >= min_weight, INSIDE iff it is valid and st < 0; phi = (double) st / (double) w.
 *   4 vertices  cube c has the nodes c + {0, 1}^3; node j has the offsets (j & 1, j >> 1 & 1, j >> 2 & 1) on axes 0, 1, 2.  It is
 *               COMPLETE iff all eight are valid voxels, ACTIVE iff complete and their INSIDE bits are not all equal.  Its twelve
 *               edges in the order axis a = 0, 1, 2 and, within an axis, the offsets 00, 10, 01, 11 on the two other axes, the
 *               lower axis first; lo is the end with offset 0 along a.  For each edge whose ends differ in INSIDE:
 *               tau = phi_lo / (phi_lo - phi_hi), and the crossing is lo's offsets with coordinate a replaced by tau.
 *               m_a = (0.0 plus the crossings' coordinate a, added in edge order) / (double) k, k the number of crossings.
 *               Position o_a + ((double) c_a + m_a) * cell.  Normal: G_a = 0.0 plus (phi_hi - phi_lo) of the four edges along a in
 *               edge order, L = sqrt((G_0 G_0 + G_1 G_1) + G_2 G_2), (float)(G_a / L), zeros when L is 0 or not finite; it points
 *               into free space, towards the cameras.  Colour: nc and sc summed over the eight nodes, the channel
 *               (2 sc + nc) / (2 nc) in integers, alpha 255; 0 when nc == 0.  Info (c_0, c_1, c_2, mask | k << 8), mask the eight
 *               INSIDE bits.  The vertices in ascending ord(c) of the cube's low node.
 *   5 triangles node c and axis a with c and c + e_a both valid and differing in INSIDE; b = (a + 1) % 3, c' = (a + 2) % 3; the
 *               cubes round the edge Q0 = c - e_b - e_c', Q1 = c - e_c', Q2 = c, Q3 = c - e_b.  A quad is emitted iff all four are
 *               complete (they are then active); with v0 .. v3 their vertex indices: (v0, v1, v2), (v0, v2, v3) when c is INSIDE,
 *               (v0, v2, v1), (v0, v3, v2) otherwise: the geometric normal faces free space.  The quads in ascending
 *               (ord(c), a), the two triangles of a quad adjacent.
 * Outputs.  d_out_xyz [max_vertices][3] float64, d_out_normal [max_vertices][3] float32, d_out_rgba8 [max_vertices] uint32,
 * d_out_info [max_vertices][4] int32, d_out_tri [max_tris][3] int32 (full vertex indices, also at or past max_vertices).
 * d_report [8] int32: n, used points, seed cells, voxels, valid voxels, vertices (the full count), triangles (the full count), 0.
 * More vertices or triangles than the capacity: the first ones are written and pgx_check_status reports PGX_E_CAPACITY.  More
 * voxels than max_voxels: PGX_E_CAPACITY, report[5] and report[6] are 0, report[3] > max_voxels (the entries of the table in use:
 * the voxel count unless the table is full), no vertex or triangle is written, and no probe runs for more than one round of the
 * table.
 * Returned at once (PGX_E_BADARG), with nothing written: the refusals of pgx_cloud_merge_dev for the arguments the calls share,
 * band outside [1, 3], trunc_cells outside [1, 8], min_weight < 1, min_agree < 0, max_voxels, max_vertices or max_tris outside
 * [0, 2^28], null required pointers (the four vertex outputs may be NULL with max_vertices == 0, d_out_tri with max_tris == 0), an
 * output that overlaps an input.
 * Workspace: 58 bytes per entry of a table of the power of two >= max(2 max_voxels, 256) entries, 4 bytes per entry of the list
 * and 16 bytes per block of 256 of them; nothing per vertex or triangle.
 * Results depend on the inputs only: the same bits from run to run, for any slot layout of the same frames, on a used
 * workspace and from the host form; a permuted list gives the same vertices and triangles up to renumbering.
 * Asynchronous on the context's stream. */
int pgx_mesh_dev(pgx_ctx *ctx, const double *d_xyz /* [max_in][3] */, const int32_t *d_src /* [max_in][2] */,
                 const int32_t *d_count /* [1] or NULL */, int max_in, const double *d_depth /* [R][H][W] */,
                 const int32_t *d_views /* [R][1 + S] */, int R, int S, int W, int H, int n_frames, const double *d_P,
                 const int32_t *d_agree /* [R][H][W] or NULL */, int min_agree, const uint32_t *d_rgba8 /* [F][H][W] or NULL */,
                 int F, const int32_t *d_frame_ids /* [F] or NULL */, double cell, double ox, double oy, double oz, int band,
                 int trunc_cells, int min_weight, int max_voxels, int max_vertices, int max_tris,
                 double *d_out_xyz /* [max_vertices][3] */, float *d_out_normal /* [max_vertices][3] */,
                 uint32_t *d_out_rgba8 /* [max_vertices] */, int32_t *d_out_info /* [max_vertices][4] */,
                 int32_t *d_out_tri /* [max_tris][3] */, int32_t *d_report /* [8] */);
/* Host form: host arrays in the layouts above, the same kernels; it returns when the results are in the caller's buffers.  The
 * list has n_in entries (no d_count); agree may be NULL; rgba8 [n_frames][H][W] by frame number (no slots) or NULL; the report
 * is downloaded first, then min(report[5], max_vertices) rows of the four vertex outputs and min(report[6], max_tris) triangles. */
int pgx_mesh(pgx_ctx *ctx, const double *xyz, const int32_t *src, int n_in, const double *depth, const int32_t *views, int R, int S,
             int W, int H, int n_frames, const double *P, const int32_t *agree, int min_agree, const uint32_t *rgba8, double cell,
             double ox, double oy, double oz, int band, int trunc_cells, int min_weight, int max_voxels, int max_vertices,
             int max_tris, double *out_xyz, float *out_normal, uint32_t *out_rgba8, int32_t *out_info, int32_t *out_tri,
             int32_t *report);

/* ---- the mesh cleaned: small components dropped, smoothed, normals again ---------------------------- */
/* The mesh above is as rough as its maps and carries a closed blob for every wrong pixel that survived the filter.  These calls
 * finish it where it lies, on the same stream with no host round trip: the connected components with few triangles are dropped,
 * the rest is smoothed without shrinking (Taubin's lambda | mu on fixed-point positions) and takes its normals from the smoothed
 * triangles.  Integers wherever a sum is taken (so no order of execution changes a bit; int64 arithmetic wraps in two's
 * complement), float64 elsewhere, one IEEE operation at a time in the order written, nothing contracted: bit-identical to a numpy
 * restatement (tests/mesh_clean_ref.py).  Not in the C# reference.  k_meshclean.hip.
 *
 * pgx_mesh_clean_dev.
 * Inputs.  The outputs of pgx_mesh_dev, read where they lie: d_xyz [max_vertices][3] float64, d_normal [max_vertices][3] float32,
 * d_rgba8 [max_vertices] uint32, d_info [max_vertices][4] int32, d_tri [max_tris][3] int32; any mesh in that layout.  d_counts int32
 * [8] on the device or NULL (pgx_mesh_dev's d_report fits): nv = min(max(d_counts[5], 0), max_vertices),
 * nt = min(max(d_counts[6], 0), max_tris), or the capacities with NULL; both are read on the device.  The grid of the fixed-point
 * positions: cell, o = (ox, oy, oz), normally the mesh's.  min_tris >= 1, min_frac_pm in [0, 1000], iters in [0, 64], lambda in
 * (0, 1], mu in [-1.5, 0].
 *   1 valid, used  vertex v < nv is VALID iff its three coordinates are finite and t_a = (X_a - o_a) / cell satisfies
 *               -2^20 <= t_a < 2^20 on every axis; its fixed-point position is q_a = (int64) floor(t_a * 65536.0 + 0.5).  Triangle
 *               k < nt is USED iff its three indices are in [0, nv), pairwise distinct, and its three vertices are valid (this
 *               disposes of the indices at or past max_vertices that pgx_mesh_dev writes after a capacity overflow).
 *   2 components   two vertices are connected when a used triangle holds both; a component is named by its smallest vertex.
 *               cnt(C) = its used triangles, big = the largest cnt (0 without a used triangle).  A component is KEPT iff
 *               cnt >= min_tris and 1000 cnt >= min_frac_pm big, in int64.  A vertex in no used triangle is dropped.  A vertex
 *               is KEPT iff it is in a used triangle and its component is kept, a triangle iff it is used and its component is
 *               kept.
 *   3 smoothing    only with iters > 0: iters times the half-step with f = lambda, then (unless mu == 0) the half-step with f = mu.
 *               A half-step, for every kept vertex v with d kept triangles that hold it, from the values before the half-step
 *               (Jacobi): D_a = the int64 sum over those triangles of (q_a[o1] - q_a[v]) + (q_a[o2] - q_a[v]), o1 and o2 the
 *               triangle's two other vertices (an edge shared by two triangles counts twice, a boundary edge once: this is the
 *               rule);  r = floor((f * (double) D_a) / (double)(2 d) + 0.5), the conversion of D_a rounding to nearest, r clamped
 *               to [-2^62, 2^62];  q'_a = q_a + (int64) r.
 *   4 normals      only with iters > 0, on the final q.  Per kept triangle (a, b, c): e1 = (double)(q[b] - q[a]),
 *               e2 = (double)(q[c] - q[a]) per axis (the differences in int64); n = e1 x e2, each component x y - z w as in rule 2
 *               of pgx_cloud_merge_dev: n_0 = e1_1 e2_2 - e1_2 e2_1, n_1 = e1_2 e2_0 - e1_0 e2_2, n_2 = e1_0 e2_1 - e1_1 e2_0;
 *               L = sqrt((n_0 n_0 + n_1 n_1) + n_2 n_2).  The triangle contributes nothing when L is 0 or not finite; otherwise
 *               m_a = (int) floor((n_a / L) * 32767.0 + 0.5).  Per kept vertex s_a = the int64 sum of m_a over the kept triangles
 *               that hold it, x_a = (double) s_a, L' = sqrt((x_0 x_0 + x_1 x_1) + x_2 x_2); the normal is (float)(x_a / L'), zeros
 *               when L' is 0.  pgx_mesh_dev's winding faces free space, so these normals do.
 *   5 output       the kept vertices in ascending old index, the kept triangles in ascending old index with their vertices' new
 *               indices in the old order (the winding stays).  iters == 0: xyz and normal are copied bit for bit; otherwise
 *               xyz_a = o_a + ((double) q_a / 65536.0) * cell and the normal of rule 4.  rgba8 and info are always copied.
 * Outputs.  d_out_xyz [max_out_vertices][3] float64, d_out_normal [max_out_vertices][3] float32, d_out_rgba8 [max_out_vertices]
 * uint32, d_out_info [max_out_vertices][4] int32, d_out_tri [max_out_tris][3] int32 (full new indices, also at or past
 * max_out_vertices).  Optional: d_vertex_map [max_vertices] int32 = the new index (the full one), -1 for a vertex that is not
 * valid or in no used triangle, -2 for one of a dropped component; d_comp [max_vertices] int32 = the name of the vertex's
 * component, -1 where vertex_map is -1.  Rows >= nv of both are not written.
 * d_report [8] int32: nv, nt, used triangles, components, components kept, vertices out (the full count), triangles out (the
 * full count), big.  More vertices or triangles kept than the capacity: the first ones are written and pgx_check_status reports
 * PGX_E_CAPACITY.
 * Returned at once (PGX_E_BADARG), with nothing written: max_vertices, max_tris, max_out_vertices or max_out_tris outside
 * [0, 2^28], cell not finite or <= 0, an origin that is not finite, min_tris < 1, min_frac_pm outside [0, 1000], iters outside
 * [0, 64], lambda not finite or outside (0, 1], mu not finite or outside [-1.5, 0], null required pointers (the four vertex inputs
 * may be NULL with max_vertices == 0, d_tri with max_tris == 0, the four vertex outputs with max_out_vertices == 0, d_out_tri with
 * max_out_tris == 0), an output that overlaps an input.
 * Workspace: 81 bytes per entry of max_vertices, 25 bytes per entry of max_tris, 32 bytes per block of 256 entries of the
 * larger of the two; sized and carved before any launch.
 * Results depend on the inputs only: the same bits from run to run, on a used workspace and from the host form; a permuted
 * triangle list gives the same vertices, and the same triangles in the new order.
 * Asynchronous on the context's stream. */
int pgx_mesh_clean_dev(pgx_ctx *ctx, const double *d_xyz /* [max_vertices][3] */, const float *d_normal /* [max_vertices][3] */,
                       const uint32_t *d_rgba8 /* [max_vertices] */, const int32_t *d_info /* [max_vertices][4] */,
                       const int32_t *d_tri /* [max_tris][3] */, const int32_t *d_counts /* [8] or NULL */, int max_vertices,
                       int max_tris, double cell, double ox, double oy, double oz, int min_tris, int min_frac_pm, int iters,
                       double lambda, double mu, int max_out_vertices, int max_out_tris,
                       double *d_out_xyz /* [max_out_vertices][3] */, float *d_out_normal /* [max_out_vertices][3] */,
                       uint32_t *d_out_rgba8 /* [max_out_vertices] */, int32_t *d_out_info /* [max_out_vertices][4] */,
                       int32_t *d_out_tri /* [max_out_tris][3] */, int32_t *d_vertex_map /* [max_vertices] or NULL */,
                       int32_t *d_comp /* [max_vertices] or NULL */, int32_t *d_report /* [8] */);
/* Host form: host arrays in the layouts above, the same kernels; it returns when the results are in the caller's buffers.  The
 * mesh has n_vertices vertices and n_tris triangles (no d_counts); vertex_map and comp may be NULL; the report is downloaded
 * first, then min(report[5], max_out_vertices) rows of the four vertex outputs and min(report[6], max_out_tris) triangles. */
int pgx_mesh_clean(pgx_ctx *ctx, const double *xyz, const float *normal, const uint32_t *rgba8, const int32_t *info,
                   const int32_t *tri, int n_vertices, int n_tris, double cell, double ox, double oy, double oz, int min_tris,
                   int min_frac_pm, int iters, double lambda, double mu, int max_out_vertices, int max_out_tris, double *out_xyz,
                   float *out_normal, uint32_t *out_rgba8, int32_t *out_info, int32_t *out_tri, int32_t *vertex_map, int32_t *comp,
                   int32_t *report);

/* ---- the mesh decimated: adaptive vertex clustering over grid blocks ------------------------------- */
/* Surface nets gives one vertex per active cube: a flat wall costs as many triangles per square metre as a corner.  These calls
 * merge the vertices of a grid block of 2^l cells into one where the triangle normals round the block agree, up to level lmax, and
 * keep them apart where they do not; on the same stream, reading the previous stage's report on the device.  Integers wherever a
 * sum is taken (no order of execution changes a bit; int64 arithmetic wraps in two's complement), float64 elsewhere, one IEEE
 * operation at a time in the order written, nothing contracted: bit-identical to a numpy restatement
 * (tests/mesh_decimate_ref.py).  Not in the C# reference.  k_meshdecimate.hip.
 *
 * pgx_mesh_decimate_dev.
 * Inputs.  A mesh in pgx_mesh_dev's layout, read where it lies: d_xyz, d_normal, d_rgba8, d_info, d_tri with the capacities
 * max_vertices and max_tris (d_normal and d_info belong to the layout and are not read).  d_counts int32 [8] on the device or NULL:
 * nv = min(max(d_counts[5], 0), max_vertices), nt = min(max(d_counts[6], 0), max_tris), or the capacities with NULL; the reports
 * of pgx_mesh_dev, pgx_mesh_clean_dev and of this call fit.  The grid: cell, o = (ox, oy, oz).  lmin in [0, 6], lmax in [lmin, 6],
 * flat_q in [0, 1024].
 *   1 valid, used, q   rule 1 of pgx_mesh_clean_dev: vertex v < nv is VALID iff its coordinates are finite and
 *               t_a = (X_a - o_a) / cell satisfies -2^20 <= t_a < 2^20; q_a = min((int64) floor(t_a * 65536.0 + 0.5), 2^36 - 1) (the
 *               clamp is this stage's: t just below 2^20 rounds to 2^36, one past the last cell; the clamp keeps every q in a
 *               cell of the grid).  Triangle k < nt is USED iff its indices are in [0, nv), pairwise distinct, and its vertices
 *               valid.  A vertex is a MEMBER iff it is in a used triangle.
 *   2 triangle normals   per used triangle (a, b, c): e1, e2, n and L as in rule 4 of pgx_mesh_clean_dev, on q;
 *               m_a = (int64) floor((n_a / L) * 1024.0 + 0.5), m = 0 when L is 0 or not finite.
 *   3 blocks, flat   the block of vertex v at level l is B_a = q_a >> (16 + l), the shift arithmetic (the floor): a side of 2^l cells.
 *               For every level l in lmin + 1 .. lmax and every block: N = the number of incidences (triangle, corner) of used
 *               triangles whose corner vertex lies in the block, S_a = the int64 sum of those triangles' m_a (a triangle with
 *               three corners in the block counts three times), S2 = (S_0 S_0 + S_1 S_1) + S_2 S_2 in int64.  The block is FLAT
 *               iff (double) S2 >= (double)(flat_q * flat_q) * ((double) N * (double) N).  With flat_q = 1024 a block whose
 *               normals are all exactly one axis passes at equality; with flat_q = 0 every block passes.
 *   4 level     L(v) of a member = the largest l in lmin .. lmax such that v's blocks at every level lmin + 1 .. l are flat
 *               (lmin when there is none or lmax == lmin).  The cluster of a member is the pair (L(v), block of v at L(v)): a
 *               partition of the members.
 *   5 clusters  a cluster is named by its smallest member; clusters are ordered by name.  Over its n members, each once, with
 *               org_a = B_a << (16 + L): s_a = sum (q_a - org_a), Q_a = org_a + (2 s_a + n) / (2 n) (integers; s_a >= 0), and per
 *               byte of rgba8 the sum sc and the byte (2 sc + n) / (2 n).  Q lies in the cluster's block.
 *   6 triangles a used triangle maps to its three clusters and is DEGENERATE unless they are pairwise distinct.  Otherwise it is
 *               rotated so that the cluster of the smallest name comes first (the winding stays).  Triangles with the same rotated
 *               triple are duplicates: the one of the smallest old index is KEPT.  The same clusters in the opposite winding are
 *               another triangle.  The kept triangles are written in ascending old index as the rotated triples of new indices.
 *   7 output    the output vertices are the clusters that occur in a kept triangle, in order of name.
 *               xyz_a = o_a + ((double) Q_a / 65536.0) * cell; rgba8 of rule 5; info = (name, L, n, 0).  The normal is rule 4 of
 *               pgx_mesh_clean_dev on the kept triangles and the Q values (m in 1/32767, zeros when the sum is zero).  A kept
 *               triangle is FLIPPED iff the integer dot product of its m in 1/32767 (zeros when L is 0 or not finite) with the m of
 *               rule 2 of the same triangle is negative.
 * Outputs.  d_out_xyz, d_out_normal, d_out_rgba8, d_out_info [max_out_vertices] and d_out_tri [max_out_tris][3] (full new
 * indices, also at or past max_out_vertices).  Optional: d_vertex_map [max_vertices] int32 = the new index of the vertex's cluster
 * (the full one), -1 for a vertex that is no member, -2 for a member whose cluster is in no kept triangle; d_level [max_vertices]
 * int32 = L(v), -1 for a vertex that is no member.  Rows >= nv of both are not written.
 * d_report [8] int32: nv, nt, used triangles, clusters, duplicates dropped, vertices out, triangles out (the full counts),
 * flipped (among all kept triangles); used = degenerate + duplicates + triangles out.  More vertices or triangles than the
 * capacity: the first ones are written and pgx_check_status reports PGX_E_CAPACITY.
 * Returned at once (PGX_E_BADARG), with nothing written: max_vertices, max_tris, max_out_vertices or max_out_tris outside
 * [0, 2^28], cell not finite or <= 0, an origin that is not finite, lmin outside [0, 6], lmax outside [lmin, 6], flat_q outside
 * [0, 1024], null required pointers (the four vertex inputs may be NULL with max_vertices == 0, d_tri with max_tris == 0, the four
 * vertex outputs with max_out_vertices == 0, d_out_tri with max_out_tris == 0), an output that overlaps an input.
 * Workspace: 30 bytes per entry of max_vertices, 28 per entry of max_tris, 157 per entry of the vertex tables (the power of two
 * >= 2 max_vertices, at least 512), 4 per entry of the triangle table (likewise of max_tris), 16 per block of 256 entries; sized and
 * carved before any launch: 1.3 GB for 2.8 M vertices and 4.6 M triangles, 84 GB at max_vertices = 2^28.  A workspace that cannot be
 * allocated returns PGX_E_HIP with nothing launched: the practical limit is the device's free memory over 350 to 660 bytes a vertex.
 * Results depend on the inputs only: the same bits from run to run, on a used workspace and from the host form; a permuted
 * triangle list gives the same vertices bit for bit and the same set of triangle rows.
 * Asynchronous on the context's stream. */
int pgx_mesh_decimate_dev(pgx_ctx *ctx, const double *d_xyz /* [max_vertices][3] */, const float *d_normal /* [max_vertices][3] */,
                          const uint32_t *d_rgba8 /* [max_vertices] */, const int32_t *d_info /* [max_vertices][4] */,
                          const int32_t *d_tri /* [max_tris][3] */, const int32_t *d_counts /* [8] or NULL */, int max_vertices,
                          int max_tris, double cell, double ox, double oy, double oz, int lmin, int lmax, int flat_q,
                          int max_out_vertices, int max_out_tris, double *d_out_xyz /* [max_out_vertices][3] */,
                          float *d_out_normal /* [max_out_vertices][3] */, uint32_t *d_out_rgba8 /* [max_out_vertices] */,
                          int32_t *d_out_info /* [max_out_vertices][4] */, int32_t *d_out_tri /* [max_out_tris][3] */,
                          int32_t *d_vertex_map /* [max_vertices] or NULL */, int32_t *d_level /* [max_vertices] or NULL */,
                          int32_t *d_report /* [8] */);
/* Host form: host arrays in the layouts above, the same kernels; it returns when the results are in the caller's buffers.  The
 * mesh has n_vertices vertices and n_tris triangles (no d_counts); vertex_map and level may be NULL; the report is downloaded
 * first, then min(report[5], max_out_vertices) rows of the four vertex outputs and min(report[6], max_out_tris) triangles. */
int pgx_mesh_decimate(pgx_ctx *ctx, const double *xyz, const float *normal, const uint32_t *rgba8, const int32_t *info,
                      const int32_t *tri, int n_vertices, int n_tris, double cell, double ox, double oy, double oz, int lmin, int lmax,
                      int flat_q, int max_out_vertices, int max_out_tris, double *out_xyz, float *out_normal, uint32_t *out_rgba8,
                      int32_t *out_info, int32_t *out_tri, int32_t *vertex_map, int32_t *level, int32_t *report);

/* ---- measurement hooks (bench.py) ---------------------------------------------------- */
/* When on, the named hot kernels are bracketed by HIP events on the launch stream. */
int pgx_profile_enable(pgx_ctx *ctx, int on);
/* Bracket only the kernel group `name` (NULL or "": every group again).  Two event records per launch cost about 10 us
 * of device time each way on a busy stream (0.6 ms per step of the bench job with every launch bracketed): the timed
 * region of bench.py brackets the dominant kernel only, the untimed stand-alone pass brackets everything. */
int pgx_profile_filter(pgx_ctx *ctx, const char *name);
/* Sums since the last reset for kernel `name` ("dewarp_gray", "fast", "pyramid", "pyramid_append", "ham_argmin", ...):
 * launches and total milliseconds.  Synchronises the stream. */
int pgx_profile_get(pgx_ctx *ctx, const char *name, int *launches, double *total_ms);
int pgx_profile_reset(pgx_ctx *ctx);
/* When on, a multi-chunk pgx_match_batch_dev runs its stages in order on the context's stream instead of side by side on
 * the library's own streams: the event times above are then stand-alone kernel times (side by side they overlap and
 * stretch each other). */
int pgx_profile_serialize(pgx_ctx *ctx, int on);
/* Counters of the last pgx_match* call: rounds run on the all-CU distance kernel, and the
 * descriptor-pair distance evaluations those launches issued (sum over rounds and image pairs of
 * n1*n2; evaluations_round0 = the first launch alone = sum of N1*N2).  Synchronises the stream. */
int pgx_match_stats(pgx_ctx *ctx, int *rounds_wide, int64_t *evaluations, int64_t *evaluations_round0);

/* Diagnostic counters of the match tail since the last call, 64-bit (they count per image pair and step: a long run
 * overflows 32 bits): [3] queue entries, [4] matrix-row scans, [6] proposals of the per-pair finish; the others are
 * used by developer builds only.  Cleared on read.  Synchronises the stream. */
int pgx_debug_counters(pgx_ctx *ctx, int64_t *out8);

/* ---- host-side helpers (no GPU work) -------------------------------------------------- */
/* Utils.NextGaussianPair (Utils.cs:14-38) on a seeded splitmix64 stream; out [P][4]. */
int pgx_make_brief_pairs(uint64_t seed, int sigma, int P, int32_t *out);
/* The steering table of a pair table (steered BRIEF above; not in the C# reference): pairs_rot_out [B][P][4], dirs_out [B][2].
 * For k < B / 4, theta = 2 pi k / B in double: dirs[k] = (rint(16384 cos theta), rint(16384 sin theta)), and every end point
 * (dx, dy) becomes (rint(c dx - s dy), rint(s dx + c dy)), in image coordinates (x right, y down).  For k >= B / 4 the
 * entries are the EXACT quarter turn (x, y) -> (-y, x) of direction k - B / 4, both end points and dirs; no libm is used
 * again.  The quarter-turn relation is what makes the 90-degree invariance exact.  Direction 0 is the input table.  Input
 * offsets beyond +-2^20, B outside {4, 8, ..., 64}: PGX_E_BADARG. */
int pgx_make_steering(const int32_t *pairs, int P, int B, int32_t *pairs_rot_out, int32_t *dirs_out);
/* DeWarp.GetDistortionMatrix (DeWarp.cs:39-107) in float64 on the host; out [H][W][2].
 * MathNet's Cubic.RealRoots is restated from its published algorithm (parity unpinned). */
int pgx_build_dewarp_map(int W, int H, const double *coeffs, int ncoeffs, int32_t *out);

#ifdef __cplusplus
}
#endif
#endif /* PGX_H */
