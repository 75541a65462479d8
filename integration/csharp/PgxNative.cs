// PgxNative.cs -- P/Invoke surface of libpgx.so (include/pgx.h), to be added to
// dotnet_src/ImageProcessing.  NOT compiled in this repository (no .NET SDK in the build image);
// it is the literal binding a maintainer adds.  See INTEGRATION.md.
using System;
using System.Runtime.InteropServices;

namespace ImageProcessing.Native;

[StructLayout(LayoutKind.Sequential)]
public struct PgxKeypoint { public int X, Y, FastScore; public float Value; }

[StructLayout(LayoutKind.Sequential)]
public struct PgxPair { public int K1, K2, Dist; }

internal static unsafe class PgxNative
{
    private const string Lib = "pgx"; // libpgx.so next to the executable or on LD_LIBRARY_PATH

    public const int Ok = 0, EDimMismatch = 1, EOobSource = 2, EEmptySet = 3, ECapacity = 4, EBadArg = 5, EHip = 6,
        ENotConfigured = 7, ERccl = 8;   // include/pgx.h: PGX_OK, PGX_E_*
    public const int DistNone = int.MaxValue;                                             // PGX_DIST_NONE
    public const int SrcRgba64 = 0, SrcRgba8 = 1;                                         // PGX_SRC_*
    public const int StageDetect = 0, StageMatchWide = 1, StageMatchRows = 2, StageMatchDone = 3;   // PGX_STAGE_*
    public const int CommIdBytes = 128;                                                   // PGX_COMM_ID_BYTES
    public const int TriFewViews = 1, TriDegenerate = 2, TriBehind = 4, TriParallax = 8, TriReproj = 16;   // PGX_TRI_* (0 = valid)
    public const int RegBadK = 1, RegFewPoints = 2, RegNoSolution = 4, RegFewInliers = 8;   // PGX_REG_* (0 = registered)
    public const int CnsFewViews = 1, CnsLowParallax = 2, CnsNoConsensus = 4, CnsShort = 8;   // PGX_CNS_* (0 = a consensus, kept)
    public const int VerFewMatches = 1, VerNoModel = 2, VerFewInliers = 4;                 // PGX_VER_* (0 = accepted)
    public const int DepNoCamera = 1, DepNoViews = 2, DepEdge = 4, DepHighCost = 8;       // PGX_DEP_* (0 = a depth)
    public const int DvwNoCamera = 1, DvwFewPoints = 2, DvwFewViews = 4, DvwNarrow = 8;   // PGX_DVW_* (0 = S sources and a range)
    public const int InitSkipped = 1, InitBadInput = 2, InitDegenerate = 4, InitFewFront = 8, InitFewPoints = 16;   // PGX_INIT_* (0 = eligible)

    // Exports of include/pgx.h that this binding deliberately leaves out (tests/test_csharp_binding.py holds the list to the
    // header): the caller's-HIP-stream hook and the measurement hooks (a managed host owns no hipStream_t and reads no HIP event
    // times), the version string, the communicator query, and the two host-side helpers whose managed originals the host
    // keeps (Utils.NextGaussianPair, DeWarp.GetDistortionMatrix).
    // OMITTED: pgx_version pgx_set_stream pgx_comm_info pgx_profile_enable pgx_profile_filter pgx_profile_get pgx_profile_reset
    // OMITTED: pgx_profile_serialize pgx_match_stats pgx_debug_counters pgx_make_brief_pairs pgx_build_dewarp_map

    [DllImport(Lib)] public static extern int pgx_ctx_create(int device, out IntPtr ctx);
    [DllImport(Lib)] public static extern void pgx_ctx_destroy(IntPtr ctx);
    [DllImport(Lib)] public static extern IntPtr pgx_last_error(IntPtr ctx);
    [DllImport(Lib)] public static extern int pgx_set_dewarp_map(IntPtr ctx, int* uv, int w, int h);
    [DllImport(Lib)] public static extern int pgx_set_dewarp_coeffs(IntPtr ctx, int w, int h, double* coeffs, int ncoeffs);
    [DllImport(Lib)] public static extern int pgx_get_dewarp_map(IntPtr ctx, int* uvOut, int w, int h);
    [DllImport(Lib)] public static extern int pgx_set_brief_pairs(IntPtr ctx, int* pairs, int p);
    // steered BRIEF (not in the reference): pairsRot [b][p][4] and dirs [b][2] from pgx_make_steering; pairsRot = null turns it off
    [DllImport(Lib)] public static extern int pgx_set_brief_steering(IntPtr ctx, int* pairsRot, int* dirs, int b, int radius);
    [DllImport(Lib)] public static extern int pgx_make_steering(int* pairs, int p, int b, int* pairsRotOut, int* dirsOut);
    // scale pyramid (not in the reference): nLevels in [1, 8] (1 = off), stepQ16 in [69632, 131072]; rules in include/pgx.h
    [DllImport(Lib)] public static extern int pgx_set_pyramid(IntPtr ctx, int nLevels, int stepQ16);
    [DllImport(Lib)] public static extern int pgx_pyramid_level(IntPtr ctx, float* gray, int w, int h, int level, float* levelOut);
    [DllImport(Lib)] public static extern int pgx_pyramid_dims(int w, int h, int nLevels, int stepQ16, int* dimsOut, int* scaleOut);
    [DllImport(Lib)] public static extern int pgx_set_detect_params(IntPtr ctx, float threshold, int suppressionRadius);
    [DllImport(Lib)] public static extern int pgx_set_capacity(IntPtr ctx, int maxRaw, int maxKeypoints);
    [DllImport(Lib)] public static extern int pgx_set_source_format(IntPtr ctx, int format); // 0 = Rgba64, 1 = Rgba32 bytes (widened x257 on the device)
    [DllImport(Lib)] public static extern int pgx_set_match_chunk(IntPtr ctx, int imagePairsPerChunk);
    [DllImport(Lib)] public static extern int pgx_gate_match(IntPtr ctx, IntPtr other, int stage);  // the same wait inside the next matcher call, behind its init kernel
    [DllImport(Lib)] public static extern int pgx_wait_stage(IntPtr ctx, IntPtr other, int stage);   // PGX_STAGE_*: 0 detect, 1 match wide, 2 match rows, 3 match done
    [DllImport(Lib)] public static extern int pgx_dewarp(IntPtr ctx, ushort* rgba64, int w, int h, ushort* outRgba64);
    [DllImport(Lib)] public static extern int pgx_gray(IntPtr ctx, ushort* rgba64, int w, int h, float* outGray);
    [DllImport(Lib)] public static extern int pgx_fast(IntPtr ctx, float* gray, int w, int h, PgxKeypoint* o, int capacity, out int n);
    [DllImport(Lib)] public static extern int pgx_brief(IntPtr ctx, float* gray, int w, int h, PgxKeypoint* kps, int n, uint* desc);
    [DllImport(Lib)] public static extern int pgx_orient(IntPtr ctx, float* gray, int w, int h, PgxKeypoint* kps, int n, int* bins);
    [DllImport(Lib)] public static extern int pgx_nms(IntPtr ctx, PgxKeypoint* kps, int n, int w, int h, int* order, out int nOut);
    [DllImport(Lib)] public static extern int pgx_match(IntPtr ctx, uint* d1, int n1, uint* d2, int n2, int words, PgxPair* o);
    // many image pairs, managed arrays, one call: descs[f] -> frame f's descriptors, pairList [m][2], lists back to back in `o`
    [DllImport(Lib)] public static extern int pgx_match_batch(IntPtr ctx, uint** descs, int* counts, int nFrames, int words,
                                                              int* pairList, int nPairs, PgxPair* o, long* outOffsets);
    [DllImport(Lib)] public static extern int pgx_detect(IntPtr ctx, ushort* rgba64, int w, int h, PgxKeypoint* kp, uint* desc,
                                                         int capacity, out int n, out int nRaw);
    // exact nearest neighbours of one pair (not KeypointMatching: see INTEGRATION.md); idx, dist [n1][k], colNn [n2] or null
    [DllImport(Lib)] public static extern int pgx_knn(IntPtr ctx, uint* d1, int n1, uint* d2, int n2, int words, int k, int* idx,
                                                      int* dist, int* colNn);
    // epipolar-guided nearest neighbours of one pair: f [9] row-major (h1^T F h2 = 0), band in pixels; outputs as pgx_knn
    [DllImport(Lib)] public static extern int pgx_knn_guided(IntPtr ctx, uint* d1, PgxKeypoint* kp1, int n1, uint* d2, PgxKeypoint* kp2,
                                                             int n2, int words, float* f, float band, int k, int* idx, int* dist,
                                                             int* colNn);

    // batched, device-resident entry points and the multi-GPU / pose / track-graph additions (include/pgx.h)
    [DllImport(Lib)] public static extern int pgx_detect_batch_dev(IntPtr ctx, void* dRgba64, int f, int w, int h, void* dKp, void* dDesc,
                                                                   void* dCounts, void* dNraw, int capacity);
    [DllImport(Lib)] public static extern int pgx_detect_batch_steered_dev(IntPtr ctx, void* dRgba64, int f, int w, int h, void* dKp,
                                                                           void* dDesc, void* dCounts, void* dNraw, int capacity,
                                                                           void* dBins);
    // pyramid mode: dOrigin [f][capacity][3] = (level, x_l, y_l), dLevelStats [f][nLevels][2]; dBins may be null
    [DllImport(Lib)] public static extern int pgx_detect_batch_pyramid_dev(IntPtr ctx, void* dRgba64, int f, int w, int h, void* dKp,
                                                                           void* dDesc, void* dCounts, void* dNraw, int capacity,
                                                                           void* dOrigin, void* dLevelStats, void* dBins);
    [DllImport(Lib)] public static extern int pgx_match_batch_dev(IntPtr ctx, void* dDesc, void* dCounts, int stride, int words,
                                                                  void* dPairlist, int m, int maxCount, void* dOut);
    [DllImport(Lib)] public static extern int pgx_knn_batch_dev(IntPtr ctx, void* dDesc, void* dCounts, int stride, int words,
                                                                void* dPairlist, int m, int maxCount, int k, void* dIdx, void* dDist,
                                                                void* dColNn);
    [DllImport(Lib)] public static extern int pgx_match_nn_batch_dev(IntPtr ctx, void* dDesc, void* dCounts, int stride, int words,
                                                                     void* dPairlist, int m, int maxCount, int maxDist, float ratio,
                                                                     int crossCheck, void* dOut);
    [DllImport(Lib)] public static extern int pgx_knn_guided_batch_dev(IntPtr ctx, void* dDesc, void* dKp, void* dCounts, int stride,
                                                                       int words, void* dPairlist, int m, int maxCount, void* dF,
                                                                       float band, int k, void* dIdx, void* dDist, void* dColNn);
    [DllImport(Lib)] public static extern int pgx_match_guided_batch_dev(IntPtr ctx, void* dDesc, void* dKp, void* dCounts, int stride,
                                                                         int words, void* dPairlist, int m, int maxCount, void* dF,
                                                                         float band, int maxDist, float ratio, int crossCheck,
                                                                         void* dOut);
    [DllImport(Lib)] public static extern int pgx_check_status(IntPtr ctx);
    [DllImport(Lib)] public static extern int pgx_comm_unique_id(byte* id128);
    [DllImport(Lib)] public static extern int pgx_comm_init(IntPtr ctx, int rank, int world, byte* id128);
    [DllImport(Lib)] public static extern int pgx_comm_destroy(IntPtr ctx);
    [DllImport(Lib)] public static extern int pgx_allgather_dev(IntPtr ctx, void* dBuf, nuint bytesPerRank);
    [DllImport(Lib)] public static extern int pgx_sequence_step_dev(IntPtr ctx, void* dFramesLocal, int nLocalFrames, int frameSlots, int w, int h,
                                                                    void* dKpLocal, void* dDescAll, void* dCountsAll, void* dNrawLocal, int capacity,
                                                                    void* dPairlistLocal, int nLocalPairs, int pairSlots, void* dOutAll);
    [DllImport(Lib)] public static extern int pgx_fundamental_ransac_dev(IntPtr ctx, void* dKp, void* dMatches, void* dCounts, void* dPairlist, int m,
                                                                         int stride, int nSamples, int pairsPerSample, float threshold, int rankCheck,
                                                                         ulong seed, float* dF, int* dInliers, int* dBestSample);
    [DllImport(Lib)] public static extern int pgx_pose_dev(IntPtr ctx, void* dKp, void* dMatches, void* dCounts, void* dPairlist, int m, int stride,
                                                           float* dF, float* dRt, int* dVotes, int* dBest, float* dPoints);
    [DllImport(Lib)] public static extern int pgx_tracks_create(int* counts, int nFrames, out IntPtr tracks);
    [DllImport(Lib)] public static extern void pgx_tracks_destroy(IntPtr tracks);
    [DllImport(Lib)] public static extern int pgx_tracks_add_pair(IntPtr tracks, int frameA, int frameB, PgxPair* matches, int n, int maxDist);
    [DllImport(Lib)] public static extern int pgx_tracks_finish(IntPtr tracks, int minLen, out int nTracks, out int nNodes);
    [DllImport(Lib)] public static extern int pgx_tracks_get(IntPtr tracks, int* trackOffsets, int* nodes);
    [DllImport(Lib)] public static extern int pgx_tracks_dropped(IntPtr tracks, out int nComponents, out int nNodes);
    // the same graph built on the device over the lists where the matcher / the all-gather left them
    [DllImport(Lib)] public static extern int pgx_tracks_dev(IntPtr ctx, void* dMatches, void* dCounts, void* dPairlist, int m, int f, int stride,
                                                             void* dFrameIds, int nFrames, int maxDist, int minLen, void* dTrackOf,
                                                             void* dOffsets, void* dNodes, void* dSummary);
    // split mode: components inconsistent at maxDist are split at the tighter gates (host array, strictly decreasing) instead of
    // dropped; dSummary [16], [8 + l] = nodes in tracks of level l
    [DllImport(Lib)] public static extern int pgx_tracks_split_dev(IntPtr ctx, void* dMatches, void* dCounts, void* dPairlist, int m, int f,
                                                                   int stride, void* dFrameIds, int nFrames, int maxDist, int* gates,
                                                                   int nGates, int minLen, void* dTrackOf, void* dOffsets, void* dNodes,
                                                                   void* dSummary);
    [DllImport(Lib)] public static extern int pgx_tracks_finish_split(IntPtr tracks, int* gates, int nGates, int minLen, out int nTracks,
                                                                      out int nNodes, int* summary);
    // one 3D point per track from the caller's cameras (p [nFrames][12] float64, row-major 3x4, NaN rows = no pose yet): the device
    // form follows the graph on the same stream and reads nTracks from dTrackSummary[0]; the host form takes what pgx_tracks_get
    // wrote and every frame's keypoints one after another (kps), and returns when xyz, quality, flags, nodeErr and summary are filled
    [DllImport(Lib)] public static extern int pgx_triangulate_tracks_dev(IntPtr ctx, void* dKp, int f, int stride, void* dFrameIds, int nFrames,
                                                                         void* dP, void* dOffsets, void* dNodes, void* dTrackSummary,
                                                                         int maxTracks, double minParallaxDeg, double maxReprojPx,
                                                                         int refineIters, void* dXyz, void* dQuality, void* dFlags,
                                                                         void* dNodeErr, void* dSummary);
    [DllImport(Lib)] public static extern int pgx_triangulate_tracks(IntPtr ctx, PgxKeypoint* kps, int* counts, int nFrames, double* p,
                                                                     int* trackOffsets, int* nodes, int nTracks, double minParallaxDeg,
                                                                     double maxReprojPx, int refineIters, double* xyz, double* quality,
                                                                     int* flags, double* nodeErr, int* summary);
    // bundle adjustment of the free cameras (k [nFrames][4] fx fy cx cy, rt [nFrames][12] R row-major then t, float64) and the
    // points of the tracks: the device form follows the triangulation on the same stream and reads nTracks from
    // dTrackSummary[0]; the host form takes what pgx_tracks_get wrote and every frame's keypoints one after another (kps)
    [DllImport(Lib)] public static extern int pgx_bundle_adjust_dev(IntPtr ctx, void* dKp, int f, int stride, void* dFrameIds, int nFrames,
                                                                    void* dK, void* dRtIn, void* dFixed, void* dOffsets, void* dNodes,
                                                                    void* dTrackSummary, int maxTracks, void* dXyzIn, void* dTrackFlags,
                                                                    int maxIters, double huberPx, double lambda0, void* dRtOut,
                                                                    void* dPOut, void* dXyzOut, void* dNodeErr, void* dTrace,
                                                                    void* dReport);
    [DllImport(Lib)] public static extern int pgx_bundle_adjust(IntPtr ctx, PgxKeypoint* kps, int* counts, int nFrames, double* k,
                                                                double* rtIn, int* fixedFrames, int* trackOffsets, int* nodes,
                                                                int nTracks, double* xyzIn, int* trackFlags, int maxIters,
                                                                double huberPx, double lambda0, double* rtOut, double* pOut,
                                                                double* xyzOut, double* nodeErr, double* trace, int* report);
    // frame registration by P3P RANSAC against the track points (k [nFrames][4] fx fy cx cy, rt [nFrames][12] R row-major then
    // t, float64; frames with reg != 0 are placed): the device form reads nTracks from dTrackSummary[0]; the host form takes
    // what pgx_tracks_get wrote and every frame's keypoints one after another (kps)
    [DllImport(Lib)] public static extern int pgx_register_frames_dev(IntPtr ctx, void* dKp, int f, int stride, void* dFrameIds, int nFrames,
                                                                      void* dK, void* dRtIn, void* dRegister, void* dOffsets, void* dNodes,
                                                                      void* dTrackSummary, int maxTracks, void* dXyz, void* dTrackFlags,
                                                                      int nSamples, double inlierPx, int minInliers, int refineIters,
                                                                      ulong seed, void* dRtOut, void* dPOut, void* dFrameStats,
                                                                      void* dFrameErr, void* dNodeInlier, void* dReport);
    [DllImport(Lib)] public static extern int pgx_register_frames(IntPtr ctx, PgxKeypoint* kps, int* counts, int nFrames, double* k,
                                                                  double* rtIn, int* reg, int* trackOffsets, int* nodes, int nTracks,
                                                                  double* xyz, int* trackFlags, int nSamples, double inlierPx,
                                                                  int minInliers, int refineIters, ulong seed, double* rtOut,
                                                                  double* pOut, int* frameStats, double* frameErr, int* nodeInlier,
                                                                  int* report);
    // track consensus, between either graph call and the triangulation: per track a two-view RANSAC over its observations
    // (p [nFrames][12] float64) and the compacted graph without the observations its winner rejects (offsetsOut, nodesOut,
    // summaryOut in the graph's layout; they must not be the inputs), trackMap old -> new index, xyzOut and flagsOut by the new
    // index, trackStats [.][4] by the old index, report [8]; dTrackOf [nFrames][stride] or null is rewritten in place
    [DllImport(Lib)] public static extern int pgx_track_consensus_dev(IntPtr ctx, void* dKp, int f, int stride, void* dFrameIds, int nFrames,
                                                                      void* dP, void* dOffsets, void* dNodes, void* dTrackSummary,
                                                                      int maxTracks, double inlierPx, double minParallaxDeg,
                                                                      int minInliers, int minLen, int maxHyp, ulong seed,
                                                                      void* dOffsetsOut, void* dNodesOut, void* dSummaryOut,
                                                                      void* dTrackMap, void* dXyzOut, void* dFlagsOut,
                                                                      void* dTrackStats, void* dTrackOf, void* dReport);
    [DllImport(Lib)] public static extern int pgx_track_consensus(IntPtr ctx, PgxKeypoint* kps, int* counts, int nFrames, double* p,
                                                                  int* trackOffsets, int* nodes, int nTracks, double inlierPx,
                                                                  double minParallaxDeg, int minInliers, int minLen, int maxHyp,
                                                                  ulong seed, int* offsetsOut, int* nodesOut, int* summaryOut,
                                                                  int* trackMap, double* xyzOut, int* flagsOut, int* trackStats,
                                                                  int* report);

    // two-view verification of match lists by epipolar RANSAC, between a matcher and pgx_tracks_dev: dOut [m][stride] (may be
    // dMatches), dF [m][9] float64, dF32 [m][9] float32 or null (what pgx_match_guided_batch_dev takes), dStats [m][8],
    // dInlier [m][stride] or null, dSampleF [m][nSamples][9] and dSampleCount [m][nSamples] or null, dReport [8]; the host form
    // runs one pair (matches, output and inlier hold n1 entries)
    [DllImport(Lib)] public static extern int pgx_verify_pairs_dev(IntPtr ctx, void* dKp, void* dMatches, void* dCounts, void* dPairlist,
                                                                   int m, int stride, int maxDist, int nSamples, double inlierPx,
                                                                   int minInliers, int refitIters, ulong seed, void* dOut, void* dF,
                                                                   void* dF32, void* dStats, void* dInlier, void* dSampleF,
                                                                   void* dSampleCount, void* dReport);
    [DllImport(Lib)] public static extern int pgx_verify_pair(IntPtr ctx, PgxKeypoint* kp1, int n1, PgxKeypoint* kp2, int n2,
                                                              PgxPair* matches, int maxDist, int nSamples, double inlierPx,
                                                              int minInliers, int refitIters, ulong seed, PgxPair* output, double* f,
                                                              int* stats, int* inlier);

    // the start of a reconstruction, between pgx_tracks_dev and the first pgx_triangulate_tracks_dev: per image pair the
    // relative pose from verification's dF [m][9] and dK [nFrames][4] (dRtPair [m][12], dPairStats [m][8], dSigma [m] or null,
    // dCandRt [m][4][12] or null), and for the chosen pair dRtOut, dPOut [nFrames][12], dFixedOut and dRegisterOut [nFrames]
    // as the next stages take them, dReport [8]; the host form runs one pair (f [9], kA and kB [4], rt [12], stats [8],
    // sigma [1], candRt [48] or null)
    [DllImport(Lib)] public static extern int pgx_init_pair_dev(IntPtr ctx, void* dKp, void* dMatches, void* dCounts, void* dPairlist,
                                                                int m, int f, int stride, void* dFrameIds, int nFrames, int maxDist,
                                                                void* dF, void* dK, double minAngleDeg, double minFrontFrac,
                                                                int minPoints, void* dRtPair, void* dPairStats, void* dSigma,
                                                                void* dCandRt, void* dRtOut, void* dPOut, void* dFixedOut,
                                                                void* dRegisterOut, void* dReport);
    [DllImport(Lib)] public static extern int pgx_relative_pose(IntPtr ctx, PgxKeypoint* kp1, int n1, PgxKeypoint* kp2, int n2,
                                                                PgxPair* matches, int maxDist, double* f, double* kA, double* kB,
                                                                double minAngleDeg, double minFrontFrac, int minPoints, double* rt,
                                                                int* stats, double* sigma, double* candRt);

    // image-pair selection on a binary visual vocabulary (256-bit descriptors): dDesc [f][stride][8], dVocab [v][8]; dWord and
    // dWdist [f][stride] (dWdist or null); dPairlist [maxPairs][2] is what every dPairlist parameter above takes, dPairScore
    // [maxPairs], dScores [f][f] or null, dSummary [8], dReport [4].  The host forms take host arrays in the same layouts.
    [DllImport(Lib)] public static extern int pgx_vocab_quantize_dev(IntPtr ctx, void* dDesc, void* dCounts, int f, int stride,
                                                                     void* dVocab, int v, void* dWord, void* dWdist);
    [DllImport(Lib)] public static extern int pgx_vocab_train_dev(IntPtr ctx, void* dDesc, void* dCounts, int f, int stride, int v,
                                                                  int iters, ulong seed, void* dVocab, void* dReport);
    [DllImport(Lib)] public static extern int pgx_select_pairs_dev(IntPtr ctx, void* dDesc, void* dCounts, int f, int stride,
                                                                   void* dVocab, int v, int weighting, int topK, int window,
                                                                   int minScore, int maxPairs, void* dPairlist, void* dPairScore,
                                                                   void* dScores, void* dSummary);
    [DllImport(Lib)] public static extern int pgx_vocab_train(IntPtr ctx, uint* desc, int* counts, int f, int stride, int v, int iters,
                                                              ulong seed, uint* vocab, int* report);
    [DllImport(Lib)] public static extern int pgx_select_pairs(IntPtr ctx, uint* desc, int* counts, int f, int stride, uint* vocab,
                                                               int v, int weighting, int topK, int window, int minScore,
                                                               int maxPairs, int* pairlist, int* pairScore, int* scores,
                                                               int* summary);

    // dense depth maps by census plane sweep and the cross-view filter (not in the reference): dGray [f][h][w] float32 by slot,
    // dP [nFrames][12] float64, dViews [r][1 + s] (reference frame, then sources; -1 = none), dRange [r][2] = (zNear, zFar);
    // dKq8, dFlags, dCost (or null) [r][h][w] int32, dDepth [r][h][w] float64, dWarp [r][s][12] and dPlanes [r][d] or null,
    // dSummary [8]; the filter writes dXyz [maxPoints][3], dSrc [maxPoints][2] = (r, v w + u), dAgree [r][h][w] or null,
    // dSummary [4].  The host forms take host arrays in the same layouts (gray [nFrames][h][w] by frame number).
    [DllImport(Lib)] public static extern int pgx_gray_batch_dev(IntPtr ctx, void* dRgba, int f, int w, int h, void* dGray);
    [DllImport(Lib)] public static extern int pgx_depth_maps_dev(IntPtr ctx, void* dGray, int f, int w, int h, void* dFrameIds, int nFrames,
                                                                 void* dP, void* dViews, int r, int s, void* dRange, int d,
                                                                 int aggRadius, int minViews, int maxCost, void* dKq8, void* dDepth,
                                                                 void* dCost, void* dFlags, void* dWarp, void* dPlanes, void* dSummary);
    [DllImport(Lib)] public static extern int pgx_depth_fuse_dev(IntPtr ctx, void* dDepth, void* dViews, int r, int s, int w, int h,
                                                                 int nFrames, void* dP, double relTol, int minAgree, int maxPoints,
                                                                 void* dXyz, void* dSrc, void* dAgree, void* dSummary);
    [DllImport(Lib)] public static extern int pgx_depth_maps(IntPtr ctx, float* gray, int nFrames, int w, int h, double* p, int* views,
                                                             int r, int s, double* range, int d, int aggRadius, int minViews,
                                                             int maxCost, int* kq8, double* depth, int* cost, int* flags, double* warp,
                                                             double* planes, int* summary);
    [DllImport(Lib)] public static extern int pgx_depth_fuse(IntPtr ctx, double* depth, int* views, int r, int s, int w, int h,
                                                             int nFrames, double* p, double relTol, int minAgree, int maxPoints,
                                                             double* xyz, int* src, int* agree, int* summary);

    // the plan of the dense stage from the sparse model, between the last triangulation and pgx_depth_maps_dev: per reference
    // (dRefs [r] frame numbers, or null: every frame, r = nFrames) dViews [r][1 + s] and dRange [r][2] as pgx_depth_maps_dev
    // takes them, dPairCounts [r][nFrames][2] or null = (shared, good), dRefStats [r][4], dReport [8]; the graph is dOffsets,
    // dNodes [maxNodes][2], dTrackSummary, the points dXyz [maxTracks][3] with dTrackFlags or null.  The host form takes host
    // arrays in the same layouts (pairCounts and refStats may be null)
    [DllImport(Lib)] public static extern int pgx_dense_views_dev(IntPtr ctx, void* dOffsets, void* dNodes, void* dTrackSummary,
                                                                  int maxTracks, int maxNodes, void* dXyz, void* dTrackFlags,
                                                                  int nFrames, void* dP, void* dRefs, int r, int s,
                                                                  double minAngleDeg, double maxAngleDeg, int minShared,
                                                                  int minPoints, int qNearPm, int qFarPm, double grow, void* dViews,
                                                                  void* dRange, void* dPairCounts, void* dRefStats, void* dReport);
    [DllImport(Lib)] public static extern int pgx_dense_views(IntPtr ctx, int* trackOffsets, int* nodes, int nTracks, double* xyz,
                                                              int* trackFlags, int nFrames, double* p, int* refs, int r, int s,
                                                              double minAngleDeg, double maxAngleDeg, int minShared, int minPoints,
                                                              int qNearPm, int qFarPm, double grow, int* views, double* range,
                                                              int* pairCounts, int* refStats, int* report);

    // the fused points merged into one cloud with normals and colour (not in the reference): dRgba8 [f][h][w] uint32 = the dewarped
    // pixel at 8 bits a channel; the merge takes the filter's dXyz [maxIn][3], dSrc [maxIn][2] and dCount (the filter's dSummary,
    // or null: maxIn entries), the maps and cameras as the filter does, dRgba8 by slot with dFrameIds or null, and writes one point
    // per occupied cell of the grid: dOutXyz [maxPoints][3] float64, dOutNormal [maxPoints][3] float32, dOutRgba8 [maxPoints],
    // dOutInfo [maxPoints][4] = (cnt, nn, nc, first), dPtNormal [maxIn][3] and dCellOf [maxIn] or null, dReport [8].  The host
    // forms take host arrays in the same layouts (rgba8 [nFrames][h][w] by frame number)
    [DllImport(Lib)] public static extern int pgx_rgba8_batch_dev(IntPtr ctx, void* dRgba, int f, int w, int h, void* dRgba8);
    [DllImport(Lib)] public static extern int pgx_cloud_merge_dev(IntPtr ctx, void* dXyz, void* dSrc, void* dCount, int maxIn,
                                                                  void* dDepth, void* dViews, int r, int s, int w, int h,
                                                                  int nFrames, void* dP, void* dRgba8, int f, void* dFrameIds,
                                                                  double cell, double ox, double oy, double oz, int normalStep,
                                                                  double discTol, int minSupport, int maxPoints, void* dOutXyz,
                                                                  void* dOutNormal, void* dOutRgba8, void* dOutInfo,
                                                                  void* dPtNormal, void* dCellOf, void* dReport);
    [DllImport(Lib)] public static extern int pgx_rgba8_batch(IntPtr ctx, void* rgba, int f, int w, int h, uint* rgba8);
    [DllImport(Lib)] public static extern int pgx_cloud_merge(IntPtr ctx, double* xyz, int* src, int nIn, double* depth, int* views,
                                                              int r, int s, int w, int h, int nFrames, double* p, uint* rgba8,
                                                              double cell, double ox, double oy, double oz, int normalStep,
                                                              double discTol, int minSupport, int maxPoints, double* outXyz,
                                                              float* outNormal, uint* outRgba8, int* outInfo, int* ptNormal,
                                                              int* cellOf, int* report);

    // a triangle mesh from the depth maps (a TSDF on a hashed grid, then surface nets; not in the managed implementation): the
    // list, maps, cameras and colours as for pgx_cloud_merge_dev, dAgree [r][h][w] (pgx_depth_fuse_dev's) or null -> dOutXyz
    // [maxVertices][3] float64, dOutNormal [maxVertices][3] float32, dOutRgba8 [maxVertices], dOutInfo [maxVertices][4],
    // dOutTri [maxTris][3] int32, dReport [8] ([5] vertices, [6] triangles).  The host form takes host arrays in the same layouts
    [DllImport(Lib)] public static extern int pgx_mesh_dev(IntPtr ctx, void* dXyz, void* dSrc, void* dCount, int maxIn, void* dDepth,
                                                           void* dViews, int r, int s, int w, int h, int nFrames, void* dP,
                                                           void* dAgree, int minAgree, void* dRgba8, int f, void* dFrameIds,
                                                           double cell, double ox, double oy, double oz, int band, int truncCells,
                                                           int minWeight, int maxVoxels, int maxVertices, int maxTris, void* dOutXyz,
                                                           void* dOutNormal, void* dOutRgba8, void* dOutInfo, void* dOutTri,
                                                           void* dReport);
    [DllImport(Lib)] public static extern int pgx_mesh(IntPtr ctx, double* xyz, int* src, int nIn, double* depth, int* views, int r,
                                                       int s, int w, int h, int nFrames, double* p, int* agree, int minAgree,
                                                       uint* rgba8, double cell, double ox, double oy, double oz, int band,
                                                       int truncCells, int minWeight, int maxVoxels, int maxVertices, int maxTris,
                                                       double* outXyz, float* outNormal, uint* outRgba8, int* outInfo, int* outTri,
                                                       int* report);

    // the mesh cleaned where it lies (not in the managed implementation): the outputs of pgx_mesh_dev and, as dCounts, its report
    // (or null: the capacities) -> the components with fewer than minTris triangles or fewer than minFracPm / 1000 of the
    // largest one's dropped, iters Taubin steps (lambda, mu), normals from the smoothed triangles: dOutXyz .. dOutTri as the
    // mesh's, dVertexMap [maxVertices] and dComp [maxVertices] int32 or null, dReport [8] ([5] vertices, [6] triangles out).
    // The host form takes host arrays in the same layouts
    [DllImport(Lib)] public static extern int pgx_mesh_clean_dev(IntPtr ctx, void* dXyz, void* dNormal, void* dRgba8, void* dInfo,
                                                                 void* dTri, void* dCounts, int maxVertices, int maxTris, double cell,
                                                                 double ox, double oy, double oz, int minTris, int minFracPm,
                                                                 int iters, double lambda, double mu, int maxOutVertices,
                                                                 int maxOutTris, void* dOutXyz, void* dOutNormal, void* dOutRgba8,
                                                                 void* dOutInfo, void* dOutTri, void* dVertexMap, void* dComp,
                                                                 void* dReport);
    [DllImport(Lib)] public static extern int pgx_mesh_clean(IntPtr ctx, double* xyz, float* normal, uint* rgba8, int* info, int* tri,
                                                             int nVertices, int nTris, double cell, double ox, double oy, double oz,
                                                             int minTris, int minFracPm, int iters, double lambda, double mu,
                                                             int maxOutVertices, int maxOutTris, double* outXyz, float* outNormal,
                                                             uint* outRgba8, int* outInfo, int* outTri, int* vertexMap, int* comp,
                                                             int* report);

    // The mesh decimated by adaptive vertex clustering.  A mesh in the layout above (dCounts: the report of pgx_mesh_dev, of
    // pgx_mesh_clean_dev or of this call on the device, or null) with the vertices of a grid block of 2^l cells, l in lmin .. lmax,
    // merged where the block's triangle normals agree (flatQ in 1/1024): dOutXyz .. dOutTri as the mesh's, dOutInfo =
    // (name, level, members, 0), dVertexMap [maxVertices] and dLevel [maxVertices] int32 or null, dReport [8] ([5] vertices,
    // [6] triangles out).  The host form takes host arrays in the same layouts
    [DllImport(Lib)] public static extern int pgx_mesh_decimate_dev(IntPtr ctx, void* dXyz, void* dNormal, void* dRgba8, void* dInfo,
                                                                    void* dTri, void* dCounts, int maxVertices, int maxTris, double cell,
                                                                    double ox, double oy, double oz, int lmin, int lmax, int flatQ,
                                                                    int maxOutVertices, int maxOutTris, void* dOutXyz, void* dOutNormal,
                                                                    void* dOutRgba8, void* dOutInfo, void* dOutTri, void* dVertexMap,
                                                                    void* dLevel, void* dReport);
    [DllImport(Lib)] public static extern int pgx_mesh_decimate(IntPtr ctx, double* xyz, float* normal, uint* rgba8, int* info, int* tri,
                                                                int nVertices, int nTris, double cell, double ox, double oy, double oz,
                                                                int lmin, int lmax, int flatQ, int maxOutVertices, int maxOutTris,
                                                                double* outXyz, float* outNormal, uint* outRgba8, int* outInfo,
                                                                int* outTri, int* vertexMap, int* level, int* report);

    /// <summary>Maps a status code back to the exception type the managed implementation throws.</summary>
    public static void Check(IntPtr ctx, int rc)
    {
        if (rc == Ok) return;
        var msg = Marshal.PtrToStringUTF8(pgx_last_error(ctx)) ?? "pgx error";
        throw rc switch
        {
            EDimMismatch or EBadArg => new ArgumentException(msg),          // DeWarp.cs:23, :48
            EOobSource => new IndexOutOfRangeException(msg),                // Matrix.cs:65, :207
            EEmptySet => new ArgumentOutOfRangeException(msg),              // KeypointMatching.cs:61
            ERccl => new System.IO.IOException(msg),                        // a collective or the RCCL library failed (multi-GPU only)
            _ => new InvalidOperationException(msg),
        };
    }
}

/// <summary>One context per GPU; registered as a DI singleton (Program.cs:40-59).</summary>
public sealed class PgxContext : IDisposable
{
    internal IntPtr Handle;
    public PgxContext(int device = 0) => PgxNative.Check(IntPtr.Zero, PgxNative.pgx_ctx_create(device, out Handle));
    public void Dispose() { if (Handle != IntPtr.Zero) { PgxNative.pgx_ctx_destroy(Handle); Handle = IntPtr.Zero; } }
}
