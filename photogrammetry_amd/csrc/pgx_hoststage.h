// pgx_hoststage.h -- buffers laid out in 256-byte-aligned sections: the workspace carver of the launchers and, on it, the
// image that a host form uploads or downloads in (HostImage), with the section lists that the twenty host forms on it share:
// tracks_in (triangulation, bundle adjustment, registration, track consensus), pair_in (verification, relative pose),
// two_sets_in and knn_out (pgx_match, pgx_knn, pgx_knn_guided), batch_in (pgx_match_batch), mesh_in (pgx_mesh_clean,
// pgx_mesh_decimate) and mesh_out (those two and pgx_mesh).  The other seven (pgx_vocab_train, pgx_select_pairs, pgx_depth_maps,
// pgx_depth_fuse, pgx_dense_views, pgx_rgba8_batch, pgx_cloud_merge) and what the three mesh forms have besides a mesh list
// declare their lists where they stand in pgx_api.hip.
// Host code without HIP: tests/hoststage_driver.cpp builds it with g++ under sanitizers, and pgx_api.hip puts the copies
// around it (stage_images, download_images).  Internal to libpgx.so; DESIGN.md section 14g.
#pragma once

#include "../../include/pgx.h"

#include <algorithm>
#include <cstring>
#include <vector>

// Hands out 256-byte-aligned sections of a workspace, so that a stage describes its layout once: the launcher carves
// the real buffer, *_ws_bytes the null one and reads total().
struct WsCarver {
    char *base;
    size_t at = 0;
    explicit WsCarver(void *ws) : base(static_cast<char *>(ws)) {}
    static size_t align256(size_t b) { return (b + 255) & ~(size_t)255; }
    size_t put(size_t bytes)   // the section's offset
    {
        const size_t p = at;
        at += align256(bytes);
        return p;
    }
    template <class T> T *take(size_t bytes)
    {
        const size_t p = put(bytes);
        return base ? reinterpret_cast<T *>(base + p) : nullptr;
    }
    size_t total() const { return at; }
};

// The inputs or the outputs of a host form as one image.  A section is declared once, add(host, n, elem, at_least, present):
// max(n, at_least) elements of `elem` bytes, the first n of which travel from the host source (pack) or to the host
// destination (moves, after the launch); none travel with host null or n 0.  An absent section is carved like any
// other, but dev() is null and nothing travels.  The sources are only read: `host` is not const for the outputs' sake.
struct HostImage {
    struct Sec { size_t off; bool present; };
    struct Move { size_t off; void *host; size_t bytes; };   // off: from the image's start
    std::vector<Sec> secs;
    std::vector<Move> moves;
    WsCarver w{nullptr};
    char *base = nullptr;                      // where the image lies on the device
    bool ascending = true;                     // no source so far begins before the end of the one declared before it
    std::vector<std::vector<int32_t>> words;   // add_words' blocks: `moves` points into them, so an image is not copied
    HostImage() = default; HostImage(const HostImage &) = delete; HostImage &operator=(const HostImage &) = delete;

    int add(const void *host, size_t n, size_t elem, size_t at_least = 0, bool present = true)
    {
        secs.push_back({w.put(std::max(n, at_least) * elem), present});
        if (present) put_at(0, host, n * elem);
        return (int)secs.size() - 1;
    }
    void put_at(size_t at, const void *host, size_t bytes)   // one more source inside the section declared last, `at` bytes in
    {
        if (!host || !bytes) return;
        ascending &= moves.empty() || moves.back().off + moves.back().bytes <= secs.back().off + at;
        moves.push_back({secs.back().off + at, const_cast<void *>(host), bytes});
    }
    int add_words(std::initializer_list<int32_t> v, size_t at_least)   // a few words held by value
    {
        words.emplace_back(v);
        return add(words.back().data(), v.size(), 4, at_least);
    }
    // keypoints by slot: counts[f] elements of frame f, frame behind frame in src, to slot f of `stride` elements
    int add_slots(const void *src, const int32_t *counts, size_t n_slots, size_t stride, size_t elem)
    {
        const int s = add(nullptr, 0, elem, n_slots * stride);
        for (size_t f = 0, k = 0; f < n_slots; k += counts[f], f++)
            put_at(f * stride * elem, static_cast<const char *>(src) + k * elem, counts[f] * elem);
        return s;
    }
    size_t total() const { return w.total(); }
    void pack(char *dst) const   // all total() bytes: zero wherever no source lies (sources in ascending order: only there)
    {
        size_t at = 0;
        if (!ascending) std::memset(dst, 0, at = total());
        for (const Move &m : moves) {
            if (ascending) std::memset(dst + at, 0, m.off - at), at = m.off + m.bytes;
            std::memcpy(dst + m.off, m.host, m.bytes);
        }
        std::memset(dst + at, 0, total() - at);
    }
    template <class T> T *dev(int s) const { return secs[s].present ? reinterpret_cast<T *>(base + secs[s].off) : nullptr; }
};

// The keypoints and the track graph of a host form, checked: stride = max(counts, 1), n_nodes = track_offsets[n_tracks].
struct HostTracks {
    const pgx_keypoint *kps; const int32_t *counts, *track_offsets, *nodes; int n_frames, n_tracks, stride; long long n_nodes;
};

// triangulation, bundle adjustment, registration: keypoints [n_frames][stride], the stage's per-frame arrays (frame_src,
// frame_bytes per frame; nullptr ends the list), offsets, nodes, with per_track the points and flags of the tracks, and
// the track summary's {n_tracks, n_nodes}
struct TracksIn { int kp, frame[3], off, nodes, xyz, flags, ts; };
inline TracksIn tracks_in(HostImage &in, const HostTracks &t, const void *const (&frame_src)[3], const size_t (&frame_bytes)[3],
                          bool per_track, const double *xyz, const int32_t *track_flags)
{
    TracksIn s{};
    s.kp = in.add_slots(t.kps, t.counts, t.n_frames, t.stride, sizeof(pgx_keypoint));
    for (int i = 0; i < 3 && frame_src[i]; i++) s.frame[i] = in.add(frame_src[i], t.n_frames, frame_bytes[i]);
    s.off = in.add(t.track_offsets, t.n_tracks + 1, 4);
    s.nodes = in.add(t.nodes, t.n_nodes, 8, 1);
    if (per_track) {
        s.xyz = in.add(xyz, t.n_tracks, 24, 1);
        s.flags = in.add(track_flags, t.n_tracks, 4, 1, track_flags != nullptr);
    }
    s.ts = in.add_words({t.n_tracks, (int32_t)t.n_nodes}, 64);
    return s;
}

// verification, relative pose: two keypoint sets as the image pair (1, 2) of three slots of S: keypoints [3][S] (slot 0
// unused), the list [S], and meta = the counts {0, n1, n2} with the pair list {1, 2} behind them
struct PairIn { int kp, list, meta; };
inline PairIn pair_in(HostImage &in, const pgx_keypoint *kp1, int n1, const pgx_keypoint *kp2, int n2, const pgx_pair *matches, int S)
{
    const size_t K = sizeof(pgx_keypoint);
    const int kp = in.add(nullptr, 0, K, 3 * S);
    in.put_at(S * K, kp1, n1 * K);
    in.put_at(2 * S * K, kp2, n2 * K);
    return {kp, in.add(matches, n1, sizeof(pgx_pair), S), in.add_words({0, n1, n2, 1, 2}, 16)};   // in this order
}

// the matchers.  No loader of k_match.hip, k_match_mfma.inc, k_knn.hip or k_guided.hip reads a descriptor or keypoint row
// at or past a frame's count, so neither list below needs slack behind its last slot.
// pgx_match, pgx_knn, pgx_knn_guided: two sets as the image pair (0, 1) of two slots of S: descriptors [2][S][words], the
// counts {n1, n2} with the pair list {0, 1} behind them, and for the guided form (F given) keypoints [2][S] and F [9]; the
// other two forms carry empty absent sections in their place
struct TwoSetsIn { int desc, kp, meta, F; };
inline TwoSetsIn two_sets_in(HostImage &in, const uint32_t *desc1, const pgx_keypoint *kp1, int n1, const uint32_t *desc2,
                             const pgx_keypoint *kp2, int n2, int S, int words, const float *F)
{
    const size_t D = (size_t)words * 4, K = sizeof(pgx_keypoint);
    TwoSetsIn s{};
    s.desc = in.add(nullptr, 0, D, 2 * (size_t)S);
    in.put_at(0, desc1, n1 * D);
    in.put_at(S * D, desc2, n2 * D);
    s.kp = in.add(nullptr, 0, K, F ? 2 * (size_t)S : 0, F != nullptr);
    if (F) in.put_at(0, kp1, n1 * K), in.put_at(S * K, kp2, n2 * K);
    s.meta = in.add_words({n1, n2, 0, 1}, 16);
    s.F = in.add(F, F ? 9 : 0, sizeof(float), 0, F != nullptr);
    return s;
}

// ... and the outputs of pgx_knn and pgx_knn_guided: idx [S][k], dist [S][k], and col_nn [S], absent with a null col_nn_out
struct KnnOut { int idx, dist, col; };
inline KnnOut knn_out(HostImage &out, int n1, int n2, int S, int k, int32_t *idx_out, int32_t *dist_out, int32_t *col_nn_out)
{
    const size_t rows = (size_t)n1 * k, slots = (size_t)S * k;
    return {out.add(idx_out, rows, 4, slots), out.add(dist_out, rows, 4, slots), out.add(col_nn_out, n2, 4, S, col_nn_out != nullptr)};
}

// pgx_match_batch: descriptors [n_frames][S][words], of which only the frames that some pair references (used[f]) are
// read from the caller, then counts [n_frames] and pair_list [n_pairs][2]
struct BatchIn { int desc, counts, pairs; };
inline BatchIn batch_in(HostImage &in, const uint32_t *const *descs, const int32_t *counts, const char *used, int n_frames, int S,
                        int words, const int32_t *pair_list, int n_pairs)
{
    const size_t D = (size_t)words * 4;
    const int desc = in.add(nullptr, 0, D, (size_t)n_frames * S);
    for (int f = 0; f < n_frames; f++)
        if (used[f]) in.put_at((size_t)f * S * D, descs[f], counts[f] * D);
    return {desc, in.add(counts, n_frames, 4), in.add(pair_list, n_pairs, 8)};   // in this order
}

// the five arrays of a mesh in pgx_mesh_dev's layout, as a stage reads them and as it writes them
struct MeshList { const double *xyz; const float *normal; const uint32_t *rgba8; const int32_t *info, *tri; };
struct MeshRows { double *xyz; float *normal; uint32_t *rgba8; int32_t *info, *tri; };

// ... and as sections of an image; mesh_dev: where they lie on the device
struct MeshIn { int xyz, normal, rgba8, info, tri; };
struct MeshOut { int xyz, normal, rgba8, info, tri; };
template <class P, class S> P mesh_dev_of(const HostImage &im, const S &s)
{
    return {im.dev<double>(s.xyz), im.dev<float>(s.normal), im.dev<uint32_t>(s.rgba8), im.dev<int32_t>(s.info), im.dev<int32_t>(s.tri)};
}
inline MeshList mesh_dev(const HostImage &in, const MeshIn &s) { return mesh_dev_of<MeshList>(in, s); }
inline MeshRows mesh_dev(const HostImage &out, const MeshOut &s) { return mesh_dev_of<MeshRows>(out, s); }

// pgx_mesh_clean, pgx_mesh_decimate: a mesh list of n vertices (xyz, normal, rgba8, info) and t triangles
inline MeshIn mesh_in(HostImage &in, const double *xyz, const float *normal, const uint32_t *rgba8, const int32_t *info, const int32_t *tri,
                      size_t n, size_t t)
{
    return {in.add(xyz, n, 24, 1), in.add(normal, n, 12, 1), in.add(rgba8, n, 4, 1), in.add(info, n, 16, 1), in.add(tri, t, 12, 1)};   // in this order
}

// ... and the mesh list that those two and pgx_mesh write, of at most mv vertices and mt triangles: carved and not downloaded.  The
// form declares the report before it (and its per-vertex maps behind the report): the report's download tells how many rows
// of these sections there are to fetch.
inline MeshOut mesh_out(HostImage &out, size_t mv, size_t mt)
{
    return {out.add(nullptr, 0, 24, mv + 1), out.add(nullptr, 0, 12, mv + 1), out.add(nullptr, 0, 4, mv + 1), out.add(nullptr, 0, 16, mv + 1),
            out.add(nullptr, 0, 12, mt + 1)};   // in this order
}
