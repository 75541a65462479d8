// Stand-alone driver of the host forms' staging images (photogrammetry_amd/csrc/pgx_hoststage.h) for tests/test_hoststage.py:
// argv[1] names a host form, whose section lists are checked at every size of the test's docstring against images laid out
// naively here.  The input lists are the header's own (tracks_in, pair_in, two_sets_in, batch_in, mesh_in), and so are knn_out
// and mesh_out; the other output lists, F and K of pgx_relative_pose, and S and `used` of pgx_match_batch are declared or
// computed here word for word as the form in pgx_api.hip does.  So are both lists of the nine later forms (pgx_track_consensus's
// inputs and pgx_mesh's mesh_out excepted): pgx_vocab_train, pgx_select_pairs, pgx_depth_maps, pgx_depth_fuse, pgx_dense_views,
// pgx_rgba8_batch, pgx_cloud_merge and pgx_mesh declare them inside pgx_api.hip, and so are the report and the per-vertex maps
// of pgx_mesh_clean and pgx_mesh_decimate.  For pgx_depth_fuse, pgx_cloud_merge and the three mesh forms the report
// must be the output image's first download, and the lists of max + 1 rows behind it none.  Host code only; the test
// builds it with -fsanitize=address,undefined, and every buffer has its exact size, so a read or write past an end is a
// sanitizer report.  Exit status 0 and "ok <checks>" on stdout, or 1 and the first failure on stderr.
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "../photogrammetry_amd/csrc/pgx_hoststage.h"

namespace {

typedef std::vector<char> Bytes;
int n_checks = 0;

#define CHECK(cond)                                                            \
    do {                                                                       \
        n_checks++;                                                            \
        if (!(cond)) {                                                         \
            std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond);    \
            std::exit(1);                                                      \
        }                                                                      \
    } while (0)

size_t up256(size_t b) { return (b + 255) / 256 * 256; }

// n elements of T with no two bytes alike in a row, in a buffer of exactly that size (nullptr for none)
template <class T> struct Src {
    std::vector<T> v;
    explicit Src(size_t n, unsigned seed) : v(n)
    {
        char *b = reinterpret_cast<char *>(v.data());
        for (size_t i = 0; i < n * sizeof(T); i++) b[i] = (char)(1 + (i * 7 + seed * 13) % 251);
    }
    T *p() { return v.empty() ? nullptr : v.data(); }
    Bytes bytes(size_t first = 0, size_t n = (size_t)-1) const
    {
        const char *b = reinterpret_cast<const char *>(v.data());
        if (n == (size_t)-1) n = v.size() - first;
        return Bytes(b + first * sizeof(T), b + (first + n) * sizeof(T));
    }
};

// a section as the driver expects it: its size and, for an input, its content (shorter than the size: zero behind it)
struct Want {
    size_t bytes;
    Bytes content;     // inputs
    bool present;
    void *dst;         // outputs: where `down` bytes go
    size_t down;
};
Want in_sec(size_t bytes, Bytes content = Bytes(), bool present = true) { return {bytes, content, present, nullptr, 0}; }
Want out_sec(size_t bytes, void *dst, size_t down, bool present = true) { return {bytes, Bytes(), present, dst, down}; }
void place(Bytes &b, size_t at, const Bytes &src) { b.insert(b.end(), at - b.size(), 0), b.insert(b.end(), src.begin(), src.end()); }
void pad(Bytes &b, size_t n) { b.resize(n, 0); }

// offsets aligned, disjoint and in declaration order, the total their sum; the packed image equal to the naive one
void check_in(HostImage &in, const std::vector<int> &ids, const std::vector<Want> &want)
{
    CHECK(in.secs.size() == want.size() && ids.size() == want.size());
    Bytes naive;
    size_t at = 0;
    char *const base = reinterpret_cast<char *>(0x10000);
    in.base = base;
    for (size_t s = 0; s < want.size(); s++) {
        CHECK(ids[s] == (int)s && in.secs[s].off == at && at % 256 == 0);
        CHECK(in.dev<char>(ids[s]) == (want[s].present ? base + at : nullptr));
        CHECK(want[s].content.size() <= want[s].bytes);
        pad(naive, at);
        if (want[s].present) naive.insert(naive.end(), want[s].content.begin(), want[s].content.end());
        at += up256(want[s].bytes);
    }
    pad(naive, at);
    CHECK(in.total() == at);
    Bytes got(in.total(), (char)0xAA);   // exactly total(): pack() must write all of it and nothing else
    in.pack(got.data());
    CHECK(got == naive);
}

// ... and for the outputs: null for an absent section, and the downloads those of the present sections with something to copy
void check_out(HostImage &out, const std::vector<int> &ids, const std::vector<Want> &want)
{
    CHECK(out.secs.size() == want.size() && ids.size() == want.size());
    char *const base = reinterpret_cast<char *>(0x20000);
    out.base = base;
    const std::vector<HostImage::Move> &d = out.moves;
    size_t at = 0, k = 0;
    for (size_t s = 0; s < want.size(); s++) {
        CHECK(ids[s] == (int)s && out.secs[s].off == at && at % 256 == 0);
        CHECK(out.dev<char>(ids[s]) == (want[s].present ? base + at : nullptr));
        if (want[s].present && want[s].dst && want[s].down) {
            CHECK(want[s].down <= want[s].bytes);
            CHECK(k < d.size() && d[k].off == at && d[k].host == want[s].dst && d[k].bytes == want[s].down);
            k++;
        }
        at += up256(want[s].bytes);
    }
    CHECK(k == d.size() && out.total() == at);
}

const int32_t COUNTS[3] = {0, 5, 2};
const int N_TRACKS[3] = {0, 1, 7}, N_NODES[2] = {0, 19};
size_t max1(size_t n) { return n > 0 ? n : 1; }

// kind 0: triangulation, 1: bundle adjustment, 2: registration, 9: track consensus (triangulation's inputs)
void tracks_form(int kind)
{
    const bool by_P = kind == 0 || kind == 9;
    for (int n_frames : {1, 3})
        for (int n_tracks : N_TRACKS)
            for (int n_nodes : N_NODES)
                for (int optional = 0; optional < 2; optional++) {
                    if (n_tracks == 0 && n_nodes > 0) continue;
                    int stride = 1, n_kp = 0;
                    for (int f = 0; f < n_frames; f++) stride = COUNTS[f] > stride ? COUNTS[f] : stride, n_kp += COUNTS[f];
                    const size_t nf = n_frames, nt = n_tracks, nn = n_nodes;
                    Src<pgx_keypoint> kps(n_kp, 1);
                    Src<double> P(nf * 12, 2), K(nf * 4, 3), Rt(nf * 12, 4), xyz(nt * 3, 5);
                    Src<int32_t> sel(nf, 6), off(nt + 1, 7), nodes(nn * 2, 8), flags(optional ? nt : 0, 9);
                    Bytes slots;
                    for (int f = 0, k = 0; f < n_frames; k += COUNTS[f], f++) place(slots, (size_t)f * stride * 16, kps.bytes(k, COUNTS[f]));
                    const int32_t ts[2] = {n_tracks, n_nodes};
                    const Bytes ts_b(reinterpret_cast<const char *>(ts), reinterpret_cast<const char *>(ts) + 8);
                    HostImage in;
                    const HostTracks t = {kps.p(), COUNTS, off.p(), nodes.p(), n_frames, n_tracks, stride, n_nodes};
                    const TracksIn i = by_P ? tracks_in(in, t, {P.p(), nullptr, nullptr}, {96, 0, 0}, false, nullptr, nullptr)
                                            : tracks_in(in, t, {K.p(), Rt.p(), sel.p()}, {32, 96, 4}, true, xyz.p(), flags.p());
                    if (by_P)
                        check_in(in, {i.kp, i.frame[0], i.off, i.nodes, i.ts},
                                 {in_sec(nf * stride * 16, slots), in_sec(nf * 96, P.bytes()), in_sec((nt + 1) * 4, off.bytes()),
                                  in_sec(max1(nn) * 8, nodes.bytes()), in_sec(256, ts_b)});
                    else
                        check_in(in, {i.kp, i.frame[0], i.frame[1], i.frame[2], i.off, i.nodes, i.xyz, i.flags, i.ts},
                                 {in_sec(nf * stride * 16, slots), in_sec(nf * 32, K.bytes()), in_sec(nf * 96, Rt.bytes()),
                                  in_sec(nf * 4, sel.bytes()), in_sec((nt + 1) * 4, off.bytes()), in_sec(max1(nn) * 8, nodes.bytes()),
                                  in_sec(max1(nt) * 24, xyz.bytes()), in_sec(max1(nt) * 4, flags.bytes(), flags.p() != nullptr),
                                  in_sec(256, ts_b)});
                    // destinations: any distinct non-null addresses; the optional per-node output absent in half of the cases
                    double d[8];
                    int32_t w[8];
                    double *const per_node = optional ? d + 7 : nullptr;
                    int32_t *const per_node_i = optional ? w + 7 : nullptr;
                    HostImage out;
                    if (kind == 0 && n_tracks > 0) {   // the form returns before any staging at n_tracks == 0
                        check_out(out, {out.add(d, n_tracks, 24), out.add(d + 1, n_tracks, 24), out.add(per_node, t.n_nodes, 8, 1, per_node != nullptr),
                                        out.add(w, n_tracks, 4), out.add(w + 1, 8, 4, 64)},
                                  {out_sec(nt * 24, d, nt * 24), out_sec(nt * 24, d + 1, nt * 24), out_sec(max1(nn) * 8, per_node, nn * 8, optional),
                                   out_sec(nt * 4, w, nt * 4), out_sec(256, w + 1, 32)});
                    } else if (kind == 1) {
                        for (int max_iters : {0, 20}) {
                            HostImage ob;
                            const size_t tr = (size_t)(max_iters + 1) * 16;
                            check_out(ob, {ob.add(d, n_frames, 96), ob.add(d + 1, n_frames, 96), ob.add(d + 2, n_tracks, 24, 1),
                                           ob.add(per_node, t.n_nodes, 8, 1, per_node != nullptr), ob.add(d + 3, max_iters + 1, 16),
                                           ob.add(w, 8, 4, 64)},
                                      {out_sec(nf * 96, d, nf * 96), out_sec(nf * 96, d + 1, nf * 96), out_sec(max1(nt) * 24, d + 2, nt * 24),
                                       out_sec(max1(nn) * 8, per_node, nn * 8, optional), out_sec(tr, d + 3, tr), out_sec(256, w, 32)});
                        }
                    } else if (kind == 2) {
                        check_out(out, {out.add(d, n_frames, 96), out.add(d + 1, n_frames, 96), out.add(w, n_frames, 16), out.add(d + 2, n_frames, 16),
                                        out.add(per_node_i, t.n_nodes, 4, 1, per_node_i != nullptr), out.add(w + 1, 8, 4, 64)},
                                  {out_sec(nf * 96, d, nf * 96), out_sec(nf * 96, d + 1, nf * 96), out_sec(nf * 16, w, nf * 16),
                                   out_sec(nf * 16, d + 2, nf * 16), out_sec(max1(nn) * 4, per_node_i, nn * 4, optional), out_sec(256, w + 1, 32)});
                    } else if (kind == 9 && n_tracks > 0) {   // the form returns before any staging at n_tracks == 0
                        // the per-track outputs null in half of the cases: carved for the kernels, not downloaded
                        int32_t *const map = optional ? w + 3 : nullptr, *const fl = optional ? w + 4 : nullptr, *const st = optional ? w + 5 : nullptr;
                        double *const pts = optional ? d : nullptr;
                        check_out(out, {out.add(w, n_tracks + 1, 4), out.add(w + 1, t.n_nodes, 8, 1), out.add(w + 2, 8, 4, 64),
                                        out.add(map, n_tracks, 4), out.add(pts, n_tracks, 24), out.add(fl, n_tracks, 4),
                                        out.add(st, n_tracks, 16), out.add(w + 6, 8, 4, 64)},
                                  {out_sec((nt + 1) * 4, w, (nt + 1) * 4), out_sec(max1(nn) * 8, w + 1, nn * 8), out_sec(256, w + 2, 32),
                                   out_sec(nt * 4, map, nt * 4), out_sec(nt * 24, pts, nt * 24), out_sec(nt * 4, fl, nt * 4),
                                   out_sec(nt * 16, st, nt * 16), out_sec(256, w + 6, 32)});
                    }
                }
}

// kind 3: verification, 4: relative pose
void pair_form(int kind)
{
    const int N[4][2] = {{0, 0}, {0, 4}, {4, 0}, {5, 3}};
    for (const int(&n)[2] : N)
        for (int optional = 0; optional < 2; optional++) {
            const int n1 = n[0], n2 = n[1], S = n1 > n2 ? n1 : (n2 > 0 ? n2 : 1);
            Src<pgx_keypoint> kp1(n1, 1), kp2(n2, 2);
            Src<pgx_pair> ml(n1, 3);
            Src<double> F(9, 4), Ka(4, 5), Kb(4, 6);
            Bytes kp, Kimg;
            place(kp, (size_t)S * 16, kp1.bytes());
            place(kp, (size_t)2 * S * 16, kp2.bytes());
            place(Kimg, 32, Ka.bytes());
            place(Kimg, 64, Kb.bytes());
            const int32_t meta[5] = {0, n1, n2, 1, 2};
            const Bytes meta_b(reinterpret_cast<const char *>(meta), reinterpret_cast<const char *>(meta) + 20);
            HostImage in;
            const PairIn i = pair_in(in, kp1.p(), n1, kp2.p(), n2, ml.p(), S);
            std::vector<int> ids = {i.kp, i.list, i.meta};
            std::vector<Want> want = {in_sec((size_t)3 * S * 16, kp), in_sec((size_t)S * 12, ml.bytes()), in_sec(64, meta_b)};
            if (kind == 4) {   // as pgx_relative_pose adds them
                ids.push_back(in.add(F.p(), 9, 8));
                ids.push_back(in.add(nullptr, 0, 32, 3));
                in.put_at(32, Ka.p(), 32);
                in.put_at(64, Kb.p(), 32);
                want.push_back(in_sec(72, F.bytes()));
                want.push_back(in_sec(96, Kimg));
            }
            check_in(in, ids, want);
            double d[8];
            int32_t w[8];
            pgx_pair pr[1];
            HostImage out;
            if (kind == 3) {
                int32_t *const inl = optional ? w + 1 : nullptr;
                check_out(out, {out.add(pr, n1, sizeof(pgx_pair), S), out.add(d, 9, 8), out.add(w, 8, 4), out.add(inl, n1, 4, S, inl != nullptr),
                                out.add(nullptr, 0, 4, 8)},
                          {out_sec((size_t)S * 12, pr, (size_t)n1 * 12), out_sec(72, d, 72), out_sec(32, w, 32),
                           out_sec((size_t)S * 4, inl, (size_t)n1 * 4, optional), out_sec(32, nullptr, 0)});
            } else {
                double *const cand = optional ? d + 2 : nullptr;
                check_out(out, {out.add(d, 12, 8), out.add(w, 8, 4), out.add(d + 1, 1, 8), out.add(cand, 48, 8, 0, cand != nullptr),
                                out.add(nullptr, 0, 96, 2 * 3), out.add(nullptr, 0, 4, 2 * 3 + 16), out.add(nullptr, 0, 4, 8)},
                          {out_sec(96, d, 96), out_sec(32, w, 32), out_sec(8, d + 1, 8), out_sec(384, cand, 384, optional),
                           out_sec(576, nullptr, 0), out_sec(88, nullptr, 0), out_sec(32, nullptr, 0)});
            }
        }
}

Bytes words_of(std::initializer_list<int32_t> v)
{
    const char *b = reinterpret_cast<const char *>(v.begin());
    return Bytes(b, b + 4 * v.size());
}

// kind 5: pgx_match, 6: pgx_knn, 7: pgx_knn_guided (the only one with keypoints and F)
void two_sets_form(int kind)
{
    const int N[3][2] = {{0, 4}, {4, 0}, {5, 3}};
    const bool guided = kind == 7;
    for (const int(&n)[2] : N)
        for (int words : {1, 8})
            for (int k : {1, 2})
                for (int col = 0; col < 2; col++) {
                    if (kind == 5 && (k == 2 || col)) continue;   // pgx_match has neither
                    const int n1 = n[0], n2 = n[1], S = n1 > n2 ? n1 : n2;
                    const size_t D = (size_t)words * 4;
                    Src<uint32_t> d1((size_t)n1 * words, 1), d2((size_t)n2 * words, 2);
                    Src<pgx_keypoint> kp1(guided ? n1 : 0, 3), kp2(guided ? n2 : 0, 4);
                    Src<float> F(guided ? 9 : 0, 5);
                    Bytes desc, kp;
                    place(desc, 0, d1.bytes());
                    place(desc, S * D, d2.bytes());
                    place(kp, 0, kp1.bytes());
                    if (guided) place(kp, (size_t)S * 16, kp2.bytes());
                    HostImage in;
                    const TwoSetsIn i = two_sets_in(in, d1.p(), kp1.p(), n1, d2.p(), kp2.p(), n2, S, words, F.p());
                    check_in(in, {i.desc, i.kp, i.meta, i.F},
                             {in_sec(2 * S * D, desc), in_sec(guided ? (size_t)2 * S * 16 : 0, kp, guided), in_sec(64, words_of({n1, n2, 0, 1})),
                              in_sec(guided ? 36 : 0, F.bytes(), guided)});
                    int32_t w[3];
                    pgx_pair pr[1];
                    HostImage out;
                    if (kind == 5) {
                        check_out(out, {out.add(pr, n1, sizeof(pgx_pair), S)}, {out_sec((size_t)S * 12, pr, (size_t)n1 * 12)});
                    } else {
                        int32_t *const cn = col ? w + 2 : nullptr;
                        const KnnOut o = knn_out(out, n1, n2, S, k, w, w + 1, cn);
                        check_out(out, {o.idx, o.dist, o.col},
                                  {out_sec((size_t)S * k * 4, w, (size_t)n1 * k * 4), out_sec((size_t)S * k * 4, w + 1, (size_t)n1 * k * 4),
                                   out_sec((size_t)S * 4, cn, (size_t)n2 * 4, col)});
                    }
                }
}

// kind 8: pgx_match_batch; S and `used` as the form computes them.  The last case has a fourth frame of 9 rows that no pair
// names: its source is null, so that reading it is a crash, and it must not widen S.
void batch_form()
{
    const int32_t counts[4] = {0, 5, 2, 9};
    const std::vector<std::vector<int32_t>> LISTS = {{}, {1, 2}, {1, 2, 2, 1}};
    for (int n_frames : {3, 4})
        for (const std::vector<int32_t> &pl : LISTS)
            for (int words : {1, 8}) {
                if (n_frames == 4 && pl.size() != 4) continue;
                const int n_pairs = (int)pl.size() / 2;
                const size_t D = (size_t)words * 4;
                int S = 1;
                char used[4] = {0, 0, 0, 0};
                for (int32_t f : pl) used[f] = 1, S = counts[f] > S ? counts[f] : S;
                CHECK(S == (n_pairs ? 5 : 1));
                std::vector<Src<uint32_t>> src;
                const uint32_t *descs[4];
                Bytes desc;
                for (int f = 0; f < n_frames; f++) {
                    src.emplace_back(f < 3 ? (size_t)counts[f] * words : 0, 10 + f);
                    if (used[f]) place(desc, (size_t)f * S * D, src[f].bytes());
                }
                for (int f = 0; f < n_frames; f++) descs[f] = src[f].p();
                const Bytes counts_b(reinterpret_cast<const char *>(counts), reinterpret_cast<const char *>(counts) + 4 * n_frames);
                const Bytes pl_b(reinterpret_cast<const char *>(pl.data()), reinterpret_cast<const char *>(pl.data()) + 4 * pl.size());
                HostImage in;
                const BatchIn i = batch_in(in, descs, counts, used, n_frames, S, words, pl.empty() ? nullptr : pl.data(), n_pairs);
                check_in(in, {i.desc, i.counts, i.pairs}, {in_sec((size_t)n_frames * S * D, desc), in_sec(4 * n_frames, counts_b), in_sec(8 * n_pairs, pl_b)});
                HostImage out;   // carved, not downloaded: the form copies all lists to its pinned buffer in one piece
                check_out(out, {out.add(nullptr, 0, sizeof(pgx_pair), (size_t)n_pairs * S)}, {out_sec((size_t)n_pairs * S * 12, nullptr, 0)});
            }
}

// ---- the nine later forms.  Their lists are declared inside pgx_api.hip; each is repeated here word for word. ----------------

// the report travels first: the form reads from it how many rows of the lists behind it to fetch
void report_first(const HostImage &out, const void *report, size_t bytes)
{
    CHECK(!out.moves.empty() && out.moves[0].off == 0 && out.moves[0].host == report && out.moves[0].bytes == bytes);
}

const int RS[3] = {0, 1, 3}, NS[3] = {0, 1, 7}, CAPS[2] = {0, 5}, DIMS[2][2] = {{1, 1}, {5, 3}};

// kind 10: pgx_vocab_train, 11: pgx_select_pairs (scores optional)
void vocab_form(int kind)
{
    for (int F : {1, 3})
        for (int stride : {1, 5})
            for (int V : {1, 7})
                for (int max_pairs : CAPS)
                    for (int optional = 0; optional < 2; optional++) {
                        if (kind == 10 && (max_pairs || optional)) continue;   // pgx_vocab_train has neither
                        const size_t nd = (size_t)F * stride;
                        Src<uint32_t> desc(nd * 8, 1), vocab(kind == 11 ? (size_t)V * 8 : 0, 3);
                        Src<int32_t> counts(F, 2);
                        uint32_t voc_out[1];
                        int32_t w[8];
                        HostImage in, out;
                        if (kind == 10) {
                            check_in(in, {in.add(desc.p(), (size_t)F * stride, 32), in.add(counts.p(), F, 4)},
                                     {in_sec(nd * 32, desc.bytes()), in_sec((size_t)F * 4, counts.bytes())});
                            check_out(out, {out.add(voc_out, V, 32), out.add(w, 4, 4, 16)},
                                      {out_sec((size_t)V * 32, voc_out, (size_t)V * 32), out_sec(64, w, 16)});
                            continue;
                        }
                        check_in(in, {in.add(desc.p(), (size_t)F * stride, 32), in.add(counts.p(), F, 4), in.add(vocab.p(), V, 32)},
                                 {in_sec(nd * 32, desc.bytes()), in_sec((size_t)F * 4, counts.bytes()), in_sec((size_t)V * 32, vocab.bytes())});
                        int32_t *const pairlist = max_pairs ? w : nullptr, *const pair_score = max_pairs ? w + 1 : nullptr;
                        int32_t *const scores = optional ? w + 2 : nullptr, *const summary = w + 3;
                        const size_t mp = max_pairs, ff = (size_t)F * F;
                        check_out(out, {out.add(pairlist, max_pairs, 8, 1), out.add(pair_score, max_pairs, 4, 1),
                                        out.add(scores, (size_t)F * F, 4, 0, scores != nullptr), out.add(summary, 8, 4, 16)},
                                  {out_sec(max1(mp) * 8, pairlist, mp * 8), out_sec(max1(mp) * 4, pair_score, mp * 4),
                                   out_sec(ff * 4, scores, ff * 4, optional), out_sec(64, summary, 32)});
                    }
}

// kind 12: pgx_depth_maps (cost, warp, planes optional: all eight combinations), 13: pgx_depth_fuse (agree optional).  The
// forms return before any staging at R == 0; their lists hold there all the same.
void depth_form(int kind)
{
    const int S = 2, D = 5;
    for (int R : RS)
        for (const int(&wh)[2] : DIMS)
            for (int n_frames : {1, 3})
                for (int optional = 0; optional < (kind == 12 ? 8 : 2); optional++)
                    for (int max_points : CAPS) {
                        if (kind == 12 && max_points) continue;   // pgx_depth_maps has no list
                        const int W = wh[0], H = wh[1];
                        const size_t npix = (size_t)W * H, n = (size_t)R * npix, nf = n_frames, r = R;
                        Src<double> P(nf * 12, 2);
                        Src<int32_t> views(r * (1 + S), 3);
                        double d[8];
                        int32_t w[8];
                        HostImage in, out;
                        if (kind == 12) {
                            Src<float> gray(nf * npix, 1);
                            Src<double> range(r * 2, 4);
                            check_in(in, {in.add(gray.p(), (size_t)n_frames * npix, 4), in.add(P.p(), n_frames, 96),
                                          in.add(views.p(), (size_t)R * (1 + S), 4), in.add(range.p(), R, 16)},
                                     {in_sec(nf * npix * 4, gray.bytes()), in_sec(nf * 96, P.bytes()), in_sec(r * (1 + S) * 4, views.bytes()),
                                      in_sec(r * 16, range.bytes())});
                            int32_t *const cost = optional & 1 ? w + 1 : nullptr;
                            double *const warp = optional & 2 ? d + 1 : nullptr, *const planes = optional & 4 ? d + 2 : nullptr;
                            int32_t *const kq8 = w, *const flags = w + 2, *const summary = w + 3;
                            double *const depth = d;
                            check_out(out, {out.add(kq8, n, 4), out.add(depth, n, 8), out.add(cost, n, 4, 0, cost != nullptr), out.add(flags, n, 4),
                                            out.add(warp, (size_t)R * S * 12, 8, 0, warp != nullptr),
                                            out.add(planes, (size_t)R * D, 8, 0, planes != nullptr), out.add(summary, 8, 4, 64)},
                                      {out_sec(n * 4, kq8, n * 4), out_sec(n * 8, depth, n * 8), out_sec(n * 4, cost, n * 4, cost != nullptr),
                                       out_sec(n * 4, flags, n * 4), out_sec(r * S * 96, warp, r * S * 96, warp != nullptr),
                                       out_sec(r * D * 8, planes, r * D * 8, planes != nullptr), out_sec(256, summary, 32)});
                            continue;
                        }
                        Src<double> depth(n, 1);
                        check_in(in, {in.add(depth.p(), n, 8), in.add(views.p(), (size_t)R * (1 + S), 4), in.add(P.p(), n_frames, 96)},
                                 {in_sec(n * 8, depth.bytes()), in_sec(r * (1 + S) * 4, views.bytes()), in_sec(nf * 96, P.bytes())});
                        int32_t *const agree = optional ? w + 1 : nullptr, *const summary = w;
                        const size_t mp = max_points;
                        check_out(out, {out.add(summary, 4, 4, 64), out.add(agree, n, 4, 0, agree != nullptr),
                                        out.add(nullptr, 0, 24, (size_t)max_points + 1), out.add(nullptr, 0, 8, (size_t)max_points + 1)},
                                  {out_sec(256, summary, 16), out_sec(n * 4, agree, n * 4, optional), out_sec((mp + 1) * 24, nullptr, 0),
                                   out_sec((mp + 1) * 8, nullptr, 0)});
                        report_first(out, summary, 16);
                    }
}

// kind 14: pgx_dense_views: track_flags, refs and pair_counts optional (all eight combinations), ref_stats null or not with them
void dense_views_form()
{
    const int S = 2;
    for (int R : RS)
        for (int n_frames : {1, 3})
            for (int n_tracks : NS)
                for (int n_nodes : {0, 19})
                    for (int optional = 0; optional < 8; optional++) {
                        if (n_tracks == 0 && n_nodes > 0) continue;
                        const size_t nt = n_tracks, nn = n_nodes, nf = n_frames, r = R;
                        Src<int32_t> off(nt + 1, 1), nodes(nn * 2, 2), flags(optional & 1 ? nt : 0, 4), refs(optional & 2 ? r : 0, 6);
                        Src<double> xyz(nt * 3, 3), P(nf * 12, 5);
                        const bool has_flags = optional & 1, has_refs = optional & 2;
                        // a null source of an optional input that is there: never at these sizes but with nothing to copy
                        const int32_t none = 0;
                        const int32_t *const track_flags = has_flags ? (nt ? flags.p() : &none) : nullptr;
                        const int32_t *const ref_list = has_refs ? (r ? refs.p() : &none) : nullptr;
                        HostImage in, out;
                        check_in(in, {in.add(off.p(), n_tracks + 1, 4), in.add(nodes.p(), n_nodes, 8, 1), in.add(xyz.p(), n_tracks, 24, 1),
                                      in.add(track_flags, n_tracks, 4, 1, track_flags != nullptr), in.add(P.p(), n_frames, 96),
                                      in.add(ref_list, R, 4, 0, ref_list != nullptr), in.add_words({n_tracks, (int32_t)n_nodes}, 64)},
                                 {in_sec((nt + 1) * 4, off.bytes()), in_sec(max1(nn) * 8, nodes.bytes()), in_sec(max1(nt) * 24, xyz.bytes()),
                                  in_sec(max1(nt) * 4, flags.bytes(), has_flags), in_sec(nf * 96, P.bytes()), in_sec(r * 4, refs.bytes(), has_refs),
                                  in_sec(256, words_of({n_tracks, n_nodes}))});
                        double d[2];
                        int32_t w[4];
                        int32_t *const views = w, *const pair_counts = optional & 4 ? w + 1 : nullptr, *const ref_stats = optional & 4 ? w + 2 : nullptr;
                        int32_t *const report = w + 3;
                        double *const range = d;
                        check_out(out, {out.add(views, (size_t)R * (1 + S), 4), out.add(range, R, 16),
                                        out.add(pair_counts, (size_t)R * n_frames, 8, 0, pair_counts != nullptr), out.add(ref_stats, R, 16),
                                        out.add(report, 8, 4, 64)},
                                  {out_sec(r * (1 + S) * 4, views, r * (1 + S) * 4), out_sec(r * 16, range, r * 16),
                                   out_sec(r * nf * 8, pair_counts, r * nf * 8, pair_counts != nullptr), out_sec(r * 16, ref_stats, r * 16),
                                   out_sec(256, report, 32)});
                    }
}

// kind 15: pgx_rgba8_batch, the source at 8 bytes a pixel (RGBA64) and at 4 (the context's RGBA8 source format)
void rgba8_form()
{
    for (int F : {1, 3})
        for (const int(&wh)[2] : DIMS)
            for (int src8 = 0; src8 < 2; src8++) {
                const size_t n = (size_t)F * wh[0] * wh[1];
                Src<uint32_t> rgba(n * (src8 ? 1 : 2), 1);
                uint32_t dst[1];
                HostImage in, out;
                check_in(in, {in.add(rgba.p(), n, src8 ? 4 : 8)}, {in_sec(n * (src8 ? 4 : 8), rgba.bytes())});
                check_out(out, {out.add(dst, n, 4)}, {out_sec(n * 4, dst, n * 4)});
            }
}

// kind 16: pgx_cloud_merge (rgba8 in; pt_normal, cell_of out optional), 17: pgx_mesh (agree, rgba8 in optional).  Both refuse R == 0.
void cloud_form(int kind)
{
    const int S = 2;
    for (int R : {1, 3})
        for (const int(&wh)[2] : DIMS)
            for (int n_in : NS)
                for (int cap : CAPS)         // max_points; max_vertices
                    for (int cap_t : CAPS)   // max_tris
                        for (int optional = 0; optional < (kind == 16 ? 8 : 4); optional++) {
                            if (kind == 16 && cap_t) continue;
                            const int n_frames = 3;
                            const size_t npix = (size_t)wh[0] * wh[1], ni = n_in, nf = n_frames, r = R;
                            const bool has_rgba8 = optional & 1, has_agree = kind == 17 && (optional & 2);
                            Src<double> xyz(ni * 3, 1), depth(r * npix, 3), P(nf * 12, 5);
                            Src<int32_t> src(ni * 2, 2), views(r * (1 + S), 4), agree(has_agree ? r * npix : 0, 6);
                            Src<uint32_t> rgba8(has_rgba8 ? nf * npix : 0, 7);
                            int32_t w[8];
                            int32_t *const report = w;
                            HostImage in, out;
                            if (kind == 16) {
                                check_in(in, {in.add(xyz.p(), ni, 24, 1), in.add(src.p(), ni, 8, 1), in.add(depth.p(), (size_t)R * npix, 8),
                                              in.add(views.p(), (size_t)R * (1 + S), 4), in.add(P.p(), n_frames, 96),
                                              in.add(rgba8.p(), (size_t)n_frames * npix, 4, 0, rgba8.p() != nullptr)},
                                         {in_sec(max1(ni) * 24, xyz.bytes()), in_sec(max1(ni) * 8, src.bytes()), in_sec(r * npix * 8, depth.bytes()),
                                          in_sec(r * (1 + S) * 4, views.bytes()), in_sec(nf * 96, P.bytes()),
                                          in_sec(nf * npix * 4, rgba8.bytes(), has_rgba8)});
                                int32_t *const pt_normal = optional & 2 ? w + 1 : nullptr, *const cell_of = optional & 4 ? w + 2 : nullptr;
                                const size_t no = cap;
                                check_out(out, {out.add(report, 8, 4, 64), out.add(pt_normal, ni * 3, 4, 0, pt_normal != nullptr),
                                                out.add(cell_of, ni, 4, 0, cell_of != nullptr), out.add(nullptr, 0, 24, no + 1),
                                                out.add(nullptr, 0, 12, no + 1), out.add(nullptr, 0, 4, no + 1), out.add(nullptr, 0, 16, no + 1)},
                                          {out_sec(256, report, 32), out_sec(ni * 12, pt_normal, ni * 12, pt_normal != nullptr),
                                           out_sec(ni * 4, cell_of, ni * 4, cell_of != nullptr), out_sec((no + 1) * 24, nullptr, 0),
                                           out_sec((no + 1) * 12, nullptr, 0), out_sec((no + 1) * 4, nullptr, 0), out_sec((no + 1) * 16, nullptr, 0)});
                            } else {
                                check_in(in, {in.add(xyz.p(), ni, 24, 1), in.add(src.p(), ni, 8, 1), in.add(depth.p(), (size_t)R * npix, 8),
                                              in.add(views.p(), (size_t)R * (1 + S), 4), in.add(P.p(), n_frames, 96),
                                              in.add(agree.p(), (size_t)R * npix, 4, 0, agree.p() != nullptr),
                                              in.add(rgba8.p(), (size_t)n_frames * npix, 4, 0, rgba8.p() != nullptr)},
                                         {in_sec(max1(ni) * 24, xyz.bytes()), in_sec(max1(ni) * 8, src.bytes()), in_sec(r * npix * 8, depth.bytes()),
                                          in_sec(r * (1 + S) * 4, views.bytes()), in_sec(nf * 96, P.bytes()),
                                          in_sec(r * npix * 4, agree.bytes(), has_agree), in_sec(nf * npix * 4, rgba8.bytes(), has_rgba8)});
                                const size_t nv = cap, nt = cap_t;
                                const int o_r = out.add(report, 8, 4, 64);
                                const MeshOut o = mesh_out(out, nv, nt);
                                check_out(out, {o_r, o.xyz, o.normal, o.rgba8, o.info, o.tri},
                                          {out_sec(256, report, 32), out_sec((nv + 1) * 24, nullptr, 0), out_sec((nv + 1) * 12, nullptr, 0),
                                           out_sec((nv + 1) * 4, nullptr, 0), out_sec((nv + 1) * 16, nullptr, 0), out_sec((nt + 1) * 12, nullptr, 0)});
                            }
                            report_first(out, report, 32);
                        }
}

// kind 18: pgx_mesh_clean (vertex_map, comp out optional), 19: pgx_mesh_decimate (vertex_map, level): the same lists, mesh_in and
// behind the report and the two per-vertex maps mesh_out
void mesh_list_form()
{
    for (int n : {0, 1, 7})
        for (int t : {0, 1, 5})
            for (int mv : {0, 1, 9})          // max_out_vertices: none, one, more than there are vertices
                for (int mt : {0, 1, 11})     // max_out_tris
                    for (int optional = 0; optional < 4; optional++) {
                        const size_t nv = n, nt = t, cv = mv, ct = mt;
                        Src<double> xyz(nv * 3, 1);
                        Src<float> normal(nv * 3, 2);
                        Src<uint32_t> rgba8(nv, 3);
                        Src<int32_t> info(nv * 4, 4), tri(nt * 3, 5);
                        int32_t w[8];
                        std::vector<int32_t> vm(optional & 1 ? nv : 0), aux(optional & 2 ? nv : 0);
                        // a null map is an absent one; at n = 0 a present one is a destination that nothing goes to
                        int32_t *const report = w, *const vertex_map = optional & 1 ? (nv ? vm.data() : w + 1) : nullptr,
                                       *const per_vertex = optional & 2 ? (nv ? aux.data() : w + 2) : nullptr;
                        HostImage in, out;
                        const MeshIn i = mesh_in(in, xyz.p(), normal.p(), rgba8.p(), info.p(), tri.p(), nv, nt);
                        check_in(in, {i.xyz, i.normal, i.rgba8, i.info, i.tri},
                                 {in_sec(max1(nv) * 24, xyz.bytes()), in_sec(max1(nv) * 12, normal.bytes()), in_sec(max1(nv) * 4, rgba8.bytes()),
                                  in_sec(max1(nv) * 16, info.bytes()), in_sec(max1(nt) * 12, tri.bytes())});
                        const MeshList di = mesh_dev(in, i);
                        CHECK(di.xyz == in.dev<double>(i.xyz) && di.normal == in.dev<float>(i.normal) && di.rgba8 == in.dev<uint32_t>(i.rgba8) &&
                              di.info == in.dev<int32_t>(i.info) && di.tri == in.dev<int32_t>(i.tri));
                        const int o_r = out.add(report, 8, 4, 64), o_vm = out.add(vertex_map, nv, 4, 1, vertex_map != nullptr),
                                  o_pv = out.add(per_vertex, nv, 4, 1, per_vertex != nullptr);
                        const MeshOut o = mesh_out(out, cv, ct);
                        check_out(out, {o_r, o_vm, o_pv, o.xyz, o.normal, o.rgba8, o.info, o.tri},
                                  {out_sec(256, report, 32), out_sec(max1(nv) * 4, vertex_map, nv * 4, vertex_map != nullptr),
                                   out_sec(max1(nv) * 4, per_vertex, nv * 4, per_vertex != nullptr), out_sec((cv + 1) * 24, nullptr, 0),
                                   out_sec((cv + 1) * 12, nullptr, 0), out_sec((cv + 1) * 4, nullptr, 0), out_sec((cv + 1) * 16, nullptr, 0),
                                   out_sec((ct + 1) * 12, nullptr, 0)});
                        const MeshRows dr = mesh_dev(out, o);
                        CHECK(dr.xyz == out.dev<double>(o.xyz) && dr.normal == out.dev<float>(o.normal) && dr.rgba8 == out.dev<uint32_t>(o.rgba8) &&
                              dr.info == out.dev<int32_t>(o.info) && dr.tri == out.dev<int32_t>(o.tri));
                        report_first(out, report, 32);
                    }
}

// sources declared out of order (no form does that): pack() still zeroes every byte that none of them covers
void out_of_order()
{
    Src<int32_t> a(3, 1), b(2, 2);
    HostImage in;
    const int s = in.add(nullptr, 0, 4, 100);
    in.put_at(200, a.p(), 12);
    in.put_at(40, b.p(), 8);
    Bytes naive;
    place(naive, 40, b.bytes());
    place(naive, 200, a.bytes());
    check_in(in, {s}, {in_sec(400, naive)});
    CHECK(!in.ascending);
}

} // namespace

int main(int argc, char **argv)
{
    static const char *const FORMS[20] = {"triangulate_tracks", "bundle_adjust", "register_frames", "verify_pair", "relative_pose",
                                          "match", "knn", "knn_guided", "match_batch", "track_consensus", "vocab_train", "select_pairs",
                                          "depth_maps", "depth_fuse", "dense_views", "rgba8_batch", "cloud_merge", "mesh", "mesh_clean",
                                          "mesh_decimate"};
    int kind = -1;
    for (int k = 0; k < 20; k++)
        if (argc == 2 && argv[1] == std::string(FORMS[k])) kind = k;
    if (kind < 0) return 2;
    out_of_order();
    if (kind < 3 || kind == 9) tracks_form(kind);
    else if (kind < 5) pair_form(kind);
    else if (kind < 8) two_sets_form(kind);
    else if (kind == 8) batch_form();
    else if (kind < 12) vocab_form(kind);
    else if (kind < 14) depth_form(kind);
    else if (kind == 14) dense_views_form();
    else if (kind == 15) rgba8_form();
    else if (kind < 18) cloud_form(kind);
    else mesh_list_form();
    std::printf("ok %d\n", n_checks);
    return 0;
}
