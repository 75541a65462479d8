// Stand-alone driver of the host forms' staging images (photogrammetry_amd/csrc/pgx_hoststage.h) for tests/test_hoststage.py:
// argv[1] names a host form, whose section lists are checked at every size of the test's docstring against images laid out
// naively here.  The input lists are the header's own (tracks_in, pair_in); the output lists, and F and K of
// pgx_relative_pose, are declared here word for word as the form in pgx_api.hip declares them.  Host code only; the test
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

// kind 0: triangulation, 1: bundle adjustment, 2: registration
void tracks_form(int kind)
{
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
                    const TracksIn i = kind == 0 ? tracks_in(in, t, {P.p(), nullptr, nullptr}, {96, 0, 0}, false, nullptr, nullptr)
                                                 : tracks_in(in, t, {K.p(), Rt.p(), sel.p()}, {32, 96, 4}, true, xyz.p(), flags.p());
                    if (kind == 0)
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

} // namespace

int main(int argc, char **argv)
{
    static const char *const FORMS[5] = {"triangulate_tracks", "bundle_adjust", "register_frames", "verify_pair", "relative_pose"};
    int kind = -1;
    for (int k = 0; k < 5; k++)
        if (argc == 2 && argv[1] == std::string(FORMS[k])) kind = k;
    if (kind < 0) return 2;
    kind < 3 ? tracks_form(kind) : pair_form(kind);
    std::printf("ok %d\n", n_checks);
    return 0;
}
