// k_vocab.hip -- image retrieval on a binary visual vocabulary (include/pgx.h: pgx_vocab_quantize_dev, pgx_vocab_train_dev,
// pgx_select_pairs_dev): which image pairs of an unordered collection are worth matching.
//
// The quantiser (k_vocab_fp4) is the exact Hamming argmin on the FP4 matrix instruction: the rows are the valid descriptors of
// one slot, the columns are the vocabulary, a buffer of its own, and the work is fp4_nn_block<1, false, VOC_RT> (pgx_fp4_nn.h),
// the body of k_knn_fp4 (k_knn.hip): the nearest word of a row is the k = 1 nearest column, ties to the smaller word.
//
// Training (k-majority) and the pair selection are integer kernels around it; every sum is an integer sum, so no order of
// evaluation changes a bit of the result:
//   k_voc_slots        one workgroup: the exclusive scan of the clamped counts (rank of a slot's first descriptor), N and Fv
//   k_voc_train_init   word j <- the descriptor of rank r_j
//   k_voc_hist         members per word (one atomic per descriptor)
//   k_voc_scan_words   one workgroup: the exclusive scan of the member counts, the scatter cursors
//   k_voc_scatter      the descriptors grouped by word (counting sort; the order inside a group is free)
//   k_voc_update       one wave per word: lane l sums bits 4l .. 4l + 3 over the members, majority with "tie keeps the old bit"
//   k_sel_hist         uint16 word histograms [F][V] (two per 32-bit atomic add; a count is at most 65535)
//   k_sel_weights      per word: df, the weight q
//   k_sel_self         per slot: self score
//   k_sel_scores       16 x 16 slot pairs per workgroup (upper triangle) over a range of words, histogram tiles of 256 words
//                      staged in LDS, the raw min-plus sums added up in int64; k_sel_norm: the normalised matrix, mirrored
//   k_sel_topk         per slot: the key of its top_k-th candidate, found bit by bit on (score << 12 | 4095 - b) keys in LDS
//   k_sel_count / _scan / _write / _fill   the selected pairs compacted in (a, b) order
#include "pgx_fp4_nn.h"
#include "pgx_block.h"       // block_scan_array, block_sum_i, block_sum_ll, block_excl_scan, gsum_i
#include "pgx_hoststage.h"   // WsCarver
#include "pgx_ransac.h"      // splitmix64

#include <climits>

namespace {

constexpr int VOC_RT = 2;                       // row tiles per wavefront
constexpr int VOC_BM = 4 * VOC_RT * 32;         // rows per workgroup
constexpr int SEL_T = 16;                       // slots per side of a score tile
constexpr int SEL_WC = 256;                     // words per staged histogram chunk
constexpr int SEL_PAD = SEL_WC + 2;             // row pitch in uint16: 129 dwords, so 16 rows fall into 16 different banks
constexpr int SEL_MAXF = 4096;

// ---- the quantiser: 256-bit descriptors against V >= 1 words on the FP4 matrix instruction -------------------------------
// out_word / out_dist [F][S]; entries i < clamp(counts[f], 0, S) are written; out_dist may be null.  Held to 240 registers and
// two waves per SIMD like k_knn_fp4 (tests/test_vocab_codegen.py pins it on the code object).
__attribute__((amdgpu_num_vgpr(120))) __global__ __launch_bounds__(256, 2) void k_vocab_fp4(
    const uint32_t *__restrict__ desc, const int32_t *__restrict__ counts, int S, int nrb, int F, const uint32_t *__restrict__ vocab,
    int V, int32_t *__restrict__ out_word, int32_t *__restrict__ out_dist)
{
    int f, bx;
    pgx_xcd_map(blockIdx.x, nrb, F, f, bx);
    const int n1 = pgx_clamp_count(counts[f], S);
    const int rb = bx * VOC_BM;
    if (rb >= n1) return;
    fp4_nn_block<1, false, VOC_RT>(desc + (size_t)f * S * 8, n1, vocab, 0, V, rb, out_word + (size_t)f * S,
                                   out_dist ? out_dist + (size_t)f * S : nullptr, nullptr);
}

// ---- scans ------------------------------------------------------------------------------------------------------------------

// one workgroup of 256: out[i] = in[0] + .. + in[i - 1] for i <= n (out may be in); clamp_to >= 0 clamps the inputs to [0, clamp_to]
__device__ __forceinline__ void scan_array(const int32_t *in, int32_t *out, int n, int clamp_to, int *sh)
{
    const int carry = block_scan_array<int, 256>(
        n, sh, [&](int i) { return clamp_to >= 0 ? pgx_clamp_count(in[i], clamp_to) : in[i]; }, [&](int i, int v) { out[i] = v; });
    if (threadIdx.x == 0) out[n] = carry;
}

// meta: [0] N, [1] Fv, [2] smallest nominated score (INT_MAX: none), [3] pairs by the window alone, [4] words with df == 0,
// [5] words with df == Fv
__global__ __launch_bounds__(256) void k_voc_slots(const int32_t *__restrict__ counts, int F, int S, int32_t *__restrict__ off,
                                                   int32_t *__restrict__ meta)
{
    __shared__ int sh[4];
    scan_array(counts, off, F, S, sh);
    int fv = 0;
    for (int f = threadIdx.x; f < F; f += 256) fv += counts[f] > 0;
    fv = block_sum_i(fv, sh);
    __syncthreads();
    if (threadIdx.x == 0) {
        meta[0] = off[F];
        meta[1] = fv;
        meta[2] = INT_MAX;
        meta[3] = meta[4] = meta[5] = 0;
    }
}

// ---- training ---------------------------------------------------------------------------------------------------------------

__global__ __launch_bounds__(256) void k_voc_train_init(const uint32_t *__restrict__ desc, const int32_t *__restrict__ off, int F, int S,
                                                        int V, uint64_t seed, uint32_t *__restrict__ vocab, int32_t *__restrict__ report,
                                                        int *status)
{
    const int N = off[F];
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j == 0) {
        report[0] = N;
        report[1] = report[2] = -1;
        report[3] = 0;
        if (N < V) atomicOr(status, (int)PGX_ST_VOC_FEW);
    }
    if (N < V || j >= V) return;
    const uint64_t lo = (uint64_t)j * (uint64_t)N / (uint64_t)V, hi = (uint64_t)(j + 1) * (uint64_t)N / (uint64_t)V; // hi > lo: N >= V
    uint64_t st = seed ^ (uint64_t)j * 0xD1B54A32D192ED03ull;
    const int rk = (int)(lo + splitmix64(st) % (hi - lo));
    int a = 0, b = F; // the last slot whose first rank is <= rk: the one that holds it (empty slots before it share its offset)
    while (b - a > 1) {
        const int mid = (a + b) >> 1;
        if (off[mid] <= rk) a = mid;
        else b = mid;
    }
    const uint32_t *src = desc + ((size_t)a * S + (rk - off[a])) * 8;
    const uint4 x = *reinterpret_cast<const uint4 *>(src), y = *reinterpret_cast<const uint4 *>(src + 4);
    *reinterpret_cast<uint4 *>(vocab + (size_t)j * 8) = x;
    *reinterpret_cast<uint4 *>(vocab + (size_t)j * 8 + 4) = y;
}

// members per word: cnt[word] += 1 for every valid descriptor
__global__ __launch_bounds__(256) void k_voc_hist(const int32_t *__restrict__ counts, int F, int S, const int32_t *__restrict__ word,
                                                  int32_t *__restrict__ cnt)
{
    const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
    const int f = (int)(idx / S), i = (int)(idx % S);
    if (f < F && i < pgx_clamp_count(counts[f], S)) atomicAdd(&cnt[word[idx]], 1);
}

// start[j] = members of the words before j (start [V + 1], in place over the counts); cursor = start; the two counters of the
// iteration's report are cleared
__global__ __launch_bounds__(256) void k_voc_scan_words(int32_t *__restrict__ start, int32_t *__restrict__ cursor, int V,
                                                        int32_t *__restrict__ report)
{
    __shared__ int sh[4];
    scan_array(start, start, V, -1, sh);
    __syncthreads();
    for (int j = threadIdx.x; j < V; j += 256) cursor[j] = start[j];
    if (threadIdx.x == 0) report[1] = report[2] = 0;
}

__global__ __launch_bounds__(256) void k_voc_scatter(const int32_t *__restrict__ counts, int F, int S, const int32_t *__restrict__ word,
                                                     int32_t *__restrict__ cursor, uint32_t *__restrict__ member)
{
    const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
    const int f = (int)(idx / S), i = (int)(idx % S);
    if (f < F && i < pgx_clamp_count(counts[f], S)) member[atomicAdd(&cursor[word[idx]], 1)] = (uint32_t)idx;
}

// one wave per word: lane l owns bits 4l .. 4l + 3 (bits (l & 7) * 4 .. + 3 of word l >> 3)
__global__ __launch_bounds__(256) void k_voc_update(const uint32_t *__restrict__ desc, const int32_t *__restrict__ off, int F,
                                                    const int32_t *__restrict__ start, const uint32_t *__restrict__ member, int V,
                                                    uint32_t *__restrict__ vocab, int32_t *__restrict__ report)
{
    if (off[F] < V) return; // PGX_ST_VOC_FEW: d_vocab stays as it is
    const int j = blockIdx.x * 4 + (threadIdx.x >> 6), l = threadIdx.x & 63;
    if (j >= V) return;
    const int s0 = start[j], c = start[j + 1] - s0, wi = l >> 3, sh = (l & 7) * 4;
    int ones[4] = {0, 0, 0, 0};
    for (int m = 0; m < c; m++) {
        const uint32_t nib = desc[(size_t)member[s0 + m] * 8 + wi] >> sh;
#pragma unroll
        for (int k = 0; k < 4; k++) ones[k] += (int)((nib >> k) & 1u);
    }
    const uint32_t oldn = (vocab[(size_t)j * 8 + wi] >> sh) & 15u;
    uint32_t newn = 0;
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const uint32_t ob = (oldn >> k) & 1u;
        newn |= (2 * ones[k] > c ? 1u : (2 * ones[k] < c ? 0u : ob)) << k;
    }
    if (c == 0) newn = oldn;
    const int changed = gsum_i<64>(__popc(newn ^ oldn));
    uint32_t w = newn << sh;
    w |= __shfl_xor(w, 1, 64);
    w |= __shfl_xor(w, 2, 64);
    w |= __shfl_xor(w, 4, 64);
    if ((l & 7) == 0) vocab[(size_t)j * 8 + wi] = w;
    if (l == 0) {
        if (c == 0) atomicAdd(&report[1], 1);
        if (changed) atomicAdd(&report[2], changed);
    }
}

// ---- pair selection ---------------------------------------------------------------------------------------------------------

struct SelArgs {
    const int32_t *counts;
    int F, S, V, Vp;          // Vp: uint16 entries per histogram row (V rounded up to even)
    int weighting, top_k, window, min_score, max_pairs;
    const int32_t *word;      // [F][S]
    uint32_t *hist;           // [F][Vp / 2] two uint16 counts per word
    int32_t *q;               // [V]
    long long *self;          // [F]
    unsigned long long *sraw; // [F][F] raw scores, entries (a, b) of the tiles with tile(a) <= tile(b)
    int wpb;                  // words per workgroup of k_sel_scores, a multiple of SEL_WC
    int32_t *scores;          // [F][F]
    long long *thr;           // [F] the smallest key a slot nominates
    int32_t *rowoff;          // [F + 1]
    int32_t *meta;            // k_voc_slots'
    int32_t *pairlist, *pair_score, *summary;
    int *status;
};

__device__ __forceinline__ int sel_h(const SelArgs &a, int f, int w)
{
    return (int)reinterpret_cast<const uint16_t *>(a.hist)[(size_t)f * a.Vp + w];
}

__global__ __launch_bounds__(256) void k_sel_hist(SelArgs a)
{
    const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
    const int f = (int)(idx / a.S), i = (int)(idx % a.S);
    if (f >= a.F || i >= pgx_clamp_count(a.counts[f], a.S)) return;
    const size_t e = (size_t)f * a.Vp + a.word[idx];
    atomicAdd(&a.hist[e >> 1], (e & 1) ? 0x10000u : 1u); // no carry between the halves: a count is at most S <= 65535
}

__global__ __launch_bounds__(256) void k_sel_weights(SelArgs a)
{
    const int w = blockIdx.x * 256 + threadIdx.x;
    if (w >= a.V) return;
    int df = 0;
    for (int f = 0; f < a.F; f++) df += sel_h(a, f, w) > 0;
    const int Fv = a.meta[1];
    int q = 1;
    if (a.weighting == 1) {
        q = 0;
        if (df > 0) {
            const uint64_t x = ((uint64_t)Fv << 16) / (uint64_t)df; // >= 2^16: df <= Fv
            const int e = 63 - __clzll((long long)x);
            q = 256 * (e - 16) + (int)((x << 8) >> e) - 256;
        }
    }
    a.q[w] = q;
    if (df == 0) atomicAdd(&a.meta[4], 1);
    if (df == Fv) atomicAdd(&a.meta[5], 1);
}

__global__ __launch_bounds__(256) void k_sel_self(SelArgs a)
{
    __shared__ long long sh[4];
    const int f = blockIdx.x;
    long long s = 0;
    for (int w = threadIdx.x; w < a.V; w += 256) s += (long long)a.q[w] * sel_h(a, f, w);
    s = block_sum_ll(s, sh);
    if (threadIdx.x == 0) a.self[f] = s;
}

// workgroup (bx, by, bz), bx >= by: the raw scores of slots a = by * 16 + ty against b = bx * 16 + tx over the words
// [bz * wpb, (bz + 1) * wpb), added to sraw[a][b] (integers: the order of the adds does not matter)
__global__ __launch_bounds__(256) void k_sel_scores(SelArgs a)
{
    __shared__ uint16_t ha[SEL_T][SEL_PAD], hb[SEL_T][SEL_PAD];
    __shared__ int32_t qs[SEL_WC];
    if (blockIdx.x < blockIdx.y) return;
    const int tx = threadIdx.x & 15, ty = threadIdx.x >> 4, a0 = blockIdx.y * SEL_T, b0 = blockIdx.x * SEL_T;
    const int wbeg = blockIdx.z * a.wpb, wend = wbeg + a.wpb < a.V ? wbeg + a.wpb : a.V;
    const uint16_t *H = reinterpret_cast<const uint16_t *>(a.hist);
    long long s = 0;
    for (int w0 = wbeg; w0 < wend; w0 += SEL_WC) {
        __syncthreads(); // the tiles of the chunk before are read
        for (int e = threadIdx.x; e < SEL_T * SEL_WC; e += 256) {
            const int rr = e / SEL_WC, c = e % SEL_WC;
            const bool in = w0 + c < wend;
            ha[rr][c] = in && a0 + rr < a.F ? H[(size_t)(a0 + rr) * a.Vp + w0 + c] : (uint16_t)0;
            hb[rr][c] = in && b0 + rr < a.F ? H[(size_t)(b0 + rr) * a.Vp + w0 + c] : (uint16_t)0;
        }
        qs[threadIdx.x] = w0 + threadIdx.x < wend ? a.q[w0 + threadIdx.x] : 0;
        __syncthreads();
#pragma unroll 8
        for (int c = 0; c < SEL_WC; c++) s += (long long)(qs[c] * min((int)ha[ty][c], (int)hb[tx][c])); // < 2^31: q < 2^12, h < 2^16
    }
    const int sa = a0 + ty, sb = b0 + tx;
    if (sa < a.F && sb < a.F && s != 0) atomicAdd(&a.sraw[(size_t)sa * a.F + sb], (unsigned long long)s);
}

// d_scores from the raw scores: entry (sa, sb) reads the raw score of (min, max), which the tile of that order holds
__global__ __launch_bounds__(256) void k_sel_norm(SelArgs a)
{
    const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (long long)a.F * a.F) return;
    const int sa = (int)(idx / a.F), sb = (int)(idx % a.F);
    int sc = -1;
    if (sa != sb && a.counts[sa] > 0 && a.counts[sb] > 0) {
        const long long s = (long long)a.sraw[(size_t)(sa < sb ? sa : sb) * a.F + (sa < sb ? sb : sa)];
        const long long fa = a.self[sa], fb = a.self[sb], mn = fa < fb ? fa : fb;
        sc = (int)((s << 20) / (mn > 1 ? mn : 1));
    }
    a.scores[idx] = sc;
}

__device__ __forceinline__ long long sel_key(int sc, int b) { return ((long long)sc << 12) | (long long)(4095 - b); }

// slot a nominates b: a candidate (a score, at least min_score) among the first top_k in (score descending, b ascending) order
__device__ __forceinline__ bool sel_nominates(const SelArgs &a, int sa, int sb)
{
    const int sc = a.scores[(size_t)sa * a.F + sb];
    return sc >= 0 && sc >= a.min_score && sel_key(sc, sb) >= a.thr[sa];
}

__global__ __launch_bounds__(256) void k_sel_topk(SelArgs a)
{
    __shared__ long long key[SEL_MAXF];
    __shared__ int sh[4];
    const int sa = blockIdx.x;
    int ncand = 0;
    for (int b = threadIdx.x; b < a.F; b += 256) {
        const int sc = a.scores[(size_t)sa * a.F + b];
        const bool cand = sc >= 0 && sc >= a.min_score; // the diagonal and empty slots hold -1
        key[b] = cand ? sel_key(sc, b) : -1;
        ncand += cand;
    }
    __syncthreads();
    ncand = block_sum_i(ncand, sh);
    long long T = 0; // every candidate
    if (a.top_k == 0) T = LLONG_MAX;
    else if (ncand > a.top_k) {
        // the top_k-th largest key: the largest T with at least top_k keys >= T, bit by bit (keys are distinct and below 2^33)
        for (int bit = 32; bit >= 0; bit--) {
            const long long t = T | (1ll << bit);
            int n = 0;
            for (int b = threadIdx.x; b < a.F; b += 256) n += key[b] >= t;
            if (block_sum_i(n, sh) >= a.top_k) T = t;
        }
    }
    if (threadIdx.x == 0) a.thr[sa] = T;
}

// pair (sa, sb), sa < sb: 0 not selected, 1 selected by a nomination, 2 selected by the window alone
__device__ __forceinline__ int sel_state(const SelArgs &a, int sa, int sb, int &sc)
{
    sc = a.scores[(size_t)sa * a.F + sb];
    if (sc < 0) return 0; // an empty slot
    if (sel_nominates(a, sa, sb) || sel_nominates(a, sb, sa)) return 1;
    return sb - sa <= a.window ? 2 : 0;
}

__global__ __launch_bounds__(256) void k_sel_count(SelArgs a)
{
    __shared__ int sh[4];
    const int sa = blockIdx.x;
    int n = 0, nw = 0, mn = INT_MAX;
    for (int sb = sa + 1 + threadIdx.x; sb < a.F; sb += 256) {
        int sc;
        const int st = sel_state(a, sa, sb, sc);
        n += st != 0;
        nw += st == 2;
        if (st == 1) mn = min(mn, sc);
    }
    n = block_sum_i(n, sh);
    nw = block_sum_i(nw, sh);
#pragma unroll
    for (int m = 1; m < 64; m <<= 1) mn = min(mn, __shfl_xor(mn, m, 64));
    if (threadIdx.x == 0) {
        a.rowoff[sa] = n;
        if (nw) atomicAdd(&a.meta[3], nw);
    }
    if ((threadIdx.x & 63) == 0 && mn != INT_MAX) atomicMin(&a.meta[2], mn);
}

__global__ __launch_bounds__(256) void k_sel_scan(SelArgs a)
{
    __shared__ int sh[4];
    scan_array(a.rowoff, a.rowoff, a.F, -1, sh);
    __syncthreads();
    if (threadIdx.x == 0) {
        const int total = a.rowoff[a.F];
        a.summary[0] = total;
        a.summary[1] = a.meta[1];
        a.summary[2] = a.meta[4];
        a.summary[3] = a.meta[5];
        a.summary[4] = a.meta[3];
        a.summary[5] = a.meta[2] == INT_MAX ? -1 : a.meta[2];
        a.summary[6] = a.summary[7] = 0;
        if (total > a.max_pairs) atomicOr(a.status, (int)PGX_ST_SEL_CAP);
    }
}

__global__ __launch_bounds__(256) void k_sel_write(SelArgs a)
{
    __shared__ int sh[4];
    const int sa = blockIdx.x;
    int at = a.rowoff[sa];
    for (int b0 = sa + 1; b0 < a.F; b0 += 256) { // uniform trip count: the scan has barriers
        const int sb = b0 + threadIdx.x;
        int sc = -1;
        const int on = sb < a.F && sel_state(a, sa, sb, sc) != 0;
        int tot;
        const int p = at + block_excl_scan<int, 256>(on, sh, tot);
        if (on && p < a.max_pairs) {
            a.pairlist[2 * (size_t)p] = sa;
            a.pairlist[2 * (size_t)p + 1] = sb;
            a.pair_score[p] = sc;
        }
        at += tot;
    }
}

__global__ __launch_bounds__(256) void k_sel_fill(SelArgs a)
{
    const int p = blockIdx.x * 256 + threadIdx.x;
    if (p < a.max_pairs && p >= a.rowoff[a.F]) {
        a.pairlist[2 * (size_t)p] = a.pairlist[2 * (size_t)p + 1] = -1;
        a.pair_score[p] = -1;
    }
}

unsigned slot_blocks(int F, int S) { return (unsigned)(((long long)F * S + 255) / 256); }

struct TrainWs {
    int32_t *word, *off, *meta, *start, *cursor;
    uint32_t *member;
};
TrainWs carve_train(WsCarver &w, int F, int S, int V)
{
    TrainWs t;
    t.word = w.take<int32_t>((size_t)F * S * 4);
    t.member = w.take<uint32_t>((size_t)F * S * 4);
    t.off = w.take<int32_t>((size_t)(F + 1) * 4);
    t.meta = w.take<int32_t>(64);
    t.start = w.take<int32_t>((size_t)(V + 1) * 4);
    t.cursor = w.take<int32_t>((size_t)V * 4);
    return t;
}

struct SelWs {
    SelArgs a;
    int32_t *off;
    size_t hist_bytes;
};
SelWs carve_select(WsCarver &w, int F, int S, int V, bool own_scores)
{
    SelWs s{};
    s.a.Vp = (V + 1) & ~1;
    s.hist_bytes = (size_t)F * s.a.Vp * 2;
    int32_t *word = w.take<int32_t>((size_t)F * S * 4);
    s.a.word = word;
    s.a.hist = w.take<uint32_t>(s.hist_bytes);
    s.a.q = w.take<int32_t>((size_t)V * 4);
    s.a.self = w.take<long long>((size_t)F * 8);
    s.a.thr = w.take<long long>((size_t)F * 8);
    s.a.rowoff = w.take<int32_t>((size_t)(F + 1) * 4);
    s.off = w.take<int32_t>((size_t)(F + 1) * 4);
    s.a.meta = w.take<int32_t>(64);
    s.a.sraw = w.take<unsigned long long>((size_t)F * F * 8);
    s.a.scores = own_scores ? w.take<int32_t>((size_t)F * F * 4) : nullptr;
    return s;
}

} // namespace

void pgx_launch_vocab_quantize(pgx_ctx *ctx, hipStream_t s, const uint32_t *d_desc, const int32_t *d_counts, int F, int S,
                               const uint32_t *d_vocab, int V, int32_t *d_word, int32_t *d_wdist)
{
    const int nrb = (S + VOC_BM - 1) / VOC_BM;
    ProfScope ps(ctx, "vocab_quantize", s);
    hipLaunchKernelGGL(k_vocab_fp4, dim3((unsigned)nrb * (unsigned)F), dim3(256), 0, s, d_desc, d_counts, S, nrb, F, d_vocab, V, d_word,
                       d_wdist);
}

size_t pgx_vocab_train_ws_bytes(int F, int S, int V)
{
    WsCarver w(nullptr);
    carve_train(w, F, S, V);
    return w.total();
}

void pgx_launch_vocab_train(pgx_ctx *ctx, hipStream_t s, const uint32_t *d_desc, const int32_t *d_counts, int F, int S, int V, int iters,
                            uint64_t seed, uint32_t *d_vocab, int32_t *d_report, void *ws, int *status)
{
    WsCarver w(ws);
    const TrainWs t = carve_train(w, F, S, V);
    {
        ProfScope ps(ctx, "vocab_train_init", s);
        hipLaunchKernelGGL(k_voc_slots, dim3(1), dim3(256), 0, s, d_counts, F, S, t.off, t.meta);
        hipLaunchKernelGGL(k_voc_train_init, dim3((V + 255) / 256), dim3(256), 0, s, d_desc, t.off, F, S, V, seed, d_vocab, d_report, status);
    }
    for (int it = 0; it < iters; it++) {
        pgx_launch_vocab_quantize(ctx, s, d_desc, d_counts, F, S, d_vocab, V, t.word, nullptr);
        ProfScope ps(ctx, "vocab_train_update", s);
        (void)hipMemsetAsync(t.start, 0, (size_t)(V + 1) * 4, s);
        hipLaunchKernelGGL(k_voc_hist, dim3(slot_blocks(F, S)), dim3(256), 0, s, d_counts, F, S, t.word, t.start);
        hipLaunchKernelGGL(k_voc_scan_words, dim3(1), dim3(256), 0, s, t.start, t.cursor, V, d_report);
        hipLaunchKernelGGL(k_voc_scatter, dim3(slot_blocks(F, S)), dim3(256), 0, s, d_counts, F, S, t.word, t.cursor, t.member);
        hipLaunchKernelGGL(k_voc_update, dim3((V + 3) / 4), dim3(256), 0, s, d_desc, t.off, F, t.start, t.member, V, d_vocab, d_report);
    }
}

size_t pgx_select_pairs_ws_bytes(int F, int S, int V, bool own_scores)
{
    WsCarver w(nullptr);
    carve_select(w, F, S, V, own_scores);
    return w.total();
}

void pgx_launch_select_pairs(pgx_ctx *ctx, hipStream_t s, const uint32_t *d_desc, const int32_t *d_counts, int F, int S,
                             const uint32_t *d_vocab, int V, int weighting, int top_k, int window, int min_score, int max_pairs,
                             int32_t *d_pairlist, int32_t *d_pair_score, int32_t *d_scores, int32_t *d_summary, void *ws, int *status)
{
    WsCarver w(ws);
    SelWs sw = carve_select(w, F, S, V, d_scores == nullptr);
    SelArgs &a = sw.a;
    a.counts = d_counts;
    a.F = F; a.S = S; a.V = V;
    a.weighting = weighting; a.top_k = top_k; a.window = window; a.min_score = min_score; a.max_pairs = max_pairs;
    if (d_scores) a.scores = d_scores;
    a.pairlist = d_pairlist; a.pair_score = d_pair_score; a.summary = d_summary;
    a.status = status;
    pgx_launch_vocab_quantize(ctx, s, d_desc, d_counts, F, S, d_vocab, V, const_cast<int32_t *>(a.word), nullptr);
    const unsigned T = (unsigned)((F + SEL_T - 1) / SEL_T);
    {
        ProfScope ps(ctx, "select_hist", s);
        hipLaunchKernelGGL(k_voc_slots, dim3(1), dim3(256), 0, s, d_counts, F, S, sw.off, a.meta);
        (void)hipMemsetAsync(a.hist, 0, sw.hist_bytes, s);
        hipLaunchKernelGGL(k_sel_hist, dim3(slot_blocks(F, S)), dim3(256), 0, s, a);
        hipLaunchKernelGGL(k_sel_weights, dim3((V + 255) / 256), dim3(256), 0, s, a);
        hipLaunchKernelGGL(k_sel_self, dim3(F), dim3(256), 0, s, a);
    }
    {
        // the words are split over enough workgroups to fill the device when there are few slot tiles (about 2048 in all)
        const unsigned tri = T * (T + 1) / 2, chunks = (unsigned)((V + SEL_WC - 1) / SEL_WC);
        const unsigned want = 2048 / tri > 0 ? 2048 / tri : 1, nz0 = want < chunks ? want : chunks;
        a.wpb = (int)((chunks + nz0 - 1) / nz0) * SEL_WC;
        const unsigned nz = (unsigned)((V + a.wpb - 1) / a.wpb);
        ProfScope ps(ctx, "select_scores", s);
        (void)hipMemsetAsync(a.sraw, 0, (size_t)F * F * 8, s);
        hipLaunchKernelGGL(k_sel_scores, dim3(T, T, nz), dim3(256), 0, s, a);
        hipLaunchKernelGGL(k_sel_norm, dim3((unsigned)(((long long)F * F + 255) / 256)), dim3(256), 0, s, a);
    }
    {
        ProfScope ps(ctx, "select_pick", s);
        hipLaunchKernelGGL(k_sel_topk, dim3(F), dim3(256), 0, s, a);
        hipLaunchKernelGGL(k_sel_count, dim3(F), dim3(256), 0, s, a);
        hipLaunchKernelGGL(k_sel_scan, dim3(1), dim3(256), 0, s, a);
        hipLaunchKernelGGL(k_sel_write, dim3(F), dim3(256), 0, s, a);
        if (max_pairs > 0) hipLaunchKernelGGL(k_sel_fill, dim3((max_pairs + 255) / 256), dim3(256), 0, s, a);
    }
}
