"""The helpers and cases of tests/pairs_limits_cases.py are what tests/test_gpu_vocab_limits.py, tests/test_gpu_select_limits.py and
tests/test_gpu_consensus_limits.py take them for (no GPU): the restated launch rules equal the text of csrc/k_vocab.hip,
csrc/pgx_fp4.h, csrc/pgx_internal.h and csrc/k_consensus.hip; every shape the GPU tests use reaches the path it is named for;
and the tiled consensus yardstick equals tests/consensus_ref.py on a short graph and on the whole one, bit for bit, exhaustive
and sampled."""
import os
import re

import numpy as np
import pytest

import consensus_ref as cref
import pairs_limits_cases as pc
import pairs_ref as R

CSRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "photogrammetry_amd", "csrc")


def source(name):
    return open(os.path.join(CSRC, name)).read()


def constants(text):
    vals = {}
    for name, expr in re.findall(r"^constexpr int (\w+) = ([^;]+);", text, flags=re.M):
        if re.fullmatch(r"[\w\s<*+()-]+", expr) and all(w in vals for w in re.findall(r"[A-Za-z_]\w*", expr)):
            vals[name] = eval(expr, {}, dict(vals))
    return vals


# ---- the mirrored launch facts -----------------------------------------------------------------------------------------------------

def test_constants_and_rules_equal_the_kernel_sources():
    voc = source("k_vocab.hip")
    v = constants(voc)
    assert (v["VOC_BM"], v["SEL_T"], v["SEL_WC"], v["SEL_MAXF"]) == (pc.VOC_BM, pc.SEL_T, pc.SEL_WC, pc.SEL_MAXF)
    assert constants(source("pgx_fp4.h"))["F4_CHUNK"] == pc.F4_CHUNK
    # the quantiser's grid and its block map
    assert "const int nrb = (S + VOC_BM - 1) / VOC_BM;" in voc and "dim3((unsigned)nrb * (unsigned)F), dim3(256)" in voc
    assert "pgx_xcd_map(blockIdx.x, nrb, F, f, bx);" in voc and "const int rb = bx * VOC_BM;" in voc and "if (rb >= n1) return;" in voc
    body = re.search(r"void pgx_xcd_map\(int lin, int nblk, int F, int &f, int &b\)\n\{(.*?)\n\}", source("pgx_internal.h"), flags=re.S).group(1)
    for line in ("const int F8 = (F >> 3) << 3;", "if (lin < nblk * F8) {", "const int j = lin >> 3;", "f = (j / nblk) * 8 + (lin & 7);",
                 "b = j % nblk;", "const int r = lin - nblk * F8;", "f = F8 + r / nblk;", "b = r % nblk;"):
        assert line in body, line
    # the scans: 256 values per pass, a carry between the passes; the trainer's search reads the scanned offsets
    block = source("pgx_block.h")
    assert "for (int base = 0; base < n; base += NT) {" in block and "if (j < n) store(j, carry + ex);" in block and "carry += tot;" in block
    assert "block_scan_array<int, %d>(" % pc.SCAN_NT in voc and "[&](int i, int v) { out[i] = v; });" in voc
    assert "if (threadIdx.x == 0) out[n] = carry;" in voc
    assert "scan_array(counts, off, F, S, sh);" in voc and "if (off[mid] <= rk) a = mid;" in voc
    # the histogram's halves
    assert "atomicAdd(&a.hist[e >> 1], (e & 1) ? 0x10000u : 1u);" in voc and "const size_t e = (size_t)f * a.Vp + a.word[idx];" in voc
    assert "s.a.Vp = (V + 1) & ~1;" in voc
    # the split of the words over the score workgroups
    for line in ("const unsigned T = (unsigned)((F + SEL_T - 1) / SEL_T);",
                 "const unsigned tri = T * (T + 1) / 2, chunks = (unsigned)((V + SEL_WC - 1) / SEL_WC);",
                 "const unsigned want = 2048 / tri > 0 ? 2048 / tri : 1, nz0 = want < chunks ? want : chunks;",
                 "a.wpb = (int)((chunks + nz0 - 1) / nz0) * SEL_WC;", "const unsigned nz = (unsigned)((V + a.wpb - 1) / a.wpb);",
                 "dim3(T, T, nz), dim3(256)", "for (int w0 = wbeg; w0 < wend; w0 += SEL_WC) {",
                 "const int wbeg = blockIdx.z * a.wpb, wend = wbeg + a.wpb < a.V ? wbeg + a.wpb : a.V;"):
        assert line in voc, line
    # the threshold search, the write's blocks of 256 and the fill
    assert "for (int bit = 32; bit >= 0; bit--) {" in voc and "else if (ncand > a.top_k) {" in voc
    assert "for (int b0 = sa + 1; b0 < a.F; b0 += 256) {" in voc and "if (on && p < a.max_pairs) {" in voc
    assert "if (max_pairs > 0) hipLaunchKernelGGL(k_sel_fill" in voc
    cns = source("k_consensus.hip")
    c = constants(cns)
    assert (c["CNS_GRID_MAX"], c["CNS_NT"]) == (pc.CNS_GRID_MAX, pc.CNS_NT)
    assert "const long long want = ((long long)max_tracks + 3) / 4;" in cns
    assert "return (int)(want < 1 ? 1 : (want > CNS_GRID_MAX ? CNS_GRID_MAX : want));" in cns
    assert "__device__ __forceinline__ int cns_class(int n) { return n > 32 ? 2 : (n > 8 ? 1 : 0); }" in cns
    for cls, G in pc.CNS_LANES.items():
        assert "(k_cns_score<%d, %d>), dim3(grid), dim3(CNS_NT)" % (G, cls) in cns and "cns_write_phase<%d, %d>(a, nt);" % (G, cls) in cns
    assert "hipLaunchKernelGGL(k_cns_write, dim3(grid), dim3(CNS_NT)" in cns
    tg = source("pgx_trackgraph.h")
    assert "const long long ngroups = (long long)gridDim.x * blockDim.x / (G);" in tg and "t += ngroups)" in tg


def test_restated_rules_at_known_points():
    assert [pc.nrb(s) for s in (1, 256, 257, 512, 513, 65535)] == [1, 1, 2, 2, 3, 256]
    assert pc.score_split(64, 65536)[2:4] == (512, 128)                      # the benched shape of tools/bench_pairs.py
    assert pc.score_split(4096, 16)[1:4] == (1, 256, 1) and pc.score_split(9, 777)[1:4] == (4, 256, 4)
    assert pc.score_split(24, 1024)[1:4] == (4, 256, 4)                        # the older tests: one chunk per workgroup
    assert [pc.cns_grid(n) for n in (0, 1, 4, 5, 4096, 4097, 16400)] == [1, 1, 1, 2, 1024, 1024, 1024]
    assert [pc.second_pass_start(16400, c) for c in (2, 1, 0)] == [4096, 16384, 65536]
    assert [pc.cns_class(n) for n in (2, 8, 9, 32, 33, 65)] == [0, 0, 1, 1, 2, 2]
    assert [pc.scan_passes(n) for n in (1, 256, 257, 600)] == [1, 1, 2, 3]


# ---- the quantiser's shapes ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("F", pc.QUANT_F)
@pytest.mark.parametrize("S", pc.QUANT_S)
def test_block_map_is_a_bijection_and_the_shapes_reach_both_branches(F, S):
    n = pc.nrb(S)
    assert n == {260: 2, 515: 3}[S] and F >= 8
    got = [pc.xcd_map(lin, n, F) for lin in range(n * F)]
    assert sorted(got) == [(f, b) for f in range(F) for b in range(n)]
    counts = pc.quantiser_counts(F, S)
    assert {0, 256, 257}.issubset(counts.tolist()) and (counts < 0).any() and (counts > S).any()
    work = pc.working_blocks(F, S, counts)
    F8 = F & ~7
    assert any(f < F8 and b == n - 1 for f, b in work)                        # the first branch, a row block past the first
    assert F % 8 == 0 or any(f >= F8 and b == n - 1 for f, b in work)         # the else branch, likewise
    assert any((f, 0) not in work for f in range(F))                          # a slot whose workgroups all leave at once
    desc, c2, vocab = pc.quantiser_case(F, S, 33)
    assert desc.shape == (F, S, 8) and (c2 == counts).all() and len({d.tobytes() for d in desc}) == F


def test_stride_limit_case():
    desc, counts, vocab = pc.stride_limit_case()
    assert desc.shape == (3, 65535, 8) and pc.nrb(65535) == 256 and counts.tolist() == [65535, 65281, 70000]
    assert (65281 - 1) // pc.VOC_BM == 255 and 65281 % pc.VOC_BM == 1         # slot 1 ends one row into the last row block
    assert pc.xcd_map(3 * 256 - 1, 256, 3) == (2, 255)                        # F < 8: the else branch alone
    n = R.clamp_counts(counts, 65535)
    for f, i, w in pc.STRIDE_LIMIT_ROWS:
        assert i < n[f] and (desc[f, i] == vocab[w]).all()
    assert {i for f, i, _ in pc.STRIDE_LIMIT_ROWS if f == 0} == {65534, 65279, 65280, 65281}


def test_train_case():
    desc, counts = pc.train_case()
    assert desc.shape == (600, 3, 8) and pc.scan_passes(600) == 3 and counts.min() == 0 and counts.max() == 3
    for a, b in pc.TRAIN_EMPTY:
        assert (counts[a:b] == 0).all() and (a == 0 or counts[a - 1] > 0) and (b == 600 or counts[b] > 0)
    assert pc.TRAIN_EMPTY[0][0] == 0 and pc.TRAIN_EMPTY[1][0] < 256 < pc.TRAIN_EMPTY[1][1] and pc.TRAIN_EMPTY[2][1] == 600
    N = int(counts.sum())
    assert N > 600                                                            # ranks past the first two passes of the scan
    wide, wcounts = pc.restride(desc, counts, 7)
    assert wide.shape == (600, 7, 8) and (wcounts == counts).all() and (R.valid_rows(wide, wcounts) == R.valid_rows(desc, counts)).all()
    assert (wide[:, :3] != desc).any()


# ---- the selection's shapes ---------------------------------------------------------------------------------------------------------

def test_chunk_shapes_reach_the_second_chunk():
    assert pc.score_split(257, 3329) == (153, 14, 512, 7, 257) and pc.score_split(529, 1537) == (595, 7, 768, 3, 1)
    places = {(257, 3329): [(1, 0, 255), (2, 1, 0), (6, 1, 0)], (529, 1537): [(0, 0, 255), (1, 1, 0), (1, 2, 0), (2, 0, 0)]}
    for (F, V), planted in pc.CHUNK_SHAPES.items():
        tri, chunks, wpb, nz, last = pc.score_split(F, V)
        assert wpb > pc.SEL_WC and chunks > 2048 // tri
        assert [pc.chunk_place(w, wpb) for w, _ in planted] == places[(F, V)]
        assert last % pc.SEL_WC == 1                                           # the last chunk of the last slice is one word
        desc, counts, vocab = pc.chunk_collection(F, V)
        bare, bcounts, bvocab = pc.chunk_collection(F, V, with_planted=False)
        assert (vocab == bvocab).all() and desc.shape == (F, pc.CHUNK_STRIDE, 8) and counts.max() <= pc.CHUNK_STRIDE
        h = R.histograms(desc, counts, vocab)
        assert h.sum() == counts.sum() and (counts == 0).sum() == 2           # every descriptor is a word of the vocabulary
        for w, pair in planted:
            assert np.flatnonzero(h[:, w]).tolist() == sorted(pair) and (h[list(pair), w] == pc.CHUNK_COPIES).all()
            assert (bcounts[list(pair)] == counts[list(pair)] - pc.CHUNK_COPIES).all()
        # frames share words in every chunk of every slice
        df = (h > 0).sum(0)
        for c in range(chunks):
            assert (df[c * pc.SEL_WC:(c + 1) * pc.SEL_WC] >= 2).sum() >= (1 if c == chunks - 1 else 20), c


def test_halves_cases():
    assert pc.half_of(0, 6, 3) == (1, 1) and pc.half_of(1, 6, 2) == (4, 0) and pc.half_of(0, 6, 2) == (1, 0)
    assert pc.half_of(0, 7, 6) == (3, 0) and pc.half_of(1, 7, 5) == (6, 1) and pc.half_of(0, 7, 7)[0] == 3   # 7: the padding
    for V, w0, w1 in pc.HALVES:
        desc, counts, vocab = pc.halves_case(V, w0, w1)
        h = R.histograms(desc, counts, vocab)
        assert h[0, w0] == 65535 == h[1, w1] and h[0].sum() == 65535 == h[2].sum() and h[2].min() >= 65535 // V
    assert {pc.half_of(0, V, w0)[1] for V, w0, _ in pc.HALVES} == {0, 1}


def test_tied_and_grouped_cases():
    desc, counts, vocab = pc.tied_case(pc.TIED_EMPTY)
    assert desc.shape == (600, 4, 8) and (counts == 0).sum() == 5 and pc.TIED_F > 2 * 256
    sc = R.select(desc, counts, vocab, 0, 1, 0, 1, 10)["scores"]      # weighting 0: under idf a word of every frame weighs 0
    live = counts > 0
    assert (sc[np.ix_(live, live)][~np.eye(595, dtype=bool)] == 1 << 20).all() and (sc[~live] == -1).all()
    desc, counts, vocab = pc.grouped_case()
    sc = R.select(desc, counts, vocab, 1, 1, 0, 1, 10)["scores"]
    assert (sc == 0).sum() > 10000 and (sc > 0).sum() > 2000 and (counts == 0).sum() == 3 and counts[0] > 0 and counts[1] > 0


# ---- consensus --------------------------------------------------------------------------------------------------------------------

def test_consensus_graph_reaches_the_second_pass_of_both_classes():
    g = pc.consensus_graph()
    n = pc.CNS_TRACKS
    assert len(g["off"]) == n + 1 and pc.cns_grid(n) == pc.CNS_GRID_MAX
    lens = np.diff(g["off"])
    long2, mid2 = pc.second_pass_start(n, 2), pc.second_pass_start(n, 1)
    assert (long2, mid2) == (4096, 16384) and n > mid2
    assert set(np.flatnonzero(lens > 32).tolist()) == set(pc.CNS_LONG_AT) and set(lens[list(pc.CNS_LONG_AT)].tolist()) == {33, 65}
    assert set(np.flatnonzero((lens > 8) & (lens <= 32)).tolist()) == set(pc.CNS_MID_AT) and set(lens[list(pc.CNS_MID_AT)].tolist()) == {9, 32}
    assert {4096, 4097, 8191, 8192}.issubset(pc.CNS_LONG_AT) and min(pc.CNS_LONG_AT) < 4096
    assert {16384, 16385, n - 1}.issubset(pc.CNS_MID_AT) and min(pc.CNS_MID_AT) < 16384
    # every pattern of the two classes (length x clean / middle / last) in a first pass and in a later one
    for at, start in ((pc.CNS_LONG_AT, long2), (pc.CNS_MID_AT, mid2)):
        first = {g["pattern"][t] for t in at if t < start}
        later = {g["pattern"][t] for t in at if t >= start}
        assert len(first) == 6 and later == first
    assert (lens[[t for t in range(n) if t not in pc.CNS_LONG_AT + pc.CNS_MID_AT]] == 2).all()
    # nodes are distinct, inside the table, and a track's copies of a pattern carry the pattern's pixels
    assert len({tuple(x) for x in g["nodes"].tolist()}) == len(g["nodes"]) and g["nodes"][:, 1].max() == g["stride"] - 1
    for t in (0, 1, 4096, 8192, 16384, n - 1):
        nd = g["nodes"][g["off"][t]:g["off"][t + 1]]
        assert [(int(f), tuple(g["kps"][f][k])) for f, k in nd] == g["patterns"][g["pattern"][t]]
    assert 65 * 64 // 2 == 2080 <= 4096                                       # every track exhaustive under max_hyp = 2080


def test_tiled_yardstick_equals_the_yardstick_on_the_whole_graph():
    """the yardstick's own loop over the 16400 tracks (1.6 s), sampled tracks included"""
    g = pc.consensus_graph()
    in_summary = np.array([0, 0, 21, 22, 23, 99, 24, 5], np.int32)
    to = pc.graph_track_of(g)
    kw = dict(inlier_px=4.0, min_parallax_deg=1.0, min_inliers=2, min_len=2, max_hyp=64, seed=5)
    want = cref.consensus(g["kps"], g["P"], g["off"], g["nodes"], in_summary=in_summary, track_of=to, stride=g["stride"], **kw)
    got = pc.consensus_expected(g, in_summary, track_of=to, **kw)
    for k in ("offsets", "nodes", "summary", "map", "flags", "stats", "report", "near", "keep", "track_of", "xyz"):
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape and got[k].tobytes() == want[k].tobytes(), k
    assert got["sampled"].sum() == 30 and (want["stats"][got["sampled"], 2] > 0).any()      # a sampled winner past h = 0


@pytest.mark.parametrize("max_hyp", [2080, 64, 40])
def test_tiled_yardstick_equals_the_yardstick_on_a_short_graph(max_hyp):
    g = pc.consensus_graph(150, long_at=(3, 50, 51, 52, 53, 54, 55, 149), mid_at=(0, 60, 61, 62, 63, 64, 65, 100))
    in_summary = np.array([0, 0, 21, 22, 23, 99, 24, 5], np.int32)
    to = pc.graph_track_of(g)
    kw = dict(inlier_px=4.0, min_parallax_deg=1.0, min_inliers=2, min_len=2, max_hyp=max_hyp, seed=5)
    want = cref.consensus(g["kps"], g["P"], g["off"], g["nodes"], in_summary=in_summary, track_of=to, stride=g["stride"], **kw)
    got = pc.consensus_expected(g, in_summary, track_of=to, **kw)
    for k in ("offsets", "nodes", "summary", "map", "flags", "stats", "report", "near", "keep", "track_of", "xyz"):
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape and got[k].tobytes() == want[k].tobytes(), k
    lens = np.diff(g["off"])
    assert (got["sampled"] == (lens * (lens - 1) // 2 > max_hyp)).all() and got["sampled"].any() == (max_hyp < 2080)
    assert (to == -9).any() and (got["track_of"][to == -9] == -9).all()
    # the graph is worth the comparison: kept and removed two-node tracks, dropped observations, nothing near a threshold
    assert not want["near"].any() and (want["map"] < 0).sum() > 20 and (want["map"] >= 0).sum() > 20 and want["report"][4] >= 8
    long_or_mid = lens > 2
    if max_hyp == 2080:
        odd = np.arange(150)[long_or_mid]
        assert sorted(want["stats"][odd, 0] - want["stats"][odd, 1]) == [0] * 6 + [1] * 10   # clean patterns keep all, the others lose one
    assert pc.probe_seed(5, 0) == 5 and cref.sampled_pair(pc.probe_seed(5, 77), 0, 9, 33) == cref.sampled_pair(5, 77, 9, 33)
