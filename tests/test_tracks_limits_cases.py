"""The cases of tests/tracks_limits_cases.py reach what tests/test_gpu_tracks_limits.py names them for (no GPU).  Every builder
and parameter set of the GPU module is held here to its reach facts, read from the shapes and from the oracles' arrays, so that
a later change to a generator cannot quietly shrink a case below its limit; the launch constants the cases mirror are held to
the text of csrc/k_tracks.hip, so that a changed constant fails here instead of moving a limit out from under them; and at the
small cases the vectorised oracles are held to their sequential / literal formulations."""
import os
import re

import numpy as np
import pytest

import tracks_limits_cases as tc
import tracks_split_ref as ref
from oracle import tracks_np

SRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "photogrammetry_amd", "csrc", "k_tracks.hip")
BLOCK = os.path.join(os.path.dirname(SRC), "pgx_block.h")   # block_scan_array and block_tally_add, which k_tracks.hip calls


# ---------------------------------------------------------------------------------------------------- the mirrored launch facts

def test_constants_equal_the_kernel_source():
    text = open(SRC).read()
    vals = {}
    for name, expr in re.findall(r"^constexpr int (\w+) = ([^;]+);", text, flags=re.M):
        for tok in re.findall(r"[A-Za-z_]\w*", expr):
            expr = re.sub(r"\b%s\b" % tok, str(vals[tok]), expr)
        assert re.fullmatch(r"[\d\s*+()-]+", expr), (name, expr)
        vals[name] = eval(expr)
    for name in ("TRK_NT", "SCAN_NT", "SCAN_ITEMS", "TRK_UNION_GRID", "TRKS_UNION_GRID", "FL_SLOTS", "TRK_INIT_GRID_MAX"):
        assert vals[name] == getattr(tc, name), name
    # the cap is what trk_init_grid applies, to the larger of the node count and the table entries, in workgroups of TRK_NT
    body = text[text.index("unsigned trk_init_grid("):text.index("// init -> union -> flatten")]
    assert "if (gi > TRK_INIT_GRID_MAX) gi = TRK_INIT_GRID_MAX;" in body and "(init_items + TRK_NT - 1) / TRK_NT" in body
    assert "a.N > (long long)a.n_frames * a.T ? a.N : (long long)a.n_frames * a.T" in body
    # k_trk_scan_sums: SCAN_NT block sums per pass; the union grids; the table size; the two hash rules and the priority
    block = open(BLOCK).read()
    assert "block_scan_array<unsigned long long, SCAN_NT>(a.bsum, a.bsum, nb, lds);" in text
    assert "for (int base = 0; base < n; base += NT) {" in block and "if (j < n) store(j, carry + ex);" in block and "carry += tot;" in block
    assert "n_items < TRK_UNION_GRID ? n_items : TRK_UNION_GRID" in text and "n_items < TRKS_UNION_GRID ? n_items : TRKS_UNION_GRID" in text
    assert text.count("a.T = 64;") == 1 and "while (a.T < 2 * stride) a.T <<= 1;" in text
    assert "return (uint32_t)x * %du;" % tc.HASH_MUL in text
    assert "block_tally_add(hkey, hcnt, hmin, FL_SLOTS, r, x);" in text
    assert "((uint32_t)r * %du) >> 9;" % tc.HASH_MUL in block and "h &= (uint32_t)(slots - 1);" in block
    assert "(r * %du) >> 7;" % tc.HASH_MUL in text and "h &= (uint32_t)(a.T - 1);" in text
    assert (tc.SCAN_PASS, tc.INIT_PASS) == (262144, 1048576)


def test_hash_helpers():
    assert [tc.table_size(s) for s in (1, 4, 32, 33, 256, 300, 512, 513, 1024)] == [64, 64, 64, 128, 512, 1024, 1024, 2048, 2048]
    assert int(tc.prio(3)) == (3 * 2654435761) % 2**32 and int(tc.lds_home(3)) == ((3 * 2654435761) % 2**32 >> 9) & 511
    assert int(tc.table_home(77, 64)) == ((77 * 2654435761) % 2**32 >> 7) & 63
    assert not tc.wraps([0, 1, 62, 63], 64) and tc.wraps([63, 63], 64) and tc.wraps([61, 62, 62, 63], 64)
    assert not tc.wraps([61, 62, 63], 64) and not tc.wraps([], 64)


# ----------------------------------------------------------------------------------------------------------- the three passes

def reach_counts(case, boundary, split):
    first = tc.first_ids(case, split)
    return int((first >= boundary).sum()), int((first < boundary).sum())


@pytest.mark.parametrize("name", sorted(tc.SCAN_CARRY))
def test_scan_carry_reach(name):
    kw = tc.SCAN_CARRY[name]
    for case in (tc.sparse_frames(**kw), tc.other(kw)):
        assert case.reach["nb"] > tc.SCAN_NT and case.reach["N"] > tc.SCAN_PASS
        beyond, before = reach_counts(case, tc.SCAN_PASS, False)
        assert beyond >= 20 and before >= 1 and case.oracle(False)[3][2] >= 1, (beyond, before)
        beyond, before = reach_counts(case, tc.SCAN_PASS, True)
        assert beyond >= 20 and before >= 1 and sum(case.oracle(True)[3][9:]) > 0
        if name == "514":
            assert case.reach["nb"] > 2 * tc.SCAN_NT
            assert reach_counts(case, 2 * tc.SCAN_PASS, False)[0] >= 5 and reach_counts(case, 2 * tc.SCAN_PASS, True)[0] >= 5
    case = tc.sparse_frames(**kw)
    d = case.dev
    if kw.get("dense"):
        assert d["frame_ids"] is None and len(d["counts"]) == d["n_frames"] == 260 and (d["counts"] > 0).sum() == 6
    else:
        assert len(d["counts"]) == 7 and (d["frame_ids"] == -1).sum() == 1 and len(case.ora["pl"]) == len(d["pl"]) - 1


def test_node_passes_reach():
    for case in (tc.sparse_frames(**tc.NODE_PASSES), tc.other(tc.NODE_PASSES)):
        assert case.reach["N"] > tc.INIT_PASS
        beyond, before = reach_counts(case, tc.INIT_PASS, False)
        assert beyond >= 20 and before >= 1 and case.oracle(False)[3][2] >= 1
        assert reach_counts(case, tc.INIT_PASS, True)[0] >= 20
        assert tc.late_tracks_beyond(case, tc.INIT_PASS) >= 1          # active[] and the reset beyond the first pass


@pytest.mark.parametrize("seed", tc.TABLE_PASSES_SEEDS)
def test_table_passes_reach(seed):
    kw = tc.table_passes(seed)
    case = tc.sparse_frames(**kw)
    assert case.reach["table_entries"] > tc.INIT_PASS and case.reach["N"] < tc.INIT_PASS // 8 and case.reach["T"] == 64
    boundary = (tc.INIT_PASS // case.reach["T"]) * case.dev["stride"]    # first node of the first frame whose table lies in pass 2
    assert boundary == 16384 * 4
    beyond, before = reach_counts(case, boundary, False)
    assert beyond >= 1 and before >= 1 and case.oracle(False)[3][2] >= 1
    assert tc.late_tracks_beyond(case, boundary) >= 1
    assert tc.other(kw).oracle(True)[3] != case.oracle(True)[3]


# ------------------------------------------------------------------------------------------------------------------ the union

@pytest.mark.parametrize("M,stride", tc.UNION_SETS)
def test_union_items_reach(M, stride):
    case = tc.union_items(M, stride)
    items = {(255, 64): 255, (256, 64): 256, (257, 64): 257, (513, 64): 513, (129, 300): 258}[(M, stride)]
    assert case.reach["union_items"] == items == M * tc.chunks_of(stride)
    lo, hi = case.reach["last_item"]
    assert lo == (tc.chunks_of(stride) - 1) * tc.TRK_NT and hi == stride and case.dev["counts"][case.dev["pl"][-1][0]] == stride
    for split in (False, True):
        off, nodes, tof, s = case.oracle(split)
        for cut in (tc.without_rows(case, M - 1, lo, hi), tc.without_rows(case, M - 1, 0, stride)):
            c_off, c_nodes, c_tof, c_s = cut.oracle(split)
            assert c_s != s and not np.array_equal(c_tof, tof)
        assert s[0] > 20 and s[2] >= 1
    assert sum(case.oracle(True)[3][9:]) > 0


# --------------------------------------------------------------------------------------------------------------- the conflicts

def tof_at(tof, nodes):
    return [int(tof[f, k]) for f, k in nodes]


@pytest.mark.parametrize("stride", tc.CONFLICT_STRIDES)
def test_conflicts_reach(stride):
    case = tc.conflicts(stride)
    r = case.reach
    assert sorted(case.ora["counts"].tolist()) == sorted([0, 1, 255, 256, 257, stride, stride, stride])
    (k, k2) = r["forms"]["wave"]
    assert k // 64 == k2 // 64
    (k, k2) = r["forms"]["chunk"]
    assert k // 64 != k2 // 64 and k // tc.TRK_NT == k2 // tc.TRK_NT
    for name in ("chunks", "edge", "ends"):
        (k, k2) = r["forms"][name]
        assert k // tc.TRK_NT != k2 // tc.TRK_NT
    tof0, tof1 = case.oracle(False)[2], case.oracle(True)[2]
    for name, nodes in r["hard"].items():
        assert tof_at(tof0, nodes) == [-2] * len(nodes) == tof_at(tof1, nodes), name
    for name, nodes in r["soft"].items():
        assert tof_at(tof0, nodes) == [-2] * len(nodes), name
        t = tof_at(tof1, nodes)
        assert t[0] >= 0 and t[1] == -1 and set(t[2:]) == {t[0]}, (name, t)      # a track, and the second keypoint alone
    for nodes in r["kept"]:
        for tof in (tof0, tof1):
            t = tof_at(tof, nodes)
            assert t[0] >= 0 and set(t) == {t[0]}
    s1 = case.oracle(True)[3]
    assert s1[9] > 0 and s1[2] == len(r["hard"])


# --------------------------------------------------------------------------------------------------------------- the table wrap

@pytest.mark.parametrize("kind,stride", tc.WRAP_SETS)
def test_table_wrap_reach(kind, stride):
    case = tc.table_wrap(kind, stride)
    assert case.dev["stride"] == stride and (case.ora["counts"][list(case.reach["wrap"] + case.reach["plain"])] == stride).all()
    glob, lds = tc.wrapping_tables(case)
    if kind == "global":
        assert case.reach["T"] == 64 and case.reach["single_wrap"][:5] == (8, 10, 19, 21, 30)
        assert len(glob) >= 4 and set(glob) <= set(case.reach["wrap"])
    else:
        assert len(lds) >= 4 and {f for f, _ in lds} <= set(case.reach["wrap"]) and {ch for _, ch in lds} == {0}
    # every node is a track or flagged at min_len = 1, and both kinds of roots stand in the wrapping frames' tables
    for split in (False, True):
        off, nodes, tof, s = case.oracle(split, 1)
        valid = np.arange(stride)[None, :] < case.ora["counts"][:, None]
        assert (tof[valid] != -1).all() and (tof[valid] == -2).any() and s[2] >= 2
        for f in glob + [f for f, _ in lds]:
            assert (tof[f] == -2).any() and (tof[f] >= 0).any()


# ---------------------------------------------------------------------------------------------------------------- long tracks

def test_long_tracks_reach():
    case = tc.long_tracks()
    n = case.dev["n_frames"]
    assert n == 300 and case.dev["stride"] == 8
    s0, s1 = case.oracle(False)[3], case.oracle(True)[3]
    assert s0[5] == n and s0[0] == 6 and s0[2:4] == [1, 2 * n] and s0[6] == 2 * n
    assert sorted(np.diff(case.oracle(False)[0]).tolist()) == [case.reach["gap_track_len"]] + [n] * 5
    assert 2 <= case.reach["gap_track_len"] < n
    assert s1[5] == n and s1[0] == 8 and s1[2] == 0 and s1[9] == 2 * n           # two whole tracks resolved at level 1


# --------------------------------------------------------------------------------------- oracle cross-checks at the small cases

SMALL = ([lambda s=s: (tc.conflicts(s), 2) for s in tc.CONFLICT_STRIDES] + [lambda a=a: (tc.table_wrap(*a), 1) for a in tc.WRAP_SETS] +
         [lambda: (tc.long_tracks(), 2), lambda: (tc.union_items(257, 64), 2), lambda: (tc.union_items(129, 300), 2),
          lambda: (tc.sparse_frames(**tc.TABLE_PASSES), 2)])


@pytest.mark.parametrize("i", range(len(SMALL)))
def test_vectorised_oracles_equal_the_sequential_and_literal_ones(i):
    case, min_len = SMALL[i]()
    o, (max_dist, gates) = case.ora, case.gates
    assert case.reach["N"] <= 70000
    named = np.flatnonzero(o["counts"])              # the sequential forms walk every frame: renumber the named ones densely
    dense = -np.ones(len(o["counts"]), dtype=np.int64)
    dense[named] = np.arange(len(named))
    keep = (dense[o["pl"]] >= 0).all(axis=1)
    pl = [tuple(int(x) for x in dense[p]) for p in o["pl"][keep]]
    lists = [o["m"][p] for p in np.flatnonzero(keep)]

    def renumber(tracks):
        return [[(int(named[f]), k) for f, k in t] for t in tracks]

    for split in (False, True):
        off, nodes, tof, s = case.oracle(split, min_len)
        if split:
            tr, e_tof, e_s = ref.literal(o["counts"][named], pl, lists, max_dist, gates, min_len)
            assert s == [int(x) for x in ref.summary16(e_s)]
        else:
            tr, e_tof, e_s = tracks_np.tracks(o["counts"][named], pl, lists, max_dist, min_len)
            assert s == [e_s[k] for k in ref.KEYS] + [0]
        assert tc.as_lists(off, nodes) == renumber(tr)
        w = e_tof.shape[1]
        assert (tof[named][:, :w] == e_tof).all() and (tof[named][:, w:] == -1).all()
        rest = np.ones(len(tof), dtype=bool)
        rest[named] = False
        assert (tof[rest] == -1).all()
