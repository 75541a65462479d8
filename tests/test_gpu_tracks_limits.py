"""GPU tests of the track graph (csrc/k_tracks.hip: pgx_tracks_dev, pgx_tracks_split_dev) past its scan, grid-stride, chunk
and table limits: the later passes of k_trk_scan_sums and its carry, the grid-stride passes of k_trk_init, k_trks_prep and
k_trks_reset over the nodes and over the per-frame tables, the grid-stride of k_trk_union / k_trks_union, a conflict whose
only witness is the frame's hash table, the probe wrap of both tables, k_trk_rank over segments of n_frames entries, and
n_frames far above the number of slots.  The cases and the host-side proof that each reaches its path are
tests/tracks_limits_cases.py and tests/test_tracks_limits_cases.py.  Every comparison is exact and array for array --
offsets, nodes, track_of over all n_frames * stride entries and every summary slot -- against oracle.tracks_np.tracks_arrays
or tracks_split_ref.arrays; the workspace is the context's and persists between calls, so the cases whose paths a stale
workspace would break run again behind a different case and must repeat themselves bit for bit."""
import numpy as np
import pytest

import photogrammetry_amd as pg
import tracks_limits_cases as tc
from geom_gpu import run_tracks_split

pytestmark = pytest.mark.gpu

HOST_FORM_NODES = 20000         # the sequential host form is compared too up to this many nodes


@pytest.fixture(scope="module")
def engine():
    e = pg.Engine(0)
    yield e
    e.close()


def run(engine, case, split, min_len=2):
    d, (max_dist, gates) = case.dev, case.gates
    return run_tracks_split(engine, d["counts"], [tuple(p) for p in d["pl"].tolist()], d["m"], d["stride"], max_dist,
                            gates if split else None, min_len, frame_ids=d["frame_ids"], n_frames=d["n_frames"])


def first_difference(got, exp):
    if got.shape != exp.shape:
        return "shapes %s, %s" % (got.shape, exp.shape)
    at = np.flatnonzero(got.reshape(-1) != exp.reshape(-1))
    return "first of %d at flat index %d: %d, expected %d" % (len(at), at[0], got.reshape(-1)[at[0]], exp.reshape(-1)[at[0]])


def check(engine, case, split, min_len=2, host=True):
    """one call against the oracle (and the host form where the case is small) -> the device's arrays"""
    got = run(engine, case, split, min_len)
    e_off, e_nodes, e_tof, e_s = case.oracle(split, min_len)
    assert got[3] == e_s, (got[3], e_s)
    for name, g, e in (("offsets", got[0], e_off), ("nodes", got[1], e_nodes), ("track_of", got[2], e_tof)):
        assert np.array_equal(g, e), (name, first_difference(g, e))
    assert got[2].shape == (case.dev["n_frames"], case.dev["stride"])
    if host and case.reach["N"] <= HOST_FORM_NODES:
        o, (max_dist, gates) = case.ora, case.gates
        h = pg.tracks_host(o["counts"], [tuple(p) for p in o["pl"].tolist()], list(o["m"]), max_dist, min_len,
                           gates=gates if split else None)
        assert h[0] == tc.as_lists(e_off, e_nodes) and list(h[1:3]) == e_s[2:4]
        if split:
            assert h[3] == e_s[8:9 + len(gates)]
    return got


def same(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a[:3], b[:3])) and a[3] == b[3]


def check_around(engine, case, between, split, min_len=2):
    """the case, a different case on the same context, the case again: both runs equal the oracle and each other"""
    first = check(engine, case, split, min_len)
    check(engine, between, split, min_len, host=False)
    again = check(engine, case, split, min_len, host=False)
    assert same(first, again)


def check_twice(engine, case, split, min_len=2):
    first = check(engine, case, split, min_len)
    assert same(first, check(engine, case, split, min_len, host=False))


@pytest.mark.parametrize("split", (False, True), ids=("plain", "split"))
@pytest.mark.parametrize("name", sorted(tc.SCAN_CARRY))
def test_scan_carry(engine, name, split):
    """More than 256 (and more than 512) scan blocks: passes 2 and 3 of k_trk_scan_sums' b0 loop, their carry into the track
    indices and node offsets of the tracks beyond node id 262 144 (524 288), and offsets[n_tracks]; six slots naming frames
    on both sides of the boundaries, or 260 slots of which six have keypoints."""
    kw = tc.SCAN_CARRY[name]
    case = tc.sparse_frames(**kw)
    assert case.reach["nb"] > tc.SCAN_NT
    check_around(engine, case, tc.other(kw), split)
    if name == "514":
        assert same(run(engine, tc.permuted(case, 1), split), case.oracle(split))


@pytest.mark.parametrize("split", (False, True), ids=("plain", "split"))
def test_node_array_passes(engine, split):
    """1030 frames x 1024: more than 4096 x 256 nodes, so k_trk_init, k_trks_prep and k_trks_reset take a second grid-stride
    pass over parent / root / rep / size / flag / cursor / track_of / active; frames 1024, 1025 and 1029 lie wholly in it."""
    case = tc.sparse_frames(**tc.NODE_PASSES)
    assert case.reach["N"] > tc.INIT_PASS
    check_around(engine, case, tc.other(tc.NODE_PASSES), split)
    if split:
        assert same(run(engine, tc.permuted(case, 2), split), case.oracle(split))


@pytest.mark.parametrize("split", (False, True), ids=("plain", "split"))
@pytest.mark.parametrize("seed", tc.TABLE_PASSES_SEEDS)
def test_table_passes(engine, seed, split):
    """16500 frames x 4 keypoints: 66 000 nodes, but 16500 x 64 table entries -- the tables of frames 16384 and up are cleared
    in the second pass only.  A root left there by the first call or by level 0 would flag a consistent component."""
    kw = tc.table_passes(seed)
    case = tc.sparse_frames(**kw)
    assert case.reach["table_entries"] > tc.INIT_PASS > case.reach["N"]
    check_around(engine, case, tc.other(kw), split)
    assert same(run(engine, tc.permuted(case, 3), split), case.oracle(split))


@pytest.mark.parametrize("M,stride", tc.UNION_SETS)
def test_union_grid_stride(engine, M, stride):
    """255, 256, 257, 513 and 258 work items for the 256 workgroups of k_trk_union and k_trks_union; the last item's edges
    decide tracks, so an item left out shows."""
    case = tc.union_items(M, stride)
    for split in (False, True):
        check(engine, case, split)
    if M == 257:
        for split in (False, True):
            assert same(run(engine, tc.permuted(case, 4), split), case.oracle(split))


@pytest.mark.parametrize("stride", tc.CONFLICT_STRIDES)
def test_conflict_witnesses(engine, stride):
    """Two keypoints of one frame in one wave, in one chunk, and in different chunks (the frame's table is the only witness), at
    level 0 and again at level 1; counts 0, 1, 255, 256, 257 and stride; consistent neighbours must stay tracks."""
    case = tc.conflicts(stride)
    for split in (False, True):
        for min_len in (2, 1):
            check_twice(engine, case, split, min_len)
    if stride == 513:
        for split in (False, True):
            assert same(run(engine, tc.permuted(case, 5), split), case.oracle(split))


@pytest.mark.parametrize("kind,stride", tc.WRAP_SETS)
def test_table_probe_wrap(engine, kind, stride):
    """Frames whose table fills past its last slot: the probe sequence goes on at slot 0, in the per-frame table (T = 64) and
    in the 512-slot LDS table.  min_len = 1: every node is a track, so a false flag or a lost root shows."""
    case = tc.table_wrap(kind, stride)
    for split in (False, True):
        check_twice(engine, case, split, 1)
    if kind == "global":
        for split in (False, True):
            assert same(run(engine, tc.permuted(case, 6), split, 1), case.oracle(split, 1))


def test_long_tracks(engine):
    """300 frames x 8: k_trk_rank over segments of 300 entries (the longest tested before had 64), at level 0 and, for the two
    tracks that one edge joins, at level 1."""
    case = tc.long_tracks()
    assert case.oracle(False)[3][5] == case.dev["n_frames"] == 300
    for split in (False, True):
        check(engine, case, split)
        assert same(run(engine, tc.permuted(case, 7), split), case.oracle(split))
