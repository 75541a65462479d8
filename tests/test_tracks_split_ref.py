"""CPU tests (no GPU) of the split track graph (include/pgx.h, "split mode"):
  * the three formulations of tests/tracks_split_ref.py -- literal nesting, sequential refinement, vectorised -- agree on
    random small graphs, and with no gates they are the frozen oracle (oracle/tracks_np.py);
  * a hand-built case has its known answer: a joined pair of tracks splits, a conflict at every gate stays dropped, a node
    that splits off alone is no track;
  * the host form (pgx_tracks_finish_split through pg.tracks_host(..., gates=...)) gives the literal answer, also under
    per-pair max_dist values below a gate, and adding pairs stays linear in their number;
  * the new kernels are in libpgx.so's code object with no private segment, no spills and at most 32 VGPRs.
"""
import ctypes as C
import functools
import time

import numpy as np
import pytest

import photogrammetry_amd as pg
import photogrammetry_amd._lib as L
import geom_gpu
import tracks_split_ref as ref
from codeobj import kernels
from oracle import tracks_np

INT_MAX = 2**31 - 1


# geom_gpu's lists with sparser pairs and with the rejected rows of NN lists (k2 = -1)
random_case = functools.partial(geom_gpu.random_case, p_pair=0.5, k2_lo=-1)


def check_all(counts, pl, m, stride, max_dist, gates, min_len):
    a = ref.literal(counts, pl, m, max_dist, gates, min_len)
    b = ref.sequential(counts, pl, m, max_dist, gates, min_len)
    assert a[0] == b[0] and a[2] == b[2] and (a[1] == b[1]).all()
    off, nodes, tof, s = ref.arrays(counts, pl, m, stride, max_dist, gates, min_len)
    assert geom_gpu.as_lists(off, nodes) == a[0] and s == a[2]
    w = a[1].shape[1]
    assert (tof[:, :w] == a[1]).all() and (tof[:, w:] == -1).all()
    assert sum(s["per_level"]) == s["n_nodes"] and len(s["per_level"]) == len(gates) + 1
    return a


@pytest.mark.parametrize("seed", range(8))
def test_formulations_agree_on_random_graphs(seed):
    F, stride = 4 + seed, [5, 9, 17, 12, 8, 30, 6, 21][seed]
    counts, pl, m = random_case(seed, F, stride)
    for max_dist, gates, min_len in ((59, [40, 20, 10, 5, 2, 1, 0], 2), (30, [20, 8], 1), (45, [44], 3), (10, [], 2),
                                     (60, [3], 2)):
        check_all(counts, pl, m, stride, max_dist, gates, min_len)


@pytest.mark.parametrize("seed", range(4))
def test_no_gates_is_the_frozen_oracle(seed):
    F, stride = 5 + seed, [7, 33, 16, 64][seed]
    counts, pl, m = random_case(100 + seed, F, stride)
    for max_dist, min_len in ((0, 2), (4, 1), (30, 3)):
        tr, tof, s = check_all(counts, pl, m, stride, max_dist, [], min_len)
        e_tr, e_tof, e_s = tracks_np.tracks(counts, pl, m, max_dist, min_len)
        assert tr == e_tr and (tof == e_tof).all() and s == dict(e_s, per_level=[e_s["n_nodes"]])
        off, nodes, tof2, s2 = ref.arrays(counts, pl, m, stride, max_dist, [], min_len)
        e = tracks_np.tracks_arrays(counts, pl, m, stride, max_dist, min_len)
        assert (off == e[0]).all() and (nodes == e[1]).all() and (tof2 == e[2]).all() and s2 == dict(e[3], per_level=[e[3]["n_nodes"]])


def test_hand_built_case():
    counts, pl, m, stride, max_dist, gates, exp = ref.hand_built()
    tr, tof, s = check_all(counts, pl, m, stride, max_dist, gates, 2)
    assert tr == exp
    assert s["per_level"] == [0, 10] and s["dropped"] == 1 and s["dropped_nodes"] == 3 and s["largest_dropped"] == 3
    assert s["edges"] == 11 and s["longest"] == 4
    assert tof[6, 1] == -1 and tof[4, 0] == tof[4, 1] == tof[5, 0] == -2 and tof[5, 1] == tof[7, 1] == -1
    # without the gate every one of the three components is dropped
    tr0, _, s0 = tracks_np.tracks(counts, pl, m, max_dist, 2)
    assert tr0 == [] and s0["dropped"] == 3


@pytest.fixture(scope="module")
def lib():
    """The host form lives in libpgx.so: build it (no GPU needed) before the first call."""
    L.build()
    return L.lib()


def _host(counts, pl, m, max_dist, gates, min_len):
    return pg.tracks_host(counts, pl, [m[p] for p in range(len(pl))], max_dist, min_len, gates=gates)


def test_host_form_equals_the_literal_rule(lib):
    counts, pl, m, stride, max_dist, gates, exp = ref.hand_built()
    tr, nd, ndn, per_level = _host(counts, pl, m, max_dist, gates, 2)
    assert tr == exp and (nd, ndn) == (1, 3) and per_level == [0, 10]
    for seed in range(6):
        F, stride = 4 + seed, [5, 9, 17, 12, 8, 30][seed]
        counts, pl, m = random_case(200 + seed, F, stride)
        for max_dist, gates, min_len in ((59, [40, 20, 10, 5, 2, 1, 0], 2), (30, [20, 8], 1), (10, [], 2)):
            tr, _, s = ref.literal(counts, pl, m, max_dist, gates, min_len)
            assert _host(counts, pl, m, max_dist, gates, min_len) == (tr, s["dropped"], s["dropped_nodes"], s["per_level"])
        # without gates: today's host form, unchanged
        e_tr, _, e_s = tracks_np.tracks(counts, pl, m, 30, 2)
        assert pg.tracks_host(counts, pl, [m[p] for p in range(len(pl))], 30, 2) == (e_tr, e_s["dropped"], e_s["dropped_nodes"])


def test_host_form_rejects_bad_gates(lib):
    counts, pl, m, stride, max_dist, gates, exp = ref.hand_built()
    for bad in ([64], [40, 40], [20, 30], [-1], [60, 50, 40, 30, 20, 10, 5, 1]):
        with pytest.raises(pg.ArgumentException):
            _host(counts, pl, m, max_dist, bad, 2)


def test_host_form_per_pair_gate(lib):
    """add_pair keeps only the edges within the pair's own max_dist, so at a level whose gate lies above that max_dist the
    pair's edges enter up to its max_dist only: the pair's gate at level l is min(its max_dist, g_l).  Here pair (0, 3) is
    added under 59 (its joining edge at 60 is never stored: A and B are tracks at level 0), and pair (6, 7) under 52, with
    the gates [55, 40]: its edge at 50 is stored and enters level 1 (gate 55 > 52), so the component resolves only at 40."""
    counts, pl, m, stride, _, _, _ = ref.hand_built()
    per_pair = {(0, 3): 59, (6, 7): 52}
    gates = [55, 40]
    c = np.ascontiguousarray(counts, dtype=np.int32)
    h = C.c_void_p()
    assert lib.pgx_tracks_create(c.ctypes.data_as(C.c_void_p), len(c), C.byref(h)) == 0
    try:
        for p, (a, b) in enumerate(pl):
            rows = np.ascontiguousarray(m[p], dtype=np.int32)
            assert lib.pgx_tracks_add_pair(h, a, b, rows.ctypes.data_as(C.c_void_p), len(rows), per_pair.get((a, b), 64)) == 0
        g = np.array(gates, dtype=np.int32)
        s = np.zeros(16, dtype=np.int32)
        nt, nn = C.c_int(0), C.c_int(0)
        assert lib.pgx_tracks_finish_split(h, g.ctypes.data_as(C.c_void_p), len(g), 2, C.byref(nt), C.byref(nn),
                                           s.ctypes.data_as(C.c_void_p)) == 0
    finally:
        lib.pgx_tracks_destroy(h)
    # the same graph with every entry beyond its pair's max_dist removed, under one max_dist of 64
    m2 = m.copy()
    for p, ab in enumerate(pl):
        m2[p][m2[p][:, 2] > per_pair.get(ab, 64)] = [0, 0, INT_MAX]
    tr, _, e = ref.literal(counts, pl, m2, 64, gates, 2)
    assert s.tolist() == ref.summary16(e)
    assert tr == [[(0, 0), (1, 0), (2, 0), (3, 0)], [(0, 1), (1, 1), (2, 1), (3, 1)], [(6, 0), (7, 0)]]
    assert e["per_level"] == [8, 0, 2] and e["dropped_nodes"] == 3


def test_host_form_builds_in_linear_time(lib):
    """Adding pairs must not copy the kept edges on every call: 496 pairs x 4096 entries (2 M edges) take well under a second
    (a per-pair exact reserve made this about 8 s)."""
    F, K = 32, 4096
    rng = np.random.default_rng(5)
    counts = np.full(F, K, dtype=np.int32)
    pl = [(a, b) for a in range(F) for b in range(a + 1, F)]
    rows = np.stack([np.tile(np.arange(K), (len(pl), 1)), rng.integers(0, K, (len(pl), K)), rng.integers(0, 64, (len(pl), K))],
                    axis=2).astype(np.int32)
    c = np.ascontiguousarray(counts)
    h = C.c_void_p()
    assert lib.pgx_tracks_create(c.ctypes.data_as(C.c_void_p), F, C.byref(h)) == 0
    try:
        t0 = time.perf_counter()
        for p, (a, b) in enumerate(pl):
            r = np.ascontiguousarray(rows[p])
            assert lib.pgx_tracks_add_pair(h, a, b, r.ctypes.data_as(C.c_void_p), K, 64) == 0
        dt = time.perf_counter() - t0
    finally:
        lib.pgx_tracks_destroy(h)
    assert dt < 3.0, dt


def test_split_kernels_exist_without_scratch():
    for needle in ("k_trks_prep", "k_trks_mark", "k_trks_reset", "k_trks_union", "k_trks_flatten"):
        mds = kernels(needle)
        assert len({md["name"] for md in mds}) == 1, (needle, [md["name"] for md in mds])
        for md in mds:
            assert md["private_segment_fixed_size"] == 0, md
            assert md["vgpr_spill_count"] == 0 and md["sgpr_spill_count"] == 0, md
            assert md["vgpr_count"] <= 32, md      # co-resident with the next step's distance kernel
