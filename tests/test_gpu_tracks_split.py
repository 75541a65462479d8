"""GPU tests of the split track graph (pgx_tracks_split_dev; include/pgx.h, "split mode") against the yardstick of
tests/tracks_split_ref.py: a component inconsistent at max_dist is split at the first tighter gate where its parts are
consistent instead of being dropped whole.  Every comparison is array for array -- offsets, nodes, per-node track ids and
all 16 summary slots -- on hand-built cases, random lists, the layouts of the gathered buffers (slot permutation, padding,
frame subsets), NN lists with rejected rows, a bench-size job whose junk edges join every true track into one component,
and the job's own lists through ShardedSequence.  The host form (pgx_tracks_finish_split) must agree, and with no gates the
mode must be pgx_tracks_dev.
"""
import numpy as np
import pytest
import torch

import photogrammetry_amd as pg
import tracks_split_ref as ref
from geom_gpu import DEV, INT_MAX, as_lists, constructed_job, random_case, run_tracks, run_tracks_split, tracks_buffers
from match_gpu import run_nn, upload
from oracle import tracks_np
from photogrammetry_amd import dist as pdist
from photogrammetry_amd import synth

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def engine():
    e = pg.Engine(0)
    yield e
    e.close()


def check(engine, counts, pl, m, stride, max_dist, gates, min_len=2, host=True):
    off, nodes, tof, s = run_tracks_split(engine, counts, pl, m, stride, max_dist, gates, min_len)
    e_off, e_nodes, e_tof, e_s = ref.arrays(counts, pl, m, stride, max_dist, gates, min_len)
    assert (off == e_off).all() and (nodes == e_nodes).all() and (tof == e_tof).all()
    assert s == ref.summary16(e_s), (s, e_s)
    if host:
        h = pg.tracks_host(counts, pl, [m[p] for p in range(len(pl))], max_dist, min_len, gates=gates)
        assert h == (as_lists(off, nodes), s[2], s[3], s[8:9 + len(gates)])
    return off, nodes, tof, s


def test_hand_built_case(engine):
    counts, pl, m, stride, max_dist, gates, exp = ref.hand_built()
    off, nodes, tof, s = check(engine, counts, pl, m, stride, max_dist, gates)
    assert as_lists(off, nodes) == exp and s[8:10] == [0, 10] and s[2:4] == [1, 3]
    assert tof[6, 1] == -1 and tof[4, 0] == tof[4, 1] == tof[5, 0] == -2
    # the same lists through today's graph: every component dropped
    _, _, _, s0 = run_tracks(engine, counts, pl, m, stride, max_dist)
    assert s0[0] == 0 and s0[2] == 3


@pytest.mark.parametrize("seed", range(6))
def test_random_lists_equal_reference(engine, seed):
    F, stride = 5 + seed, [7, 64, 300, 257, 33, 1024][seed]
    counts, pl, m = random_case(seed, F, stride)
    for max_dist, gates, min_len in ((59, [40, 20, 10, 5, 2, 1, 0], 2), (30, [8], 1), (45, [30, 12, 3], 3), (20, [], 2)):
        check(engine, counts, pl, m, stride, max_dist, gates, min_len, host=stride <= 300)


@pytest.mark.parametrize("seed", range(3))
def test_no_gates_is_tracks_dev_and_kept_tracks_survive(engine, seed):
    """n_gates = 0 is pgx_tracks_dev bit for bit (slots [0..7]); with gates every track pgx_tracks_dev keeps is kept unchanged
    (level-0 groups are the same) and dropped_nodes never grows."""
    F, stride = 6 + seed, [64, 257, 1024][seed]
    counts, pl, m = random_case(10 + seed, F, stride)
    for max_dist in (3, 30, 59):
        p_off, p_nodes, p_tof, p_s = run_tracks(engine, counts, pl, m, stride, max_dist)
        off, nodes, tof, s = run_tracks_split(engine, counts, pl, m, stride, max_dist, [])
        assert (off == p_off).all() and (nodes == p_nodes).all() and (tof == p_tof).all()
        assert s[:8] == p_s and s[8] == p_s[1] and s[9:] == [0] * 7
        kept = {tuple(t) for t in as_lists(p_off, p_nodes)}
        for gates in ([max_dist - 1], [max_dist - 1, max_dist // 2, 0]):
            off, nodes, tof, s = run_tracks_split(engine, counts, pl, m, stride, max_dist, gates)
            assert kept <= {tuple(t) for t in as_lists(off, nodes)}
            assert s[3] <= p_s[3] and s[8] == p_s[1]


def test_pair_order_slot_permutation_padding_and_frame_subset(engine):
    F, stride = 7, 96
    counts, pl, m = random_case(42, F, stride, dmax=40)
    max_dist, gates = 30, [20, 6, 2]
    e_off, e_nodes, e_tof, e_s = ref.arrays(counts, pl, m, stride, max_dist, gates)
    assert e_s["per_level"][1:] != [0, 0, 0]         # the case exercises the refinement levels
    o = np.random.default_rng(3).permutation(len(pl))
    off, nodes, tof, s = run_tracks_split(engine, counts, [pl[i] for i in o], m[o], stride, max_dist, gates)
    assert (off == e_off).all() and (nodes == e_nodes).all() and (tof == e_tof).all() and s == ref.summary16(e_s)
    G, fs = 3, 3
    slot = [(f % G) * fs + f // G for f in range(F)]
    ids = -np.ones(G * fs, dtype=np.int32)
    c_s = np.zeros(G * fs, dtype=np.int32)
    for f in range(F):
        ids[slot[f]] = f
        c_s[slot[f]] = counts[f]
    c_s[ids < 0] = 50
    pl_s = [(slot[a], slot[b]) for a, b in pl] + [(8, 0), (-1, -1)]
    m_s = np.concatenate([m, np.zeros((2, stride, 3), dtype=np.int32)])
    off, nodes, tof, s = run_tracks_split(engine, c_s, pl_s, m_s, stride, max_dist, gates, frame_ids=ids, n_frames=F)
    assert (off == e_off).all() and (nodes == e_nodes).all() and (tof == e_tof).all() and s == ref.summary16(e_s)
    sub = [1, 2, 4, 6]
    ids2 = -np.ones(G * fs, dtype=np.int32)
    for i, f in enumerate(sub):
        ids2[slot[f]] = i
    keep = [p for p, (a, b) in enumerate(pl) if a in sub and b in sub]
    e2 = ref.arrays(counts[sub], [(sub.index(pl[p][0]), sub.index(pl[p][1])) for p in keep], m[keep], stride, max_dist, gates)
    off, nodes, tof, s = run_tracks_split(engine, c_s, pl_s, m_s, stride, max_dist, gates, frame_ids=ids2, n_frames=len(sub))
    assert (off == e2[0]).all() and (nodes == e2[1]).all() and (tof == e2[2]).all() and s == ref.summary16(e2[3])


def test_bench_size_recovers_the_tracks_of_the_giant_component(engine):
    """64 x 4096, all 2016 pairs: at max_dist = 200 the junk matches (>= 90) join every true track into one inconsistent
    component, which pgx_tracks_dev drops (test_gpu_tracks.py).  Split at the gate 64, it falls apart into exactly the
    ground-truth tracks -- pgx_tracks_dev's result at max_dist = 64 -- all of them at level 1."""
    F, K = 64, 4096
    counts, pl, m, perm, vis = constructed_job(F, K, 7)
    _, _, _, p_s = run_tracks(engine, counts, pl, m, K, 200)
    assert p_s[2] >= 1 and p_s[6] > 1000
    off, nodes, tof, s = run_tracks_split(engine, counts, pl, m, K, 200, [64])
    t_off, t_nodes, t_tof, t_s = run_tracks(engine, counts, pl, m, K, 64)
    assert (off == t_off).all() and (nodes == t_nodes).all() and (tof == t_tof).all()
    nvis = vis.sum(0)
    assert s[0] == int((nvis >= 2).sum()) and s[1] == int(nvis[nvis >= 2].sum()) and s[2] == 0
    assert s[8:10] == [0, s[1]] and s[4] == p_s[4]
    e_off, e_nodes, e_tof, e_s = ref.arrays(counts, pl, m, K, 200, [64])
    assert (off == e_off).all() and (nodes == e_nodes).all() and (tof == e_tof).all() and s == ref.summary16(e_s)
    # four gates, as in the measurements; the levels below 64 find nothing left to split
    off4, nodes4, tof4, s4 = run_tracks_split(engine, counts, pl, m, K, 200, [64, 48, 32, 16])
    assert (off4 == off).all() and (nodes4 == nodes).all() and (tof4 == tof).all() and s4[:10] == s[:10] and s4[10:] == [0] * 6


def test_nn_lists_are_accepted(engine):
    """Lists of pgx_match_nn_batch_dev: rejected rows are (i, -1, PGX_DIST_NONE) and never link."""
    rng = np.random.default_rng(8)
    base, _, _ = synth.true_match_descriptors(600, 8, 4, flip=0.0)
    F, stride = 6, 640
    descs = []
    for f in range(F):
        keep = rng.permutation(600)[: 450 + 30 * f]
        bits = np.unpackbits(base[keep].view(np.uint8), axis=1)
        bits ^= (rng.random(bits.shape) < 0.15).astype(np.uint8)
        descs.append(np.packbits(bits, axis=1).view(np.uint32))
    dev = upload(stride, 8, descs)
    counts = dev[3]
    pl = [(i, j) for i in range(F) for j in range(i + 1, F)]
    m = run_nn(engine, dev, stride, 8, pl, 120, 0.95, False)
    assert (m[..., 1] == -1).any() and (m[m[..., 1] == -1][:, 2] == INT_MAX).all()
    off, nodes, tof, s = check(engine, counts, pl, m, stride, 120, [80, 60, 40])
    assert s[0] > 100


def test_bad_arguments_and_duplicate_frames(engine):
    i32 = dict(dtype=torch.int32, device=DEV)
    t = torch.zeros(64, **i32)
    s16 = torch.zeros(16, **i32)
    for gates in ([10, 20], [64], [70], [30, 30], [-1], [60, 50, 40, 30, 20, 10, 5, 1]):
        with pytest.raises(pg.ArgumentException):
            engine.tracks_split_dev(t, t, t, 1, 2, 4, 2, 64, gates, 2, t, t, t, s16)
    # two slots naming frame 0: reported by check_status, and the context stays usable
    counts, pl, m, stride, max_dist, gates, exp = ref.hand_built()
    ids = np.arange(8, dtype=np.int32)
    ids[5] = 0
    nf = 8
    d_m, d_c, d_pl, d_ids, (track_of, offsets, nodes) = tracks_buffers(counts, pl, m, stride, ids, nf)
    engine.tracks_split_dev(d_m, d_c, d_pl, len(pl), 8, stride, nf, max_dist, gates, 2, track_of, offsets, nodes, s16,
                            d_frame_ids=d_ids)
    with pytest.raises(pg.ArgumentException):
        engine.check_status()
    off, nodes, tof, s = run_tracks_split(engine, counts, pl, m, stride, max_dist, gates)
    assert as_lists(off, nodes) == exp


def _small_job(engine, gates):
    W, H, NKP, radius, F = 640, 360, 1024, 16, 6
    engine.set_brief_pairs(pg.make_brief_pairs(0, 50, 256))
    engine.set_detect_params(np.float32(0.1), radius)
    engine.set_capacity(1 << 17, NKP)
    engine.set_dewarp_map(pg.build_dewarp_map(W, H, [3e-4, 1e-7, 0, 0, 0]))
    base = torch.from_numpy(synth.make_frame(W, H, seed=77, n_shapes=3000)).to(DEV)
    d_frames = torch.empty((F, H, W, 4), dtype=torch.uint16, device=DEV)
    for i in range(F):
        d_frames.view(torch.int64)[i] = torch.roll(base.view(torch.int64), shifts=(2 * i, 5 * i), dims=(0, 1))
    pl = pdist.all_pairs(F)
    tr = {"max_dist": 80, "min_len": 2}
    if gates is not None:
        tr["gates"] = gates
    job = pdist.ShardedSequence(engine, W, H, F, pl, NKP, 8, DEV, stream=torch.cuda.Stream(device=DEV), tracks=tr)
    torch.cuda.synchronize()
    job.step(d_frames)
    engine.check_status()
    torch.cuda.synchronize()
    return job, pl, NKP


def test_sharded_sequence_with_gates(engine):
    job, pl, NKP = _small_job(engine, [60, 40, 24])
    counts = job.counts()
    lists = np.stack([job.matches(p).cpu().numpy() for p in range(len(pl))])
    e_off, e_nodes, e_tof, e_s = ref.arrays(counts, pl, lists, NKP, 80, [60, 40, 24])
    summ = job.track_summary()
    assert summ == dict({k: e_s[k] for k in ref.KEYS}, per_level=e_s["per_level"]) and summ["n_tracks"] > 100
    assert job.tracks() == as_lists(e_off, e_nodes) and (job.track_of.cpu().numpy() == e_tof).all()
    # without gates: today's path and today's result
    job0, pl0, _ = _small_job(engine, None)
    lists0 = np.stack([job0.matches(p).cpu().numpy() for p in range(len(pl0))])
    exp, _, exp_s = tracks_np.tracks(job0.counts(), pl0, lists0, 80, 2)
    assert job0.tracks() == exp and job0.track_summary() == exp_s
