"""GPU tests of track consensus (csrc/k_consensus.hip: pgx_track_consensus_dev) past the grid-stride of its two longer length
classes.  The grid of k_cns_score and k_cns_write is capped at 1024 workgroups, so a lane group meets a second track only from
index 4096 on in the whole-wave class (more than 32 nodes) and from 16384 on in the 16-lane class (9 to 32 nodes);
tests/test_gpu_consensus.py reaches the stride with two-node tracks alone.  One graph of 16400 tracks has tracks of 33 and 65
nodes below 4096 and at 4096, 4097, 8191 and 8192 (a third pass), and tracks of 9 and 32 nodes below 16384 and at 16384, 16385
and the last index; each length comes clean, with a wrong observation in the middle and with one in the last position.  The
rewritten d_track_of checks the strided passes of k_cns_write node by node.

The graph, the launch rules and the tiled yardstick are tests/pairs_limits_cases.py; tests/test_pairs_limits_cases.py holds the
tiling to tests/consensus_ref.py bit for bit.  Every integer output is exact.  The points of tracks whose expected value is
tiled from a pattern (exhaustive tracks) are compared bit for bit; the points of sampled tracks, each evaluated by the
yardstick on its own, to 1e-9 of the distance to the mean camera centre, the rule of tests/test_gpu_consensus.py.

Wall time on an MI355X: 1.0 s of pytest time for the file's two tests (0.19 s and 0.06 s per call, the rest the graph and the
context)."""
import numpy as np
import pytest

import consensus_ref as ref
import pairs_limits_cases as pc
from geom_gpu import bits
from photogrammetry_amd import synth
from test_gpu_consensus import IN_SUMMARY, INT_KEYS, run

pytestmark = pytest.mark.gpu

KW = dict(inlier_px=4.0, min_parallax_deg=1.0, min_inliers=2, min_len=2, seed=5)


@pytest.fixture(scope="module")
def graph():
    g = pc.consensus_graph()
    g["dev"] = synth.device_tracks(g["kps"], g["off"], g["nodes"])
    g["track_of"] = pc.graph_track_of(g)
    return g


@pytest.mark.parametrize("max_hyp", [2080, 64])
def test_second_pass_of_the_two_longer_classes(engine, graph, max_hyp):
    """max_hyp = 2080 covers the 65 * 64 / 2 pairs of the longest track: every track is exhaustive and its result does not
    depend on its index.  max_hyp = 64: tracks of 32 nodes and more are sampled, their hypotheses depend on the index."""
    n = pc.CNS_TRACKS
    lens = np.diff(graph["off"])
    assert pc.cns_grid(n) == pc.CNS_GRID_MAX == 1024
    for cls, named in ((2, (4096, 4097, 8191, 8192)), (1, (16384, 16385, n - 1))):
        start = pc.second_pass_start(n, cls)
        assert all(t >= start and pc.cns_class(int(lens[t])) == cls for t in named)
        assert any(pc.cns_class(int(lens[t])) == cls for t in range(start))
    assert pc.cns_class(int(lens[8192])) == 2 and 8192 >= 2 * pc.second_pass_start(n, 2)        # a third pass

    in_summary = np.zeros(8, np.int32)
    in_summary[2:8] = IN_SUMMARY
    e = pc.consensus_expected(graph, in_summary, track_of=graph["track_of"], max_hyp=max_hyp, **KW)
    sampled = lens * (lens - 1) // 2 > max_hyp
    assert (e["sampled"] == sampled).all() and (sampled == ((max_hyp == 64) & (lens >= 32))).all() and sampled[16385] == (max_hyp == 64)
    assert not e["near"].any()

    got = run(engine, graph["dev"], graph["P"], track_of=graph["track_of"], max_hyp=max_hyp, **KW)
    for k in INT_KEYS:
        assert np.array_equal(got[k], e[k]), (k, np.flatnonzero(np.asarray(got[k]).ravel() != np.asarray(e[k]).ravel())[:8]
                                              if np.shape(got[k]) == np.shape(e[k]) else (np.shape(got[k]), np.shape(e[k])))
    assert np.array_equal(got["track_of"], e["track_of"])
    assert (e["track_of"] == -9).any() and (e["track_of"] == -3).sum() == e["report"][4] > 0 and (e["track_of"] == -1).any()

    # points: by the new index
    old = np.flatnonzero(e["map"] >= 0)
    assert got["xyz"].shape == e["xyz"].shape == (len(old), 3)
    tiled = ~sampled[old]
    assert bits(got["xyz"][tiled]) == bits(e["xyz"][tiled])
    _, _, _, C, _ = ref.frames(graph["P"])
    for tn in np.flatnonzero(~tiled):
        t = old[tn]
        nd = graph["nodes"][graph["off"][t]:graph["off"][t + 1]]
        centre = C[nd[:, 0]].mean(0)
        assert np.linalg.norm(got["xyz"][tn] - e["xyz"][tn]) <= 1e-9 * np.linalg.norm(e["xyz"][tn] - centre), t

    # every long and middle track lost exactly its wrong observation, whatever its index and pass
    for at in (pc.CNS_LONG_AT, pc.CNS_MID_AT):
        for i, t in enumerate(at):
            n_k, inl, hwin, flags = got["stats"][t]
            assert n_k == lens[t] and flags == 0 and inl == n_k - (0 if i % 3 == 0 else 1), (t, got["stats"][t])
            keep = e["keep"][graph["off"][t]:graph["off"][t + 1]]
            wrong = {0: None, 1: lens[t] // 2, 2: lens[t] - 1}[i % 3]
            assert (np.flatnonzero(~keep).tolist() == ([] if wrong is None else [wrong])), t
    if max_hyp == 2080:      # exhaustive: the same pattern gives the same statistics at every index
        for at in (pc.CNS_LONG_AT, pc.CNS_MID_AT):
            for i, t in enumerate(at):
                assert (got["stats"][t] == got["stats"][at[i % 6]]).all(), t
