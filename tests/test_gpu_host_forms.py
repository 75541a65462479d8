"""GPU tests of the host forms of the five geometry stages (pgx_triangulate_tracks, pgx_bundle_adjust, pgx_register_frames,
pgx_verify_pair, pgx_relative_pose) and of the four matchers (pgx_match, pgx_knn, pgx_knn_guided, pgx_match_batch) as callers
of one staging layer (csrc/pgx_hoststage.h): all nine pack their inputs into the context's pinned
image, upload it to st_a in one copy and download from st_b.

What the stage tests do not reach: a small call behind a large one on the same context (stale bytes in the three shared
buffers), the optional outputs as NULL through the raw binding (the Engine wrappers always pass buffers), and the empty edges.
Every expected value is the device form's on the same inputs, or the same host call on a context of its own, compared on the
raw bytes."""
import contextlib

import numpy as np
import pytest
import torch

import geom_gpu as g
import match_gpu as mg
import photogrammetry_amd as pg
from geom_gpu import DEV, F64, I32, bits
from photogrammetry_amd import synth

pytestmark = pytest.mark.gpu

MAXD, NONE = 64, 2**31 - 1
K0, K1 = np.array([1200.0, 1150.0, 960.0, 540.0]), np.array([1100.0, 1250.0, 900.0, 600.0])
POSE_R, POSE_T = synth.rot_y(np.radians(8.0)), np.array([-1.0, 0.1, 0.2])
BAND = 2.0      # pixels round the epipolar line: pair_scene rounds its projections to whole pixels
MATCHERS = ("match", "knn", "guided", "match_batch")
FORMS = ("triangulate", "bundle", "register", "verify", "pose") + MATCHERS
KNN_RUNS = [(k, col) for k in (1, 2) for col in (False, True)]      # every host() of knn / guided makes these four calls
# (export, index of the optional output among its arguments, its key or keys in host()'s result)
OPTIONAL = {"triangulate": ("pgx_triangulate_tracks", 14, "node_err"), "bundle": ("pgx_bundle_adjust", 18, "node_err"),
            "register": ("pgx_register_frames", 21, "node_inlier"), "verify": ("pgx_verify_pair", 15, "inlier"),
            "pose": ("pgx_relative_pose", 16, "cand_Rt"), "knn": ("pgx_knn", 9, ("col_k1", "col_k2")),
            "guided": ("pgx_knn_guided", 13, ("col_k1", "col_k2"))}


def track_scene(n_points, nf, seed):
    """a make_scene scene with its true tracks: perturbed cameras and points for bundle adjustment, frames 2.. to register"""
    s = synth.make_scene(n_points, nf, seed=seed)
    off, nodes, pid = synth.scene_tracks(s)
    fixed, reg = np.zeros(nf, np.int32), np.ones(nf, np.int32)
    fixed[[0, nf - 1]], reg[:2] = 1, 0
    Rt, X = synth.perturb(s["Rt"], s["points"][pid], seed=2, fixed=fixed)
    flags = np.zeros(len(off) - 1, np.int32)
    flags[::5] = 8
    return dict(s=s, kps=s["kps"], off=off, nodes=nodes, fixed=fixed, reg=reg, Rt=Rt, X=X, pts=s["points"][pid], flags=flags)


def pair_scene(n1, n2, seed):
    """two views of min(n1, n2) points (a fifth of them junk in the second view) and unmatched keypoints behind them; the list
    holds one row per keypoint of the first view, shuffled -> kp1, kp2, ml [n1][3], F, K_a, K_b"""
    rng = np.random.default_rng(seed)
    n = min(n1, n2)
    X = np.c_[rng.uniform(-3, 3, n), rng.uniform(-2, 2, n), rng.uniform(4, 9, n)]
    Y = X @ POSE_R.T + POSE_T
    kp1, kp2 = np.zeros(n1, pg.KEYPOINT_DTYPE), np.zeros(n2, pg.KEYPOINT_DTYPE)
    for kp, K, Z in ((kp1, K0, X), (kp2, K1, Y)):
        kp["x"], kp["y"] = rng.integers(0, 1920, len(kp)), rng.integers(0, 1080, len(kp))
        kp["x"][:n], kp["y"][:n] = np.round(K[0] * Z[:, 0] / Z[:, 2] + K[2]), np.round(K[1] * Z[:, 1] / Z[:, 2] + K[3])
    junk = np.flatnonzero(rng.random(n) < 0.2)
    kp2["x"][junk], kp2["y"][junk] = rng.integers(0, 1920, len(junk)), rng.integers(0, 1080, len(junk))
    ml = np.zeros((n1, 3), np.int32)
    ml[:, 0], ml[:, 1], ml[:, 2] = np.arange(n1), -1, NONE
    ml[:n, 1], ml[:n, 2] = np.arange(n), rng.integers(0, MAXD + 1, n)
    kmat = lambda K: np.array([[K[0], 0.0, K[2]], [0.0, K[1], K[3]], [0.0, 0.0, 1.0]])  # noqa: E731
    F = np.linalg.inv(kmat(K0)).T @ POSE_R.T @ synth.skew(POSE_T).T @ np.linalg.inv(kmat(K1))
    return dict(kp1=kp1, kp2=kp2, ml=ml[rng.permutation(n1)], F=(F / np.linalg.norm(F)).reshape(9), Ka=K0, Kb=K1)


def match_scene(pair, seed):
    """a pair_scene with 256-bit descriptors: the points the two views share differ in at most 16 bits, the rest is random"""
    rng = np.random.default_rng(seed)
    n1, n2 = len(pair["kp1"]), len(pair["kp2"])
    d1, d2 = synth.random_descriptors(n1, 8, seed + 1), synth.random_descriptors(n2, 8, seed + 2)
    n = min(n1, n2)
    d2[:n] = d1[:n] ^ (np.uint32(1) << rng.integers(0, 32, (n, 8)).astype(np.uint32)) ^ (np.uint32(1) << rng.integers(0, 32, (n, 8)).astype(np.uint32))
    return dict(pair, d1=d1, d2=d2, F32=pair["F"].astype(np.float32))


def batch_scene(rows, pl, seed):
    return dict(descs=[synth.random_descriptors(n, 8, seed + f) for f, n in enumerate(rows)], pl=pl)


def cut(sc, n1, n2):
    """a pair or matcher scene cut to its first n1 and n2 keypoints"""
    sc = dict(sc)
    for k, n in (("kp1", n1), ("ml", n1), ("d1", n1), ("kp2", n2), ("d2", n2)):
        if k in sc:
            sc[k] = sc[k][:n]
    return sc


def knn_keys(k, col):
    tag = "_k%d%s" % (k, "_col" if col else "")
    return "idx" + tag, "dist" + tag, "col_k%d" % k


def as_pairs(rows):
    return np.ascontiguousarray(rows).reshape(-1).view(pg.PAIR_DTYPE)


def host(engine, form, sc):
    """the host form on a scene -> the wrapper's dict (knn, guided: the results of the four KNN_RUNS under knn_keys)"""
    if form == "match":
        return dict(out=engine.match(sc["d1"], sc["d2"]))
    if form in ("knn", "guided"):
        r = {}
        for k, col in KNN_RUNS:
            got = (engine.knn(sc["d1"], sc["d2"], k, col) if form == "knn" else
                   engine.knn_guided(sc["d1"], sc["kp1"], sc["d2"], sc["kp2"], sc["F32"], BAND, k, col))
            r.update(zip(knn_keys(k, col), got))
        return r
    if form == "match_batch":
        return {"list%d" % m: lst for m, lst in enumerate(engine.match_batch(sc["descs"], sc["pl"]))}
    if form == "triangulate":
        return engine.triangulate_tracks(sc["kps"], sc["s"]["P"], sc["off"], sc["nodes"], 1.0, 0.5, 10)
    if form == "bundle":
        return engine.bundle_adjust(sc["kps"], sc["s"]["K"], sc["Rt"], sc["fixed"], sc["off"], sc["nodes"], sc["X"],
                                    track_flags=sc["flags"], max_iters=5, huber_px=2.0)
    if form == "register":
        return engine.register_frames(sc["kps"], sc["s"]["K"], sc["s"]["Rt"], sc["reg"], sc["off"], sc["nodes"], sc["pts"], None, 64,
                                      g.IP, 6, 5, g.SEED)
    if form == "verify":
        return engine.verify_pair(sc["kp1"], sc["kp2"], sc["ml"], MAXD, 64, 1.5, 8, 2, g.SEED)
    return engine.relative_pose(sc["kp1"], sc["kp2"], sc["ml"], MAXD, sc["F"], sc["Ka"], sc["Kb"], 2.0, 0.7, 10)


def device(engine, form, sc):
    """the device form on the same inputs, the pair forms with their frames in slots 1 and 2 of three, the two-set matchers
    in slots 0 and 1 of two, the batch in slots of the largest set that a pair names -> the wrapper's keys"""
    if form == "match_batch":
        named = {f for p in sc["pl"] for f in p}
        S = max([len(sc["descs"][f]) for f in named] + [1])
        out = mg.run_match(engine, [d if f in named else d[:0] for f, d in enumerate(sc["descs"])], sc["pl"], S)
        return {"list%d" % m: as_pairs(out[m, :len(sc["descs"][a])]) for m, (a, _) in enumerate(sc["pl"])}
    if form in MATCHERS:
        n1, n2 = len(sc["d1"]), len(sc["d2"])
        S = max(n1, n2, 1)
        if form == "match":
            return dict(out=as_pairs(mg.run_match(engine, [sc["d1"], sc["d2"]], [(0, 1)], S)[0, :n1]))
        dev = mg.upload(S, 8, [sc["d1"], sc["d2"]], kps=[np.stack([kp["x"], kp["y"]], 1) for kp in (sc["kp1"], sc["kp2"])])
        r = {}
        for k, col in KNN_RUNS:
            idx, dist, cnn = mg.run_knn(engine, dev, S, 8, [(0, 1)], k, col, guide=([sc["F32"]], BAND) if form == "guided" else None)
            r.update(zip(knn_keys(k, col), (idx[0, :n1], dist[0, :n1]) + ((cnn[0, :n2],) if col else ())))
        return r
    if form in ("verify", "pose"):
        n1, n2 = len(sc["kp1"]), len(sc["kp2"])
        S = max(n1, n2, 1)
        kp, ml = np.zeros((3, S), pg.KEYPOINT_DTYPE), np.zeros((1, S, 3), np.int32)
        kp[1, :n1], kp[2, :n2], ml[0, :n1] = sc["kp1"], sc["kp2"], sc["ml"]
        d_kp, d_ml = torch.from_numpy(kp.view(np.int32).reshape(3, S, 4)).to(DEV), torch.from_numpy(ml).to(DEV)
        d_c, d_pl = torch.tensor([0, n1, n2], **I32), torch.tensor([[1, 2]], **I32)
        stats, rep = torch.full((1, 8), 9, **I32), torch.full((8,), 7, **I32)
        if form == "verify":
            out, Fd, inl = torch.full((1, S, 3), 77, **I32), torch.full((1, 9), 5.0, **F64), torch.full((1, S), 9, **I32)
            engine.verify_pairs_dev(d_kp, d_ml, d_c, d_pl, 1, S, MAXD, out, Fd, stats, rep, 64, 1.5, 8, 2, g.SEED, d_inlier=inl)
            engine.check_status()
            return dict(out=out.cpu().numpy()[0, :n1].reshape(-1).view(pg.PAIR_DTYPE), F=Fd.cpu().numpy()[0], stats=stats.cpu().numpy()[0],
                        inlier=inl.cpu().numpy()[0, :n1])
        d_F = torch.from_numpy(sc["F"].reshape(1, 9)).to(DEV)
        d_K = torch.from_numpy(np.stack([np.zeros(4), sc["Ka"], sc["Kb"]])).to(DEV)
        Rt, sigma, cand = torch.full((1, 12), 5.0, **F64), torch.full((1,), 5.0, **F64), torch.full((1, 4, 12), 5.0, **F64)
        fr = [torch.full((3, 12), 5.0, **F64), torch.full((3, 12), 5.0, **F64), torch.full((3,), 9, **I32), torch.full((3,), 9, **I32)]
        engine.init_pair_dev(d_kp, d_ml, d_c, d_pl, 1, 3, S, 3, MAXD, d_F, d_K, Rt, stats, *fr, rep, 2.0, 0.7, 10, d_sigma=sigma,
                             d_cand_Rt=cand)
        engine.check_status()
        return dict(Rt=Rt.cpu().numpy()[0], stats=stats.cpu().numpy()[0], sigma=float(sigma.cpu()[0]), cand_Rt=cand.cpu().numpy()[0])
    # no nodes: one row that no offset reaches, so that the device form has a buffer to be handed
    d = g.device_problem(sc["kps"], sc["off"], sc["nodes"] if len(sc["nodes"]) else np.zeros((1, 2), np.int32))
    d["n_nodes"] = len(sc["nodes"])
    if form == "bundle":
        return g.ba_run(engine, d, sc["s"]["K"], sc["Rt"], sc["fixed"], sc["X"], iters=5, huber=2.0, flags=sc["flags"])
    if form == "register":
        return g.reg_run(engine, d, sc["s"]["K"], sc["s"]["Rt"], sc["reg"], sc["pts"], n_samples=64, min_inliers=6, refine_iters=5)
    n, nn = max(d["n_tracks"], 1), d["nf"] * d["stride"]
    xyz, q, fl = torch.full((n, 3), 5.0, **F64), torch.full((n, 3), 5.0, **F64), torch.full((n,), 7, **I32)
    summ, err = torch.full((8,), 7, **I32), torch.full((nn,), 5.0, **F64)
    dP = torch.from_numpy(np.ascontiguousarray(sc["s"]["P"], np.float64).reshape(d["nf"], 12)).to(DEV)
    engine.triangulate_tracks_dev(d["kp"], d["F"], d["stride"], d["nf"], dP, d["off"], d["nodes"], d["tsum"], d["n_tracks"], xyz, q, fl,
                                  summ, 1.0, 0.5, 10, d_node_err=err)
    engine.check_status()
    n = d["n_tracks"]
    return dict(xyz=xyz.cpu().numpy()[:n], quality=q.cpu().numpy()[:n], flags=fl.cpu().numpy()[:n],
                node_err=err.cpu().numpy()[:d["n_nodes"]], summary=summ.cpu().numpy())


def same(a, b, skip=()):
    assert a.keys() == b.keys()
    for k in a:
        if k not in skip:
            assert (a[k] is None and b[k] is None) or bits(np.asarray(a[k])) == bits(np.asarray(b[k])), k


def fresh(form, sc):
    """the host form on a context of its own"""
    e = pg.Engine(0)
    try:
        return host(e, form, sc)
    finally:
        e.close()


def host_free_knn(sc):
    """the distance of every row of d1 to its nearest row of d2, on the CPU"""
    x = sc["d1"][:, None, :] ^ sc["d2"][None, :, :]
    return np.unpackbits(x.view(np.uint8), axis=2).sum(2).min(1)


@pytest.fixture(scope="module")
def scenes():
    big, small = track_scene(300, 6, 3), track_scene(20, 3, 4)
    assert max(len(k) for k in big["kps"]) >= 250 and max(len(k) for k in small["kps"]) <= 20
    pb, ps = pair_scene(300, 280, 5), pair_scene(20, 23, 6)
    mb, ms = match_scene(pb, 7), match_scene(ps, 8)
    assert (host_free_knn(mb) < 64).sum() >= 200       # the shared points are each other's nearest by a wide margin
    sc = {f: (pb, ps) if f in ("verify", "pose") else (mb, ms) if f in MATCHERS else (big, small) for f in FORMS}
    # the small batch has a frame of 300 rows that no pair names: its slots are those of the 23 rows
    sc["match_batch"] = (batch_scene((300, 280, 40), [(0, 1), (1, 0), (2, 0)], 9), batch_scene((20, 23, 300), [(0, 1), (1, 0)], 12))
    return sc


@pytest.fixture(scope="module")
def alone(scenes):
    """every small call on a context that has seen no other call"""
    return {f: fresh(f, scenes[f][1]) for f in FORMS}


@pytest.mark.parametrize("form", FORMS)
def test_a_small_call_behind_a_large_one_gives_the_bits_of_a_fresh_context(engine, scenes, alone, form):
    big, small = scenes[form]
    same(host(engine, form, big), device(engine, form, big))      # the large call itself is the device form's
    same(host(engine, form, small), alone[form])
    same(alone[form], device(engine, form, small))


def test_the_forms_share_their_staging_without_seeing_each_other(engine, scenes, alone):
    """every form's large call, then every form's small one, relative_pose straight behind bundle_adjust and the matchers
    between the geometry forms"""
    assert (alone["guided"]["idx_k2"][:, 0] >= 0).sum() >= 10      # the band holds the true matches: the lists are not trivial
    for f in FORMS:
        host(engine, f, scenes[f][0])
    for f in ("verify", "knn", "register", "match_batch", "triangulate", "guided", "bundle", "pose", "match", "verify", "knn"):
        same(host(engine, f, scenes[f][1]), alone[f])


@contextlib.contextmanager
def null_argument(engine, export, pos):
    """the raw binding's `export` called with NULL as its argument `pos`, under the wrapper's marshalling of the others"""
    L = engine._L

    class Binding:
        def __getattr__(self, name):
            f = getattr(L, name)
            return f if name != export else (lambda *a: f(*a[:pos], None, *a[pos + 1:]))
    engine._L = Binding()
    try:
        yield
    finally:
        engine._L = L


@pytest.mark.parametrize("form", list(OPTIONAL))
@pytest.mark.parametrize("size", [0, 1])
def test_a_null_optional_output_leaves_the_others_bit_for_bit(engine, scenes, alone, form, size):
    export, pos, key = OPTIONAL[form]
    keys = key if isinstance(key, tuple) else (key,)
    sc = scenes[form][size]
    full = host(engine, form, sc)
    with null_argument(engine, export, pos):
        part = host(engine, form, sc)
    same(full, part, skip=keys)
    for key in keys:
        assert not np.asarray(part[key]).any() and np.asarray(full[key]).any()      # the wrapper's zeros: nothing was written


def test_the_wrapper_passes_null_candidates_itself(engine, scenes):
    sc = scenes["pose"][1]
    full = host(engine, "pose", sc)
    part = engine.relative_pose(sc["kp1"], sc["kp2"], sc["ml"], MAXD, sc["F"], sc["Ka"], sc["Kb"], 2.0, 0.7, 10, candidates=False)
    same(full, part, skip=("cand_Rt",))
    assert part["cand_Rt"] is None


@pytest.mark.parametrize("form", ["verify", "pose"])
@pytest.mark.parametrize("n1,n2", [(0, 0), (0, 23), (20, 0)])
def test_an_empty_keypoint_set(engine, scenes, form, n1, n2):
    host(engine, form, scenes[form][0])
    sc = cut(scenes[form][1], n1, n2)
    got = host(engine, form, sc)
    same(got, device(engine, form, sc))
    assert got["stats"][0] == 0 and (form == "pose" or len(got["out"]) == n1)       # no candidates


@pytest.mark.parametrize("form", ["knn", "guided"])
@pytest.mark.parametrize("n1,n2", [(0, 0), (0, 23), (20, 0)])
def test_an_empty_descriptor_set(engine, scenes, form, n1, n2):
    host(engine, form, scenes[form][0])
    sc = cut(scenes[form][1], n1, n2)
    got = host(engine, form, sc)
    same(got, device(engine, form, sc))
    for k, col in KNN_RUNS:      # no neighbour anywhere: every row and every column that exists says so
        idx, dist, cnn = knn_keys(k, col)
        assert got[idx].shape == got[dist].shape == (n1, k) and (got[idx] == -1).all() and (got[dist] == NONE).all()
        assert not col or (got[cnn].shape == (n2,) and (got[cnn] == -1).all())


def test_match_with_an_empty_set(engine, scenes):
    big, small = scenes["match"]
    host(engine, "match", big)
    assert len(host(engine, "match", cut(small, 0, 23))["out"]) == 0        # no row: no list, no error
    with pytest.raises(pg.ArgumentOutOfRangeException):
        host(engine, "match", cut(small, 20, 0))
    same(host(engine, "match", small), device(engine, "match", small))      # the context goes on


def test_match_batch_delivers_every_list_beside_an_empty_second_set(engine, scenes):
    big, small = scenes["match_batch"]
    host(engine, "match_batch", big)
    descs, pl = [small["descs"][0], small["descs"][1], small["descs"][2][:0]], [(0, 1), (1, 2), (1, 0)]
    with pytest.raises(pg.ArgumentOutOfRangeException):
        engine.match_batch(descs, pl)
    got = {"list%d" % m: lst for m, lst in enumerate(engine.last_batch_lists)}
    d_out = mg.run_match(engine, descs, pl, 23, wait=False)      # the device form reports the same pair through the status word
    with pytest.raises(pg.ArgumentOutOfRangeException):
        engine.check_status()
    out = d_out.cpu().numpy()
    same(got, {"list%d" % m: as_pairs(out[m, :len(descs[a])]) for m, (a, _) in enumerate(pl)})
    assert len(got["list1"]) == 23 and (got["list1"]["dist"] == NONE).all() and (got["list0"]["dist"] < NONE).any()


@pytest.mark.parametrize("form", ["triangulate", "bundle", "register"])
@pytest.mark.parametrize("n_tracks", [0, 1])
def test_no_tracks_and_a_track_without_nodes(engine, scenes, form, n_tracks):
    host(engine, form, scenes[form][0])
    sc = dict(scenes[form][1])
    sc["off"], sc["nodes"] = np.zeros(n_tracks + 1, np.int32), np.zeros((0, 2), np.int32)
    sc["X"], sc["pts"], sc["flags"] = sc["X"][:n_tracks], sc["pts"][:n_tracks], sc["flags"][:n_tracks]
    got = host(engine, form, sc)
    if form == "triangulate" and n_tracks == 0:     # returns before any GPU work, the summary zeroed
        assert not got["summary"].any() and all(len(got[k]) == 0 for k in ("xyz", "quality", "flags", "node_err"))
    else:
        same(got, device(engine, form, sc))
