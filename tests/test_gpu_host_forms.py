"""GPU tests of the eighteen host forms as callers of one staging layer (csrc/pgx_hoststage.h): the five
geometry stages (pgx_triangulate_tracks, pgx_bundle_adjust, pgx_register_frames, pgx_verify_pair, pgx_relative_pose), the four
matchers (pgx_match, pgx_knn, pgx_knn_guided, pgx_match_batch) and the nine added since (LATER: pgx_track_consensus,
pgx_vocab_train, pgx_select_pairs, pgx_depth_maps, pgx_depth_fuse, pgx_dense_views, pgx_rgba8_batch, pgx_cloud_merge, pgx_mesh).
All of them pack their inputs into the context's pinned image, upload it to st_a in one copy and download from st_b; nothing
ever clears the three buffers.

What the stage tests do not reach: a small call behind a large one on the same context (stale bytes in the three shared
buffers), the optional outputs as NULL through the raw binding (the Engine wrappers always pass buffers), and the empty edges.
The later forms add to that: lists of min(report, cap) rows fetched by a second download from sections that no source
zero-fills (pgx_depth_fuse, pgx_cloud_merge, pgx_mesh), what the caller is handed with PGX_E_CAPACITY, the workspaces that two
forms carve differently (ws_depth: depth maps and filter; ws_vocab: training and selection), optional sections in the middle of
an image that move every later offset between two calls, a refused call, and the empty edges.
Every expected value is the device form's on the same inputs, or the same host call on a context of its own, compared on the
raw bytes."""
import contextlib

import numpy as np
import pytest
import torch

import cloud_gpu
import consensus_gpu
import consensus_ref
import dense_views_gpu
import dense_views_ref
import depth_gpu
import depth_ref
import geom_gpu as g
import match_gpu as mg
import mesh_gpu
import pairs_gpu
import photogrammetry_amd as pg
from geom_gpu import DEV, F64, I32, bits
from photogrammetry_amd import synth
from photogrammetry_amd._lib import PGX_E_CAPACITY

pytestmark = pytest.mark.gpu

MAXD, NONE = 64, 2**31 - 1
K0, K1 = np.array([1200.0, 1150.0, 960.0, 540.0]), np.array([1100.0, 1250.0, 900.0, 600.0])
POSE_R, POSE_T = synth.rot_y(np.radians(8.0)), np.array([-1.0, 0.1, 0.2])
BAND = 2.0      # pixels round the epipolar line: pair_scene rounds its projections to whole pixels
MATCHERS = ("match", "knn", "guided", "match_batch")
LATER = ("track_consensus", "vocab_train", "select_pairs", "depth_maps", "depth_fuse", "dense_views", "rgba8_batch", "cloud_merge", "mesh")
FORMS = ("triangulate", "bundle", "register", "verify", "pose") + MATCHERS + LATER
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


# ---- the nine later forms: a scene is the wrapper's positional inputs, `kw` its keyword arguments, and `opt` the optional inputs
# that with_optional() switches on and off

MESH_CELL, MESH_ORIGIN = mesh_gpu.CELL, mesh_gpu.ORIGIN
SELECT = dict(weighting=1, top_k=2, window=1, min_score=1, max_pairs=None, scores=True)
# per form, a value that its *_args check refuses behind the Lock (cns_args, train_args, select_args, depth_args, fuse_args,
# dvw_args, mesh_args; refused() has cloud_args' cell = 0 and rgba8_args' frame of 65536 rows)
REFUSED = {"track_consensus": dict(max_hyp=0), "vocab_train": dict(iters=65), "select_pairs": dict(weighting=2), "depth_maps": dict(D=2),
           "depth_fuse": dict(rel_tol=-1.0), "dense_views": dict(q_near_pm=900, q_far_pm=100), "mesh": dict(band=4)}


def vary(sc, **kw):
    """the scene with these keyword arguments of its wrapper changed"""
    return dict(sc, kw=dict(sc["kw"], **kw))


def refused(form, sc):
    """the scene with one argument that the form answers with PGX_E_BADARG"""
    if form == "cloud_merge":
        return dict(sc, cell=0.0)
    if form == "rgba8_batch":
        return dict(sc, rgba=np.zeros((1, 65536, 1, 4), np.uint16))
    return vary(sc, **REFUSED[form])


def consensus_scene(base, plant):
    """a track_scene with a tenth of its tracks swapped pairwise in a frame they share (plant), under the stage's defaults"""
    nodes = consensus_ref.plant_swaps(base["s"], base["off"], base["nodes"], 0.1, 11)[0] if plant else base["nodes"]
    return dict(kps=base["kps"], P=base["s"]["P"], off=base["off"], nodes=nodes, kw=dict(consensus_gpu.DEFAULTS))


def vocab_scene(counts, stride, V, seed):
    desc = synth.random_descriptors(len(counts) * stride, 8, seed).reshape(len(counts), stride, 8)
    return dict(desc=desc, counts=np.array(counts, np.int32), kw=dict(V=V, iters=2, seed=5))


def maps_scene_small(seed):
    """make_case's noise frames: two references of three frames, two sources each, eight planes, the optional outputs off"""
    gray, P = depth_gpu.make_case(24, 16, 3, seed)
    return dict(gray=gray, P=P, views=np.array([[0, 1, 2], [1, 2, 0]], np.int32), ranges=np.array([(2.0, 6.0)] * 2),
                kw=dict(D=8, agg_radius=2, min_views=2, max_cost=depth_gpu.BIG, cost=False, warp=False, planes=False))


def fuse_scene_small():
    """three maps of 24 x 16 at the true depths of depth_ref's slanted back plane and front rectangle, seen from three centres"""
    W, H, f = 24, 16, 28.8
    centres = [(0.0, 0.0, 0.0), (0.6, 0.0, 0.0), (-0.6, 0.1, 0.0)]
    depth = np.stack([depth_ref.scene_render(C, 0.1, 1, W, H, f)[1] for C in centres])
    P = np.stack([depth_ref.scene_camera(C, W, H, f).reshape(12) for C in centres])
    return dict(depth=depth, views=depth_ref.all_views(3), P=P, kw=dict(rel_tol=0.05, min_agree=2, max_points=None, agree=False))


def views_scene(base, S, refs, flags, optional, seed):
    """the plan of the dense stage on a track_scene's graph and true points; opt: the optional inputs for with_optional()"""
    nf = len(base["kps"])
    perm = np.random.default_rng(seed).permutation(nf).astype(np.int32)
    opt = dict(refs=perm[:max(nf - 1, 1)], track_flags=base["flags"])
    kw = dict(dense_views_ref.DEFAULTS, refs=opt["refs"] if refs else None, track_flags=opt["track_flags"] if flags else None,
              pair_counts=optional, ref_stats=optional)
    return dict(off=base["off"], nodes=base["nodes"], xyz=base["pts"], P=base["s"]["P"], S=S, kw=kw, opt=opt)


def cloud_scene(n, seed, colour, optional, spread=2.0):
    c = cloud_gpu.synth(n, seed, spread)
    return dict(xyz=c["xyz"], src=c["src"], depth=c["depth"], views=c["views"], P=c["P"], cell=cloud_gpu.CELL, origin=cloud_gpu.ORIGIN,
                kw=dict(rgba8=c["rgba8"] if colour else None, max_points=None, pt_normal=optional, cell_of=optional), opt=dict(rgba8=c["rgba8"]))


def mesh_caps(n, kw):
    """(max_voxels, max_vertices, max_tris) as the wrapper sets them where kw leaves them None"""
    nvox = (2 * kw["band"]) ** 3 * n if kw["max_voxels"] is None else kw["max_voxels"]
    return nvox, nvox if kw["max_vertices"] is None else kw["max_vertices"], 6 * nvox if kw["max_tris"] is None else kw["max_tris"]


def mesh_scene(n, seed, band, optional, caps=(None, None, None)):
    c = mesh_gpu.synth(n, seed)
    agree = np.random.default_rng(seed + 1).integers(0, 4, c["depth"].shape).astype(np.int32)      # a quarter below min_agree
    opt = dict(agree=agree, rgba8=c["rgba8"])
    kw = dict(agree=agree if optional else None, min_agree=1, rgba8=c["rgba8"] if optional else None, band=band, max_voxels=caps[0],
              max_vertices=caps[1], max_tris=caps[2])
    return dict(xyz=c["xyz"], src=c["src"], depth=c["depth"], views=c["views"], P=c["P"], cell=MESH_CELL, origin=MESH_ORIGIN, kw=kw, opt=opt)


def with_optional(form, sc, on):
    """the scene with every optional input and output of its form present (on) or absent"""
    if form == "depth_maps":
        return vary(sc, cost=on, warp=on, planes=on)
    if form == "depth_fuse":
        return vary(sc, agree=on)
    if form == "select_pairs":
        return vary(sc, scores=on)
    if form == "dense_views":
        return vary(sc, refs=sc["opt"]["refs"] if on else None, track_flags=sc["opt"]["track_flags"] if on else None, pair_counts=on,
                    ref_stats=on)
    if form == "cloud_merge":
        return vary(sc, rgba8=sc["opt"]["rgba8"] if on else None, pt_normal=on, cell_of=on)
    assert form == "mesh"
    return vary(sc, agree=sc["opt"]["agree"] if on else None, rgba8=sc["opt"]["rgba8"] if on else None)


def host_later(engine, form, sc):
    kw = sc.get("kw", {})
    if form == "track_consensus":
        return engine.track_consensus(sc["kps"], sc["P"], sc["off"], sc["nodes"], **kw)
    if form == "vocab_train":
        vocab, report = engine.vocab_train(sc["desc"], sc["counts"], **kw)
        return dict(vocab=vocab, report=report)
    if form == "select_pairs":
        return engine.select_pairs(sc["desc"], sc["counts"], sc["vocab"], **kw)
    if form == "depth_maps":
        return engine.depth_maps(sc["gray"], sc["P"], sc["views"], sc["ranges"], **kw)
    if form == "depth_fuse":
        return engine.depth_fuse(sc["depth"], sc["views"], sc["P"], **kw)
    if form == "dense_views":
        return engine.dense_views(sc["off"], sc["nodes"], sc["xyz"], sc["P"], sc["S"], **kw)
    if form == "rgba8_batch":
        return dict(out=engine.rgba8_batch(sc["rgba"]))
    if form == "cloud_merge":
        return engine.cloud_merge(sc["xyz"], sc["src"], sc["depth"], sc["views"], sc["P"], sc["cell"], sc["origin"], **kw)
    assert form == "mesh"
    return engine.mesh(sc["xyz"], sc["src"], sc["depth"], sc["views"], sc["P"], sc["cell"], sc["origin"], **kw)


def device_later(engine, form, sc):
    """the device form over sentinel-filled outputs, cut to the wrapper's keys and lengths; a capacity error is no error here (the
    host form's return code is the test's to look at)"""
    kw = sc.get("kw", {})
    if form == "track_consensus":
        d = synth.device_tracks(sc["kps"], sc["off"], sc["nodes"])
        r = consensus_gpu.run(engine, d, sc["P"], in_summary=(0,) * 6, **kw)      # the host form has no input summary
        del r["track_of"]
        return r
    if form == "vocab_train":
        vocab, report = pairs_gpu.run_train(engine, sc["desc"], sc["counts"], kw["V"], kw["iters"], kw["seed"])
        return dict(vocab=vocab, report=report)
    if form == "select_pairs":
        F = len(sc["counts"])
        cap = F * (F - 1) // 2 if kw["max_pairs"] is None else kw["max_pairs"]
        r = pairs_gpu.run_select(engine, sc["desc"], sc["counts"], sc["vocab"], kw["weighting"], kw["top_k"], kw["window"], kw["min_score"],
                                 cap, kw["scores"])
        n = min(int(r["summary"][0]), cap)
        return dict(pairs=r["pairlist"][:n], pair_score=r["pair_score"][:n], scores=r["scores"], summary=r["summary"])
    if form == "depth_maps":
        assert kw["cost"] == kw["warp"] == kw["planes"]
        r = depth_gpu.run_maps(engine, sc["gray"], sc["P"], sc["views"], sc["ranges"], kw["D"], kw["agg_radius"], kw["min_views"],
                               kw["max_cost"], optional=kw["cost"])
        return r if kw["cost"] else dict(r, cost=None, warp=None, planes=None)
    if form == "depth_fuse":
        r = depth_gpu.run_fuse(engine, sc["depth"], sc["views"], sc["P"], kw["rel_tol"], kw["min_agree"], kw["max_points"], kw["agree"],
                               check=False)
        n = min(int(r["summary"][0]), sc["depth"].size if kw["max_points"] is None else kw["max_points"])
        return dict(xyz=r["xyz"][:n], src=r["src"][:n], agree=r["agree"] if kw["agree"] else None, summary=r["summary"])
    if form == "dense_views":
        plan = {k: v for k, v in kw.items() if k in dense_views_ref.DEFAULTS}
        r = dense_views_gpu.run(engine, sc["off"], sc["nodes"], sc["xyz"], kw["track_flags"], sc["P"], kw["refs"], sc["S"],
                                pair_counts=kw["pair_counts"], **plan)
        assert not r.pop("status")
        return r if kw["ref_stats"] else dict(r, ref_stats=None)
    if form == "rgba8_batch":
        F, H, W = sc["rgba"].shape[:3]
        out = torch.full((F, H, W), 77, **I32)
        d_rgba = torch.from_numpy(np.ascontiguousarray(sc["rgba"])).to(DEV)      # the uploaded frames
        torch.cuda.synchronize()
        engine.rgba8_batch_dev(d_rgba, F, W, H, out)
        engine.check_status()
        return dict(out=out.cpu().numpy().view(np.uint32))
    if form == "cloud_merge":
        assert kw["pt_normal"] == kw["cell_of"]
        n = len(sc["xyz"])
        cap = n if kw["max_points"] is None else kw["max_points"]
        r = cloud_gpu.run_merge(engine, sc["xyz"], sc["src"], sc["depth"], sc["views"], sc["P"], sc["cell"], sc["origin"], max_points=cap,
                                rgba8=kw["rgba8"], optional=kw["pt_normal"], check=False)
        k = min(int(r["report"][6]), cap)
        return dict(xyz=r["xyz"][:k], normal=r["normal"][:k], rgba8=r["rgba8"][:k], info=r["info"][:k],
                    pt_normal=r["pt_normal"][:n] if kw["pt_normal"] else None, cell_of=r["cell_of"][:n] if kw["cell_of"] else None,
                    report=r["report"])
    assert form == "mesh"
    caps = mesh_caps(len(sc["xyz"]), kw)
    c = {k: sc[k] for k in ("xyz", "src", "depth", "views", "P")}
    c.update({k: kw[k] for k in ("agree", "rgba8") if kw[k] is not None})
    r = mesh_gpu.run_mesh(engine, c, caps, sc["cell"], sc["origin"], band=kw["band"], min_agree=kw["min_agree"], check=False)
    kv, kt = min(int(r["report"][5]), caps[1]), min(int(r["report"][6]), caps[2])
    return dict(xyz=r["xyz"][:kv], normal=r["normal"][:kv], rgba8=r["rgba8"][:kv], info=r["info"][:kv], tri=r["tri"][:kt], report=r["report"])


def host(engine, form, sc):
    """the host form on a scene -> the wrapper's dict (knn, guided: the results of the four KNN_RUNS under knn_keys)"""
    if form in LATER:
        return host_later(engine, form, sc)
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
    if form in LATER:
        return device_later(engine, form, sc)
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
    sc.update(later_scenes(big, small))
    return sc


def later_scenes(big, small):
    """a large and a small scene per later form: the large call dirties every section that the small one uses, whose images are
    several times shorter.  What a scene needs of another stage (a vocabulary, depth maps) and the conditions on the results come
    from calls on contexts of their own."""
    sc = {}
    sc["track_consensus"] = (consensus_scene(big, True), consensus_scene(small, False))
    r_big, r_small = (fresh("track_consensus", s) for s in sc["track_consensus"])
    assert r_big["report"][4] >= 1 and r_big["report"][3] < r_big["report"][2]       # the large call drops nodes
    assert r_small["summary"][0] >= 1                                                   # the small one keeps a track

    sc["vocab_train"] = (vocab_scene((300, 280, 300, 150, 300, 299), 300, 64, 21), vocab_scene((23, 20, 17), 23, 4, 22))
    t_big, t_small = (fresh("vocab_train", s) for s in sc["vocab_train"])
    assert bits(t_big["report"]) != bits(t_small["report"])
    sc["select_pairs"] = tuple(dict(s, vocab=t["vocab"], kw=dict(SELECT, scores=on))
                               for s, t, on in zip(sc["vocab_train"], (t_big, t_small), (True, False)))
    for s in sc["select_pairs"]:
        assert len(fresh("select_pairs", s)["pairs"]) >= 2

    ds = depth_ref.scene()
    maps_big = dict(gray=ds["gray"], P=ds["P"], views=depth_ref.all_views(), ranges=np.array([ds["range"]] * 5),
                    kw=dict(D=depth_ref.SCENE_D, agg_radius=2, min_views=2, max_cost=depth_gpu.BIG, cost=True, warp=True, planes=True))
    sc["depth_maps"] = (maps_big, maps_scene_small(31))
    m_big, m_small = (fresh("depth_maps", s) for s in sc["depth_maps"])
    assert (m_small["flags"] == 0).any() and (m_small["flags"] != 0).any()             # valid and invalid pixels

    fuse_big = dict(depth=m_big["depth"], views=maps_big["views"], P=ds["P"], kw=dict(rel_tol=0.05, min_agree=2, max_points=None, agree=True))
    sc["depth_fuse"] = (fuse_big, fuse_scene_small())
    for s in sc["depth_fuse"]:
        assert 0 < fresh("depth_fuse", s)["summary"][0] < s["depth"].size

    sc["dense_views"] = (views_scene(big, 3, False, False, True, 41), views_scene(small, 2, True, True, False, 42))
    for s in sc["dense_views"]:
        assert fresh("dense_views", s)["report"][4] >= 1                                # a reference with a finite range

    rng = np.random.default_rng(51)
    sc["rgba8_batch"] = tuple(dict(rgba=rng.integers(0, 65536, (F, H, W, 4)).astype(np.uint16)) for F, H, W in ((5, 64, 96), (2, 5, 7)))

    sc["cloud_merge"] = (cloud_scene(20000, 61, True, True), cloud_scene(300, 62, False, False, spread=4 * cloud_gpu.CELL))
    for s, several in zip(sc["cloud_merge"], (3, 1)):
        r = fresh("cloud_merge", s)
        assert 0 < r["report"][6] < len(s["xyz"]) and r["info"][:, 0].max() >= several  # the large one: cells with several points

    sc["mesh"] = (mesh_scene(20000, 71, 2, True, caps=(60000, 30000, 60000)), mesh_scene(300, 72, 1, False))
    for s in sc["mesh"]:
        r = fresh("mesh", s)["report"]
        assert r[5] > 0 and r[6] > 0
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
    between the geometry forms; then the later forms among them: the filter straight behind the depth maps and the reverse (they
    carve ws_depth differently), selection straight behind training and the reverse (ws_vocab), the mesh straight behind the
    cloud, and a matcher and a geometry form of the first nine between the dense forms"""
    assert (alone["guided"]["idx_k2"][:, 0] >= 0).sum() >= 10      # the band holds the true matches: the lists are not trivial
    for f in FORMS:
        host(engine, f, scenes[f][0])
    for f in ("verify", "knn", "register", "match_batch", "triangulate", "guided", "bundle", "pose", "match", "verify", "knn"):
        same(host(engine, f, scenes[f][1]), alone[f])
    for f in ("depth_maps", "depth_fuse", "depth_maps", "knn", "triangulate", "vocab_train", "select_pairs", "vocab_train", "match",
              "register", "cloud_merge", "mesh", "verify", "guided", "dense_views", "match_batch", "bundle", "rgba8_batch", "track_consensus",
              "pose", "knn", "depth_fuse", "match", "verify", "mesh", "guided", "triangulate", "cloud_merge", "select_pairs"):
        same(host(engine, f, scenes[f][1]), alone[f])


@pytest.mark.parametrize("form", ["depth_maps", "depth_fuse", "dense_views", "cloud_merge", "mesh", "select_pairs"])
def test_optional_sections_toggled_between_two_calls(engine, scenes, form):
    """an optional section in the middle of an image moves every offset behind it: the large scene with all of them and the small
    one with none, then the reverse; the small call is that of a fresh context under the same flags"""
    big, small = scenes[form]
    for on in (True, False):
        host(engine, form, with_optional(form, big, on))
        sc = with_optional(form, small, not on)
        same(host(engine, form, sc), fresh(form, sc))


@contextlib.contextmanager
def returning(engine):
    """the wrappers raise before they return: for the calls inside, the return codes are collected instead -> their list"""
    codes = []
    engine._chk = codes.append
    try:
        yield codes
    finally:
        del engine._chk


# form -> (its capacities, each with the report slot of its true count; two other forms to call behind it)
CAPACITIES = {"depth_fuse": ((("max_points", 0),), ("cloud_merge", "knn")), "select_pairs": ((("max_pairs", 0),), ("vocab_train", "match")),
              "cloud_merge": ((("max_points", 6),), ("mesh", "verify")),
              "mesh": ((("max_voxels", 3), ("max_vertices", 5), ("max_tris", 6)), ("depth_fuse", "triangulate"))}


@pytest.mark.parametrize("form,cap,slot,others", [(f, cap, slot, others) for f, (caps, others) in CAPACITIES.items() for cap, slot in caps])
def test_what_a_capacity_error_leaves(engine, scenes, alone, form, cap, slot, others):
    """PGX_E_CAPACITY hands the caller the report and the first `cap` rows (include/pgx.h): those of the device form at the same
    capacity, bit for bit, behind a large call that left other rows in the lists' sections; the status word does not carry over"""
    big, small = scenes[form]
    report = "summary" if form in ("depth_fuse", "select_pairs") else "report"
    true = int(alone[form][report][slot])
    if form == "mesh":      # the other two capacities as the wrapper sets them: only `cap` is exceeded
        small = vary(small, **dict(zip(("max_voxels", "max_vertices", "max_tris"), mesh_caps(len(small["xyz"]), small["kw"]))))
    assert true >= 2
    host(engine, form, big)
    for n in (true - 1, true // 2):
        sc = vary(small, **{cap: n})
        with returning(engine) as codes:
            got = host(engine, form, sc)
        assert codes == [PGX_E_CAPACITY]
        same(got, device(engine, form, sc))
        if cap == "max_voxels":      # pgx.h: the table's entries in use, no vertex and no triangle
            assert got["report"][3] > n and got["report"][5] == 0 and got["report"][6] == 0
            assert all(len(got[k]) == 0 for k in ("xyz", "normal", "rgba8", "info", "tri"))
        else:                        # pgx.h: the full count, and the first n rows
            assert got[report][slot] == true
            lists = {"max_points": ("xyz",), "max_pairs": ("pairs", "pair_score"), "max_vertices": ("xyz", "normal", "rgba8", "info"),
                     "max_tris": ("tri",)}[cap]
            assert all(len(got[k]) == n for k in lists)
            full = alone[form]       # ... which for every form but the mesh are the first n of the uncut call
            if form != "mesh":
                assert all(bits(got[k]) == bits(full[k][:n]) for k in lists)
    for f in (form,) + others:
        same(host(engine, f, scenes[f][1]), alone[f])


@pytest.mark.parametrize("form", LATER)
def test_a_refused_call_leaves_nothing_behind(engine, scenes, alone, form):
    big, small = scenes[form]
    host(engine, form, big)
    with pytest.raises(pg.ArgumentException):
        host(engine, form, refused(form, small))
    same(host(engine, form, small), alone[form])


def emptied(form, sc, what):
    """the scene without references (R), without points (n_in) or without tracks (n_tracks)"""
    if what == "n_tracks":
        sc = dict(sc, off=np.zeros(1, np.int32), nodes=np.zeros((0, 2), np.int32), xyz=np.zeros((0, 3)))
        return vary(sc, track_flags=None) if form == "dense_views" else sc
    if what == "n_in":
        return dict(sc, xyz=np.zeros((0, 3)), src=np.zeros((0, 2), np.int32))
    if form == "dense_views":
        return vary(sc, refs=np.zeros(0, np.int32))
    S = sc["views"].shape[1] - 1
    if form == "depth_maps":
        return dict(sc, views=np.zeros((0, 1 + S), np.int32), ranges=np.zeros((0, 2)))
    return dict(sc, depth=sc["depth"][:0], views=np.zeros((0, 1 + S), np.int32))


@pytest.mark.parametrize("form,what", [("depth_maps", "R"), ("depth_fuse", "R"), ("dense_views", "R"), ("cloud_merge", "n_in"), ("mesh", "n_in"),
                                       ("track_consensus", "n_tracks"), ("dense_views", "n_tracks")])
def test_an_empty_edge_behind_a_large_call(engine, scenes, alone, form, what):
    big, small = scenes[form]
    host(engine, form, big)
    got = host(engine, form, emptied(form, small, what))
    for k in ("report", "summary"):
        assert k not in got or not got[k].any(), (k, got[k])
    if (form, what) == ("dense_views", "n_tracks"):      # a row per reference all the same: no source, no range
        same(got, device(engine, form, emptied(form, small, what)))
        assert (got["views"][:, 1:] == -1).all()
    else:
        lists = {"depth_maps": ("kq8", "depth", "flags"), "depth_fuse": ("xyz", "src"), "dense_views": ("views", "range"),
                 "cloud_merge": ("xyz", "normal", "rgba8", "info"), "mesh": ("xyz", "normal", "rgba8", "info", "tri"),
                 "track_consensus": ("nodes", "map", "xyz", "flags", "stats")}[form]
        assert all(len(got[k]) == 0 for k in lists)
    same(host(engine, form, small), alone[form])


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
