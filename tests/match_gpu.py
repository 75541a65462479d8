"""What the GPU tests of the matchers (greedy, exact nearest neighbour, guided) share: the upload of per-frame descriptor sets,
the run wrappers of the five batched entry points with sentinel-filled outputs, the detect oracle and the list comparison.
The engine is always the caller's.  A plain helper module: no test module imports another."""
import numpy as np
import torch

from oracle import cref
import photogrammetry_amd as pg

DEV = "cuda:0"
I32 = dict(dtype=torch.int32, device=DEV)


def upload(stride, words, descs, kps=None):
    """descs: per frame uint32 [n][words]; kps: per frame int [n][2] (x, y), or None.
    -> (d_desc [F][stride][words], d_kp [F][stride][4] or None, d_counts [F], counts)"""
    F = len(descs)
    buf = np.zeros((F, stride, words), dtype=np.uint32)
    for f, d in enumerate(descs):
        buf[f, :len(d)] = d
    counts = np.array([len(d) for d in descs], dtype=np.int32)
    d_kp = None
    if kps is not None:
        kp = np.zeros((F, stride), dtype=pg.KEYPOINT_DTYPE)
        for f, p in enumerate(kps):
            kp["x"][f, :len(p)] = p[:, 0]
            kp["y"][f, :len(p)] = p[:, 1]
        d_kp = torch.from_numpy(kp.view(np.int32).reshape(F, stride, 4)).to(DEV)
    return torch.from_numpy(buf.view(np.int32)).to(DEV), d_kp, torch.from_numpy(counts).to(DEV), counts


def _pairs(pl):
    return torch.tensor(np.asarray(pl, dtype=np.int32).reshape(-1, 2), device=DEV)


def _guide(guide):
    if guide is None:
        return None, None
    Fs, band = guide
    return torch.from_numpy(np.stack([np.asarray(f, dtype=np.float32).reshape(9) for f in Fs])).to(DEV), band


def run_knn(engine, dev, stride, words, pl, k, col, sentinel=77, max_count=None, guide=None):
    """pgx_knn_batch_dev, or pgx_knn_guided_batch_dev with guide = (F per pair, band), on upload()'s buffers
    -> idx, dist [M][stride][k], col [M][stride] or None (host arrays; what the call leaves alone holds the sentinel)"""
    d_desc, d_kp, d_counts, _ = dev
    M = len(pl)
    idx, dist = torch.full((M, stride, k), sentinel, **I32), torch.full((M, stride, k), sentinel, **I32)
    cnn = torch.full((M, stride), sentinel, **I32) if col else None
    d_pl = _pairs(pl)
    d_F, band = _guide(guide)
    torch.cuda.synchronize()
    if guide is None:
        engine.knn_batch_dev(d_desc, d_counts, stride, words, d_pl, M, k, idx, dist, cnn, max_count=max_count)
    else:
        engine.knn_guided_batch_dev(d_desc, d_kp, d_counts, stride, words, d_pl, M, d_F, band, k, idx, dist, cnn,
                                    max_count=max_count)
    engine.check_status()
    return idx.cpu().numpy(), dist.cpu().numpy(), (cnn.cpu().numpy() if col else None)


def run_nn(engine, dev, stride, words, pl, max_dist, ratio, cross, sentinel=77, guide=None, max_count=None):
    """pgx_match_nn_batch_dev, or pgx_match_guided_batch_dev with guide = (F per pair, band) -> lists [M][stride][3]"""
    d_desc, d_kp, d_counts, _ = dev
    M = len(pl)
    out = torch.full((M, stride, 3), sentinel, **I32)
    d_pl = _pairs(pl)
    d_F, band = _guide(guide)
    torch.cuda.synchronize()
    if guide is None:
        engine.match_nn_batch_dev(d_desc, d_counts, stride, words, d_pl, M, out, max_dist, ratio, cross, max_count=max_count)
    else:
        engine.match_guided_batch_dev(d_desc, d_kp, d_counts, stride, words, d_pl, M, d_F, band, out, max_dist, ratio, cross,
                                      max_count=max_count)
    engine.check_status()
    return out.cpu().numpy()


def run_match(engine, descs, pl, stride, max_count=None, sentinel=-7, wait=True):
    """pgx_match_batch_dev on 256-bit sets uploaded here -> lists [M][stride][3] on the host.
    wait=False: the device tensor right behind the launch, nothing synchronised (the caller's check_status does that); the
    launch is asynchronous, so its buffers are kept alive on this function."""
    d_desc, _, d_counts, _ = upload(stride, 8, descs)
    d_pl = _pairs(pl)
    d_out = torch.full((len(pl), stride, 3), sentinel, **I32)
    torch.cuda.synchronize()   # see pgx.h: "_dev" buffers must be ready on, or ordered against, the context's stream
    engine.match_batch_dev(d_desc, d_counts, stride, 8, d_pl, len(pl), d_out, max_count=max_count)
    if not wait:
        run_match.keepalive = (d_desc, d_counts, d_pl, d_out)
        return d_out
    engine.check_status()
    return d_out.cpu().numpy()


def oracle_detect(frame, dmap, pairs, T, radius, cap, raw_cap=None):
    """dewarp (dmap or None) -> gray -> detect -> NMS -> BRIEF by the oracle -> (kept keypoints, descriptors, raw hits).
    raw_cap: pgx_set_capacity's max_raw_per_frame -- NMS sees the first raw_cap hits in raster order; the count is the true one."""
    src = cref.apply_distortion(frame, dmap) if dmap is not None else frame
    g = cref.gray(src)
    raw = cref.detect(g, T)
    n_raw = len(raw)
    raw = raw[:raw_cap]
    kept = raw[cref.nms(raw, radius)][:cap]
    return kept, cref.brief(g, np.stack([kept["x"], kept["y"]], 1), pairs), n_raw


def run_detect(engine, frames, cap, sentinel=-7, words=8):
    """pgx_detect_batch_dev on host frames [F][H][W][4] with the engine's current parameters, nothing synchronised: the caller's
    check_status does that -> device (d_kp [F][cap][4], d_desc [F][cap][words], d_counts [F], d_nraw [F]), sentinel-filled"""
    F, H, W = frames.shape[:3]
    d_frames = torch.from_numpy(frames).to(DEV)
    out = (torch.full((F, cap, 4), sentinel, **I32), torch.full((F, cap, words), sentinel, **I32),
           torch.full((F,), sentinel, **I32), torch.full((F,), sentinel, **I32))
    torch.cuda.synchronize()
    engine.detect_batch_dev(d_frames, F, W, H, *out, cap)
    run_detect.keepalive = d_frames
    return out


def detect_equal(out, f, kept, edesc, n_raw, sentinel=-7):
    """frame f of run_detect's buffers against oracle_detect's triple, every field exact; the rows behind the list untouched"""
    kp, desc = out[0][f].cpu().numpy(), out[1][f].cpu().numpy()
    n = len(kept)
    assert int(out[3][f]) == n_raw and int(out[2][f]) == n, (f, int(out[3][f]), n_raw, int(out[2][f]), n)
    assert (kp[:n, 0] == kept["x"]).all() and (kp[:n, 1] == kept["y"]).all(), f
    assert (kp[:n, 2] == kept["fast_score"]).all(), f
    assert kp[:n, 3].view(np.float32).tobytes() == kept["value"].tobytes(), f
    assert (desc[:n].view(np.uint32) == edesc).all(), f
    assert (kp[n:] == sentinel).all() and (desc[n:] == sentinel).all(), f


def pairs_equal(got, exp):
    """got: [n][3] rows (k1, k2, dist); exp: the oracle's list (PAIR_DTYPE)"""
    return bool((got[:, 0] == exp["k1"]).all() and (got[:, 1] == exp["k2"]).all() and (got[:, 2] == exp["dist"]).all())
