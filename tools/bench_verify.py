"""Micro-benchmark of pgx_verify_pairs_dev, timed with HIP events on a stream of its own:
  (a) the bench job's shape: 64 frames at stride 4096, all 2016 pairs (a < b), n_samples = 256
  (b) 8 frames, 28 pairs, n_samples = 4096 (many samples per pair)
The frames are make_scene's (one keypoint per visible point, integer-rounded); every scene point has a random 256-bit
descriptor of which 20 bits are flipped per view, and the match lists are pgx_match_nn_batch_dev's over those descriptors
(max_dist 80: rows without a partner in the other frame are mostly rejected there, the rest is junk).  Writes
profiles/verify_<shape>.json (or --out DIR).  For the kernel split run it under
`rocprofv3 --kernel-trace --stats -- python tools/bench_verify.py`."""
import argparse
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, ROOT)
import geom_bench as gb  # noqa: E402
import photogrammetry_amd as pg  # noqa: E402
from geom_bench import DEV, F64, I32  # noqa: E402
from photogrammetry_amd import synth  # noqa: E402

WORDS, MAX_DIST, IP, MIN_IN, REFITS, SEED = 8, 80, 1.5, 24, 2, 1


def inputs(nf, n_points, arc_deg):
    """-> (scene, pairs, stride, d_kp, d_desc, d_counts, d_pairlist)"""
    s = synth.make_scene(n_points, nf, seed=1, arc_deg=arc_deg)
    rng = np.random.default_rng(0)
    base = rng.integers(0, 2**32, size=(n_points, WORDS), dtype=np.uint32)
    stride = n_points
    kp = np.zeros((nf, stride, 4), np.int32)
    desc = np.zeros((nf, stride, WORDS), np.uint32)
    for f in range(nf):
        n = len(s["kps"][f])
        kp[f, :n, 0], kp[f, :n, 1] = s["kps"][f]["x"], s["kps"][f]["y"]
        desc[f, :n] = synth.flip_bits(rng, base[s["point_id"][f]], 20)
    pairs = [(a, b) for a in range(nf) for b in range(a + 1, nf)]
    return (s, pairs, stride, torch.from_numpy(kp).to(DEV), torch.from_numpy(desc.view(np.int32)).to(DEV),
            torch.tensor(s["counts"].astype(np.int32), **I32), torch.tensor(np.asarray(pairs, np.int32), **I32))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=11)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--shapes", default="a,b")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles"))
    args = ap.parse_args()
    eng = pg.Engine(0)
    for name in args.shapes.split(","):
        nf, n_points, arc, ns = (64, 4096, 120.0, 256) if name == "a" else (8, 4096, 40.0, 4096)
        t0 = time.time()
        s, pairs, stride, d_kp, d_desc, d_c, d_pl = inputs(nf, n_points, arc)
        gen_s = time.time() - t0
        M = len(pairs)
        nn, out = torch.empty((M, stride, 3), **I32), torch.empty((M, stride, 3), **I32)
        Fd, F32 = torch.empty((M, 9), **F64), torch.empty((M, 9), dtype=torch.float32, device=DEV)
        stats, rep = torch.empty((M, 8), **I32), torch.empty(8, **I32)
        torch.cuda.synchronize()
        eng.match_nn_batch_dev(d_desc, d_c, stride, WORDS, d_pl, M, nn, MAX_DIST)
        eng.check_status()

        def call():
            eng.verify_pairs_dev(d_kp, nn, d_c, d_pl, M, stride, MAX_DIST, out, Fd, stats, rep, ns, IP, MIN_IN, REFITS, SEED, d_F32=F32)
        ms = gb.time_on_stream(eng, call, args.steps, args.warmup)
        st, report = stats.cpu().numpy(), rep.cpu().tolist()
        # truth: the share of kept rows that link the same scene point, and of true rows kept
        o, n_in = out.cpu().numpy(), nn.cpu().numpy()
        kept_true = kept = true_in = 0
        for m, (a, b) in enumerate(pairs):
            na = len(s["point_id"][a])
            r_in, r_out = n_in[m, :na], o[m, :na]
            ok_in = r_in[:, 1] >= 0
            true = np.zeros(na, bool)
            true[ok_in] = s["point_id"][a][r_in[ok_in, 0]] == s["point_id"][b][r_in[ok_in, 1]]
            k = r_out[:, 1] >= 0
            kept += int(k.sum())
            kept_true += int((k & true).sum())
            true_in += int(true.sum())
        evals = int(ns) * int(st[:, 0].sum())
        med = float(np.median(ms))
        rec = dict(shape=name, frames=nf, pairs=M, stride=stride, n_samples=ns, inlier_px=IP, min_inliers=MIN_IN, refit_iters=REFITS,
                   candidates=int(st[:, 0].sum()), candidates_mean=float(st[:, 0].mean()), report=report,
                   refits_kept=int(st[:, 5].sum()), kept_rows=kept, kept_rows_true=kept_true, true_rows_in=true_in,
                   predicate_evaluations_scoring=evals, evaluations_per_s_whole_call=evals / (med * 1e-3), steps=args.steps,
                   ms_median=med, ms_min=float(ms.min()), ms_max=float(ms.max()), input_generation_s=round(gen_s, 1))
        gb.write_record(rec, args.out, "verify")
    eng.close()


if __name__ == "__main__":
    main()
