"""Micro-benchmark of pgx_init_pair_dev, timed with HIP events on a stream of its own, on
tools/bench_verify.py's scenes and timing loop:
  (a) the bench job's shape: 64 frames at stride 4096, all 2016 pairs (a < b)
  (b) 8 frames, 28 pairs
The inputs are what the stage is meant to get: pgx_match_nn_batch_dev's lists verified by pgx_verify_pairs_dev (its d_out and
d_F), and the scene's intrinsics.  Writes profiles/init_pair_<shape>.json (or --out DIR).  For the kernel split run it under
`rocprofv3 --kernel-trace --stats -- python tools/bench_init_pair.py --shapes a`."""
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
from bench_verify import IP, MAX_DIST, MIN_IN, REFITS, SEED, WORDS, inputs  # noqa: E402
from geom_bench import DEV, F64, I32  # noqa: E402

ANGLE, FRONT, MIN_POINTS = 2.0, 0.7, 30


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
        nn, ver = torch.empty((M, stride, 3), **I32), torch.empty((M, stride, 3), **I32)
        Fd, vstats, vrep = torch.empty((M, 9), **F64), torch.empty((M, 8), **I32), torch.empty(8, **I32)
        d_K = torch.from_numpy(np.ascontiguousarray(s["K"], np.float64)).to(DEV)
        Rt_pair, stats, sigma = torch.empty((M, 12), **F64), torch.empty((M, 8), **I32), torch.empty(M, **F64)
        Rt_out, P_out = torch.empty((nf, 12), **F64), torch.empty((nf, 12), **F64)
        fixed, reg, rep = torch.empty(nf, **I32), torch.empty(nf, **I32), torch.empty(8, **I32)
        torch.cuda.synchronize()
        eng.match_nn_batch_dev(d_desc, d_c, stride, WORDS, d_pl, M, nn, MAX_DIST)
        eng.verify_pairs_dev(d_kp, nn, d_c, d_pl, M, stride, MAX_DIST, ver, Fd, vstats, vrep, ns, IP, MIN_IN, REFITS, SEED)
        eng.check_status()

        def call():
            eng.init_pair_dev(d_kp, ver, d_c, d_pl, M, nf, stride, nf, MAX_DIST, Fd, d_K, Rt_pair, stats, Rt_out, P_out, fixed, reg, rep,
                              ANGLE, FRONT, MIN_POINTS, d_sigma=sigma)
        ms = gb.time_on_stream(eng, call, args.steps, args.warmup)
        st, report, sg = stats.cpu().numpy(), rep.cpu().tolist(), sigma.cpu().numpy()
        ms_star = report[6]
        a, b = pairs[ms_star] if ms_star >= 0 else (-1, -1)
        rot = direction = float("nan")
        if ms_star >= 0:                                       # the chosen pair against the scene's truth
            Ra, ta = s["Rt"][a, :9].reshape(3, 3), s["Rt"][a, 9:]
            Rb, tb = s["Rt"][b, :9].reshape(3, 3), s["Rt"][b, 9:]
            R_true = Rb @ Ra.T
            t_true = tb - R_true @ ta
            got = Rt_out.cpu().numpy()[b]
            R, t = got[:9].reshape(3, 3), got[9:]
            rot = float(np.degrees(np.arccos(np.clip((np.trace(R @ R_true.T) - 1.0) / 2.0, -1.0, 1.0))))
            direction = float(np.degrees(np.arccos(np.clip(t @ t_true / np.linalg.norm(t_true), -1.0, 1.0))))
        med = float(np.median(ms))
        rows = int(st[:, 0].sum())
        rec = dict(shape=name, frames=nf, pairs=M, stride=stride, min_angle_deg=ANGLE, min_front_frac=FRONT, min_points=MIN_POINTS,
                   verify_report=vrep.cpu().tolist(), report=report, candidates=rows, candidates_mean=float(st[:, 0].mean()),
                   sigma_ratio_min=float(np.nanmin(sg)) if np.isfinite(sg).any() else None, chosen_pair=[int(a), int(b)],
                   chosen_rotation_error_deg=rot, chosen_direction_error_deg=direction, scores=4 * rows,
                   scores_per_s_whole_call=4 * rows / (med * 1e-3), steps=args.steps, ms_median=med, ms_min=float(ms.min()),
                   ms_max=float(ms.max()), input_generation_s=round(gen_s, 1))
        gb.write_record(rec, args.out, "init_pair")
    eng.close()


if __name__ == "__main__":
    main()
