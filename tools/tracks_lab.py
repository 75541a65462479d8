#!/usr/bin/env python3
"""Developer tool (GPU box): the track graph alone on the bench job's own match lists.

    python tools/tracks_lab.py [--frames 64] [--reps 50] [--max-dist 64] [--gates 48,32,24,16 [--gates 48 ...]] [--out FILE]

Runs detect + match of the bench sequence once, then pgx_tracks_dev `reps` times on the resident lists and prints the
average time per call (HIP events through torch on the job's stream), the summary, a sha256 of the result arrays (to compare
builds bit for bit) and the oracle check.  Under `rocprofv3 --kernel-trace --stats` the k_trk_* rows give the split.
Every --gates G (comma-separated, "" = no gates) adds one line for the split mode (pgx_tracks_split_dev) on the same lists:
time per call, the summary with the nodes per level, sha256 (of the same arrays plus the 16-slot summary, so it never equals
the pgx_tracks_dev line's digest), and the check against tests/tracks_split_ref.py.  --out writes
all lines as one JSON list."""
import argparse
import hashlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--max-dist", type=int, default=64)
    ap.add_argument("--no-check", action="store_true")
    ap.add_argument("--gates", action="append", default=[], help="comma-separated refinement gates (repeatable; '' = none)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import numpy as np
    import torch
    import bench
    import photogrammetry_amd as pg
    from photogrammetry_amd import dist as pdist
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(0)
    W, H, NKP = bench.W, bench.H, bench.NKP
    F = args.frames
    e = pg.Engine(0)
    e.set_brief_pairs(pg.make_brief_pairs(0, 50, 256))
    e.set_detect_params(bench.THRESH, bench.RADIUS)
    e.set_capacity(1 << 18, NKP)
    e.set_dewarp_map(pg.build_dewarp_map(W, H, [3e-4, 1e-7, 0, 0, 0]))
    pl = pdist.all_pairs(F)
    stream = torch.cuda.Stream(device=dev)
    job = pdist.ShardedSequence(e, W, H, F, pl, NKP, 8, dev, stream=stream, tracks={"max_dist": args.max_dist, "min_len": 2})
    with torch.cuda.stream(stream):
        base = torch.from_numpy(bench.base_frame(W, H, 4321)).to(dev)
        d_frames = bench.roll_frames(torch, base, [(3 * i, i) for i in range(F)])
    torch.cuda.synchronize()
    job.step(d_frames)
    e.check_status()
    counts = job.counts()
    m_host = None if args.no_check else job.out_all.cpu().numpy()

    def timed(fn):
        with torch.cuda.stream(stream):
            for _ in range(3):
                fn()
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record(stream)
            for _ in range(args.reps):
                fn()
            t1.record(stream)
        torch.cuda.synchronize()
        e.check_status()
        return t0.elapsed_time(t1) / args.reps

    def digest(nt, nn, summary=None):
        h = hashlib.sha256()
        for t in (job.trk_offsets[:nt + 1], job.trk_nodes[:nn], job.track_of) + ((summary,) if summary is not None else ()):
            h.update(t.cpu().numpy().tobytes())
        return h.hexdigest()

    ms = timed(lambda: job._build_tracks(0))
    summ = job.track_summary()
    nt, nn = summ["n_tracks"], summ["n_nodes"]
    res = {"mode": "tracks_dev", "ms_per_call": ms, "frames": F, "image_pairs": len(pl), "entries": len(pl) * NKP,
           "max_dist": args.max_dist, "summary": summ, "sha256": digest(nt, nn)}
    if not args.no_check:
        from oracle import tracks_np
        e_off, e_nodes, e_tof, e_s = tracks_np.tracks_arrays(counts, pl, m_host, NKP, args.max_dist, 2)
        res["oracle_ok"] = bool(summ == e_s and (job.trk_offsets[:nt + 1].cpu().numpy() == e_off).all()
                                and (job.trk_nodes[:nn].cpu().numpy() == e_nodes).all() and (job.track_of.cpu().numpy() == e_tof).all())
    print(json.dumps(res))
    lines = [res]
    if args.gates:
        sys.path.insert(0, os.path.join(ROOT, "tests"))
        import tracks_split_ref as ref
        s16 = torch.zeros(16, dtype=torch.int32, device=dev)
        for spec in args.gates:
            gates = [int(g) for g in spec.split(",") if g.strip()]

            def split():
                e.tracks_split_dev(job.out_bufs[0], job.trk_counts[0], job.trk_pairlist, job.world * job.ps, job.world * job.fs,
                                   job.nkp, F, args.max_dist, gates, 2, job.track_of, job.trk_offsets, job.trk_nodes, s16,
                                   d_frame_ids=job.trk_frame_ids)

            ms = timed(split)
            v = s16.cpu().tolist()
            nt, nn = v[0], v[1]
            summ = {"n_tracks": v[0], "n_nodes": v[1], "dropped": v[2], "dropped_nodes": v[3], "edges": v[4], "longest": v[5],
                    "largest_dropped": v[6], "per_level": v[8:9 + len(gates)]}
            r = {"mode": "tracks_split_dev", "gates": gates, "ms_per_call": ms, "max_dist": args.max_dist, "summary": summ,
                 "sha256": digest(nt, nn, s16)}
            if not args.no_check:
                e_off, e_nodes, e_tof, e_s = ref.arrays(counts, pl, m_host, NKP, args.max_dist, gates, 2)
                r["reference_ok"] = bool(v == ref.summary16(e_s) and (job.trk_offsets[:nt + 1].cpu().numpy() == e_off).all()
                                         and (job.trk_nodes[:nn].cpu().numpy() == e_nodes).all()
                                         and (job.track_of.cpu().numpy() == e_tof).all())
            print(json.dumps(r))
            lines.append(r)
    if args.out:
        with open(args.out, "w") as fh:
            json.dump(lines, fh, indent=1)
    e.close()


if __name__ == "__main__":
    main()
