"""What tools/bench_triangulate.py, bench_bundle.py and bench_register.py share: the scene whose tracks are cut to random runs,
the upload of a track-graph problem, the timing loop on a stream of its own, and the record's way to stdout and disk."""
import json
import os

import numpy as np
import torch

from photogrammetry_amd import synth

DEV = "cuda:0"
I32 = dict(dtype=torch.int32, device=DEV)
F64 = dict(dtype=torch.float64, device=DEV)


def cut_scene(rng, nf, n_points=8000):
    """make_scene's nf frames on a 120-degree arc; every point's views cut to one run of 2..64 nodes, its length and then its
    start drawn from rng (the recorded shapes depend on that order).  -> (scene, offsets, nodes, point of each track)"""
    s = synth.make_scene(n_points, nf, seed=1, arc_deg=120.0)
    return (s,) + synth.cut_tracks(s, (2, 65), seed=rng)


def device_inputs(kps, off, nodes, **arrays):
    """synth.device_tracks' buffers, every further host array uploaded under its name, and the track lengths"""
    d = synth.device_tracks(kps, off, nodes, device=DEV)
    d.update({k: torch.from_numpy(np.ascontiguousarray(v)).to(DEV) for k, v in arrays.items()})
    d["lengths"] = np.diff(off)
    return d


def time_on_stream(eng, call, steps, warmup):
    """warmup calls on the context's stream, then steps calls on a stream of its own, one HIP event pair each -> ms [steps]"""
    for _ in range(warmup):
        call()
    eng.check_status()
    stream = torch.cuda.Stream()     # a stream of its own: handle 0 would mean the context's own stream again
    eng.set_stream(stream.cuda_stream)
    times = []
    for _ in range(steps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(stream)
        call()
        b.record(stream)
        b.synchronize()
        times.append(a.elapsed_time(b))
    eng.set_stream(0)
    eng.check_status()
    return np.array(times)


def write_record(rec, out_dir, stem):
    """one JSON line on stdout and <out_dir>/<stem>_<shape>.json"""
    print(json.dumps(rec))
    os.makedirs(out_dir, exist_ok=True)
    with open(os.path.join(out_dir, "%s_%s.json" % (stem, rec["shape"])), "w") as fh:
        json.dump(rec, fh, indent=1)
