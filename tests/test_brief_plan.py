"""CPU test of the row-sorted sample plan that pgx_set_brief_pairs derives from a 256-pair BRIEF table
(photogrammetry_amd/csrc/pgx_brief_plan.h, read by brief_256 in csrc/k_brief.hip).

The builder is plain host C++ in a header; tests/brief_plan_driver.cpp is a stand-alone program around it, built here with
-fsanitize=address,undefined and run once per table, so every table below is also a sanitizer run of the builder.

Checked per table: the plan's 512 samples are a permutation of the table's 512 end points (1024 offsets) in non-decreasing
(dy, dx) order, and every pair's two positions point back at that pair's own offsets, first end point in the low half."""
import os
import subprocess

import numpy as np
import pytest

import photogrammetry_amd as pg

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
I32 = np.iinfo(np.int32)


def _tables():
    rng = np.random.default_rng(11)
    wild = rng.integers(-60, 61, (256, 4)).astype(np.int32)
    wild[::9] = [I32.min, I32.max, I32.max, I32.min]          # the extremes of the ABI's int32 offsets
    wild[1::9, 0] = 1 << 20                                   # far beyond any image
    wild[2::9, 3] = -(1 << 30)
    wild[3::9, 2:] = wild[3::9, :2]                           # a pair whose end points coincide
    wild[4::9] = wild[4]                                      # repeated pairs
    return {
        "seed0": pg.make_brief_pairs(0, 50, 256),
        "seed7": pg.make_brief_pairs(7, 50, 256),
        "all_equal": np.full((256, 4), 3, np.int32),
        "negative_and_huge": wild,
    }


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("brief_plan") / "brief_plan_driver")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-o", exe, os.path.join(ROOT, "tests", "brief_plan_driver.cpp")],
                   check=True, capture_output=True, text=True, timeout=300)
    return exe


@pytest.mark.parametrize("name", ["seed0", "seed7", "all_equal", "negative_and_huge"])
def test_plan_is_sorted_permutation_and_positions_point_back(driver, tmp_path, name):
    pairs = _tables()[name]
    path = str(tmp_path / "pairs.bin")
    pairs.tofile(path)
    run = subprocess.run([driver, path], capture_output=True, timeout=60)
    assert run.returncode == 0 and not run.stderr, run.stderr.decode(errors="replace")[-2000:]
    plan = np.frombuffer(run.stdout, dtype=np.int32)
    assert plan.size == 1024 + 256
    smp = plan[:1024].reshape(512, 2).astype(np.int64)        # (dx, dy) in plan order
    pos = plan[1024:].view(np.uint32)
    ends = pairs.reshape(512, 2).astype(np.int64)             # end point 2p = (x1, y1), 2p + 1 = (x2, y2)

    # non-decreasing (dy, dx)
    key = list(zip(smp[:, 1].tolist(), smp[:, 0].tolist()))
    assert key == sorted(key)
    # a permutation of the table's end points, as multisets
    assert sorted(map(tuple, smp.tolist())) == sorted(map(tuple, ends.tolist()))
    # positions: in range, nothing but the two 9-bit fields set, every slot used exactly once, and each points at its own offsets
    assert (pos & ~np.uint32(0x01FF01FF) == 0).all()
    p1, p2 = (pos & 0x1FF).astype(np.int64), (pos >> 16).astype(np.int64)
    assert sorted(np.concatenate([p1, p2]).tolist()) == list(range(512))
    assert (smp[p1] == pairs[:, 0:2]).all() and (smp[p2] == pairs[:, 2:4]).all()
