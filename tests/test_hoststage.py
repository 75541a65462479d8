"""CPU test of the staging images of the twenty host forms on photogrammetry_amd/csrc/pgx_hoststage.h: the input image that
pgx_triangulate_tracks, pgx_bundle_adjust, pgx_register_frames, pgx_verify_pair, pgx_relative_pose, pgx_match, pgx_knn,
pgx_knn_guided, pgx_match_batch and, added since, pgx_track_consensus, pgx_vocab_train, pgx_select_pairs, pgx_depth_maps,
pgx_depth_fuse, pgx_dense_views, pgx_rgba8_batch, pgx_cloud_merge, pgx_mesh, pgx_mesh_clean and pgx_mesh_decimate pack and
upload in one copy, and the output image they download from.

The header is plain host C++; tests/hoststage_driver.cpp is a stand-alone program around it, built here with
-fsanitize=address,undefined and run once per host form.  It hands the packer a buffer of exactly total() bytes and sources
of exactly their sizes, so every run is also a sanitizer run of the packer.

A limit of this test: only the lists that the forms share (tracks_in, pair_in, two_sets_in, batch_in, knn_out, mesh_in,
mesh_out) are the header's own code.  Every other form declares its outputs, pgx_relative_pose its F and K, and pgx_match_batch computes its S
and its referenced frames, inside pgx_api.hip, which needs HIP; the nine later forms declare both of their lists there
(pgx_track_consensus takes its inputs from tracks_in).  The driver repeats those word for word, so a size edited in
pgx_api.hip alone is caught by tests/test_gpu_host_forms.py (every output bit for bit against the device form), not here.

Checked per form, for its section lists as the form declares them: every offset is 256-aligned, the sections are disjoint and
in declaration order and the total is the sum of the aligned sizes; the packed image equals one laid out naively in the
driver, byte for byte, with every byte that no source covers zero; an absent section gives a null device pointer and an
absent output no download; an output with nothing to download gives none, and so does a list section with a null source
and at_least = cap + 1, which pgx_depth_fuse, pgx_cloud_merge and the three mesh forms fetch themselves once the report, the
first download of their output image, has told them how many rows there are.

Sizes: n_frames 1 and 3 with counts {0, 5, 2} (stride from the largest count); n_tracks 0, 1 and 7 with n_nodes 0 and 19;
(n1, n2) in (0, 0), (0, 4), (4, 0), (5, 3); max_iters 0 and 20; every optional section once present and once absent.
The matchers: (n1, n2) in (0, 4), (4, 0), (5, 3) with words 1 and 8, k 1 and 2, col_nn present and absent, the keypoints and
F present (pgx_knn_guided) and absent (pgx_match, pgx_knn); the batch with 3 frames of {0, 5, 2} rows and the pair lists {},
{(1, 2)}, {(1, 2), (2, 1)}, and with a fourth frame of 9 rows that no pair names, whose source is null and which must
leave S at 5.
The later forms: R in 0, 1 and 3 (pgx_cloud_merge and pgx_mesh, which refuse 0: 1 and 3); n_in and n_tracks in 0, 1 and 7;
max_points, max_vertices, max_tris and max_pairs in 0 and 5; W x H of 1 x 1 and 5 x 3; the vocabulary forms with F 1 and 3,
stride 1 and 5, V 1 and 7; pgx_rgba8_batch with 8 and 4 bytes a source pixel; every optional section (cost, warp, planes,
agree, scores, track_flags, refs, pair_counts, rgba8, pt_normal, cell_of; the per-track outputs of pgx_track_consensus and
ref_stats as null destinations) once present and once absent, in every combination within a form.
pgx_mesh_clean and pgx_mesh_decimate (one list: they differ in the name of the second per-vertex map): 0, 1 and 7 vertices, 0, 1
and 5 triangles, capacities of 0, 1 and more rows than the input has (9 vertices, 11 triangles), vertex_map and the second map
present and absent in every combination, the report first."""
import os
import subprocess

import pytest

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("hoststage") / "hoststage_driver")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-o", exe, os.path.join(ROOT, "tests", "hoststage_driver.cpp")],
                   check=True, capture_output=True, text=True, timeout=300)
    return exe


@pytest.mark.parametrize("form", ["triangulate_tracks", "bundle_adjust", "register_frames", "verify_pair", "relative_pose",
                                  "match", "knn", "knn_guided", "match_batch", "track_consensus", "vocab_train", "select_pairs",
                                  "depth_maps", "depth_fuse", "dense_views", "rgba8_batch", "cloud_merge", "mesh", "mesh_clean",
                                  "mesh_decimate"])
def test_images_match_the_naive_layout(driver, form):
    run = subprocess.run([driver, form], capture_output=True, text=True, timeout=60)
    assert run.returncode == 0 and not run.stderr, run.stderr[-2000:]
    assert run.stdout.startswith("ok ") and int(run.stdout.split()[1]) > 50
