"""CPU test: photogrammetry_amd.cloud.write_mesh_ply writes a binary PLY with a face element that read_mesh_ply gives back bit
for bit; write_ply's files are what they were."""
import numpy as np
import pytest

import mesh_ref as ref
from photogrammetry_amd import cloud


def a_mesh():
    p = ref.plane_case(4.01)
    rgba8 = np.random.default_rng(3).integers(0, 2**32, p["depth"].shape, dtype=np.uint32)
    return ref.mesh(p["xyz"], p["src"], p["depth"], p["views"], 5, p["P"], ref.CELL, ref.ORIGIN, rgba8=rgba8)


@pytest.mark.parametrize("with_normal", [False, True])
@pytest.mark.parametrize("with_colour", [False, True])
def test_mesh_ply_round_trip(tmp_path, with_normal, with_colour):
    m = a_mesh()
    assert len(m["tri"]) > 1000 and (m["rgba8"] != 0).any()
    xyz = m["xyz"].copy()
    xyz[0] = [np.nextafter(1.0, 2.0), -0.0, 1e-300]              # bits a text file would lose
    path = str(tmp_path / "m.ply")
    cloud.write_mesh_ply(path, xyz, m["tri"], m["normal"] if with_normal else None, m["rgba8"] if with_colour else None)
    head = open(path, "rb").read(600).split(b"end_header\n")[0].decode("ascii").split("\n")
    assert head[:3] == ["ply", "format binary_little_endian 1.0", "element vertex %d" % len(xyz)]
    assert head[-3:-1] == ["element face %d" % len(m["tri"]), "property list uchar int vertex_indices"]
    gx, gt, gn, gc = cloud.read_mesh_ply(path)
    assert ref.bits(gx) == ref.bits(xyz) and gt.dtype == np.int32 and ref.bits(gt) == ref.bits(m["tri"])
    assert (gn is None) == (not with_normal) and (gc is None) == (not with_colour)
    assert gn is None or (gn.dtype == np.float32 and ref.bits(gn) == ref.bits(m["normal"]))
    assert gc is None or (gc.dtype == np.uint32 and ref.bits(gc) == ref.bits(m["rgba8"]))
    # the vertex element is write_ply's: the same bytes up to the header's face lines
    cloud.write_ply(str(tmp_path / "c.ply"), xyz, m["normal"] if with_normal else None, m["rgba8"] if with_colour else None)
    body = open(str(tmp_path / "c.ply"), "rb").read().split(b"end_header\n", 1)[1]
    assert open(path, "rb").read().split(b"end_header\n", 1)[1].startswith(body)


def test_mesh_ply_empty_and_bad_indices(tmp_path):
    path = str(tmp_path / "e.ply")
    cloud.write_mesh_ply(path, np.zeros((0, 3)), np.zeros((0, 3), np.int32))
    gx, gt, gn, gc = cloud.read_mesh_ply(path)
    assert gx.shape == (0, 3) and gt.shape == (0, 3) and gn is None and gc is None
    with pytest.raises(ValueError):
        cloud.write_mesh_ply(path, np.zeros((2, 3)), np.array([[0, 1, 2]], np.int32))
    cloud.write_ply(path, np.zeros((2, 3)))
    with pytest.raises(ValueError):
        cloud.read_mesh_ply(path)
