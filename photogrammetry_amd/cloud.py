"""The merged cloud as a file: binary little-endian PLY with float64 positions, optional float32 normals and optional
8-bit colours (the layout of pgx_cloud_merge's outputs), and the reader that gives the same arrays back bit for bit; the mesh
of pgx_mesh the same way, with a face element (write_mesh_ply, read_mesh_ply)."""
import numpy as np


def _dtype(normal, colour):
    fields = [("x", "<f8"), ("y", "<f8"), ("z", "<f8")]
    if normal:
        fields += [("nx", "<f4"), ("ny", "<f4"), ("nz", "<f4")]
    if colour:
        fields += [("red", "u1"), ("green", "u1"), ("blue", "u1"), ("alpha", "u1")]
    return np.dtype(fields)


_PLY_TYPE = {"<f8": "double", "<f4": "float", "u1": "uchar", "|u1": "uchar"}


def write_ply(path, xyz, normal=None, rgba8=None):
    """xyz [n][3] float64, normal [n][3] float32 or None, rgba8 [n] uint32 (channel c in bits 8 c .. 8 c + 7) or None"""
    xyz = np.ascontiguousarray(xyz, dtype=np.float64).reshape(-1, 3)
    n = len(xyz)
    dt = _dtype(normal is not None, rgba8 is not None)
    rows = np.zeros(n, dtype=dt)
    rows["x"], rows["y"], rows["z"] = xyz[:, 0], xyz[:, 1], xyz[:, 2]
    if normal is not None:
        nm = np.ascontiguousarray(normal, dtype=np.float32).reshape(n, 3)
        rows["nx"], rows["ny"], rows["nz"] = nm[:, 0], nm[:, 1], nm[:, 2]
    if rgba8 is not None:
        c = np.ascontiguousarray(rgba8, dtype=np.uint32).reshape(n)
        for k, name in enumerate(("red", "green", "blue", "alpha")):
            rows[name] = (c >> np.uint32(8 * k)) & np.uint32(255)
    head = ["ply", "format binary_little_endian 1.0", "element vertex %d" % n]
    head += ["property %s %s" % (_PLY_TYPE[dt[name].str], name) for name in dt.names]
    with open(path, "wb") as f:
        f.write(("\n".join(head + ["end_header"]) + "\n").encode("ascii"))
        f.write(rows.tobytes())


_FACE = np.dtype([("n", "u1"), ("v", "<i4", (3,))])


def write_mesh_ply(path, xyz, tri, normal=None, rgba8=None):
    """A triangle mesh (the layout of pgx_mesh's outputs) as binary little-endian PLY: the vertex element of write_ply, then a face
    element of vertex-index lists.  xyz [n][3] float64, tri [t][3] int32 (every index in [0, n)), normal [n][3] float32 or None,
    rgba8 [n] uint32 or None"""
    xyz = np.ascontiguousarray(xyz, dtype=np.float64).reshape(-1, 3)
    tri = np.ascontiguousarray(tri, dtype=np.int32).reshape(-1, 3)
    n = len(xyz)
    if len(tri) and (tri.min() < 0 or tri.max() >= n):
        raise ValueError("a triangle names a vertex outside [0, %d)" % n)
    dt = _dtype(normal is not None, rgba8 is not None)
    rows = np.zeros(n, dtype=dt)
    rows["x"], rows["y"], rows["z"] = xyz[:, 0], xyz[:, 1], xyz[:, 2]
    if normal is not None:
        nm = np.ascontiguousarray(normal, dtype=np.float32).reshape(n, 3)
        rows["nx"], rows["ny"], rows["nz"] = nm[:, 0], nm[:, 1], nm[:, 2]
    if rgba8 is not None:
        c = np.ascontiguousarray(rgba8, dtype=np.uint32).reshape(n)
        for k, name in enumerate(("red", "green", "blue", "alpha")):
            rows[name] = (c >> np.uint32(8 * k)) & np.uint32(255)
    faces = np.zeros(len(tri), dtype=_FACE)
    faces["n"], faces["v"] = 3, tri
    head = ["ply", "format binary_little_endian 1.0", "element vertex %d" % n]
    head += ["property %s %s" % (_PLY_TYPE[dt[name].str], name) for name in dt.names]
    head += ["element face %d" % len(tri), "property list uchar int vertex_indices"]
    with open(path, "wb") as f:
        f.write(("\n".join(head + ["end_header"]) + "\n").encode("ascii"))
        f.write(rows.tobytes())
        f.write(faces.tobytes())


def read_mesh_ply(path):
    """A file of write_mesh_ply -> (xyz [n][3] float64, tri [t][3] int32, normal [n][3] float32 or None, rgba8 [n] uint32 or None)"""
    with open(path, "rb") as f:
        data = f.read()
    end = data.index(b"end_header\n") + len(b"end_header\n")
    lines = data[:end].decode("ascii").split("\n")
    if lines[0] != "ply" or lines[1] != "format binary_little_endian 1.0":
        raise ValueError("not a binary little-endian PLY file")
    n = int([ln for ln in lines if ln.startswith("element vertex ")][0].split()[2])
    faces = [ln for ln in lines if ln.startswith("element face ")]
    if not faces or "property list uchar int vertex_indices" not in lines:
        raise ValueError("not a file of write_mesh_ply: no face element of vertex-index lists")
    t = int(faces[0].split()[2])
    names = [ln.split()[2] for ln in lines if ln.startswith("property ") and not ln.startswith("property list ")]
    dt = _dtype("nx" in names, "red" in names)
    if list(dt.names) != names:
        raise ValueError("not a file of write_mesh_ply: properties %s" % names)
    rows = np.frombuffer(data, dtype=dt, count=n, offset=end)
    fc = np.frombuffer(data, dtype=_FACE, count=t, offset=end + n * dt.itemsize)
    if t and (fc["n"] != 3).any():
        raise ValueError("not a file of write_mesh_ply: a face that is no triangle")
    xyz = np.stack([rows["x"], rows["y"], rows["z"]], 1)
    normal = np.stack([rows["nx"], rows["ny"], rows["nz"]], 1) if "nx" in names else None
    rgba8 = None
    if "red" in names:
        rgba8 = sum(rows[name].astype(np.uint32) << np.uint32(8 * k) for k, name in enumerate(("red", "green", "blue", "alpha")))
    return xyz, np.array(fc["v"], dtype=np.int32).reshape(t, 3), normal, rgba8


def read_ply(path):
    """A file of write_ply -> (xyz [n][3] float64, normal [n][3] float32 or None, rgba8 [n] uint32 or None)"""
    with open(path, "rb") as f:
        data = f.read()
    end = data.index(b"end_header\n") + len(b"end_header\n")
    lines = data[:end].decode("ascii").split("\n")
    if lines[0] != "ply" or lines[1] != "format binary_little_endian 1.0":
        raise ValueError("not a binary little-endian PLY file")
    n = int([ln for ln in lines if ln.startswith("element vertex ")][0].split()[2])
    names = [ln.split()[2] for ln in lines if ln.startswith("property ")]
    dt = _dtype("nx" in names, "red" in names)
    if list(dt.names) != names:
        raise ValueError("not a file of write_ply: properties %s" % names)
    rows = np.frombuffer(data, dtype=dt, count=n, offset=end)
    xyz = np.stack([rows["x"], rows["y"], rows["z"]], 1)
    normal = np.stack([rows["nx"], rows["ny"], rows["nz"]], 1) if "nx" in names else None
    rgba8 = None
    if "red" in names:
        rgba8 = sum(rows[name].astype(np.uint32) << np.uint32(8 * k) for k, name in enumerate(("red", "green", "blue", "alpha")))
    return xyz, normal, rgba8
