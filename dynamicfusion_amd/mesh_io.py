"""Mesh files (numpy only).  write_ply: binary little-endian PLY of a triangle mesh, as TsdfVolume.fetchMesh returns it."""
import numpy as np


def _host(a):
    return a.detach().cpu().numpy() if hasattr(a, "detach") else np.asarray(a)


def write_ply(path, vertices, triangles, normals=None, colors=None):
    """vertices [n, 3 or 4] float32 (a 4th column is dropped), triangles [m, 3] (u)int32 vertex indices, normals [n, 3 or 4] or None,
    colors [n, 3 or 4] uint8 in r, g, b order (a 4th column is dropped) or None.
    Layout: per vertex 3 (6 with normals) little-endian f32, then with colors 3 bytes red, green, blue; per face one byte 3 and three
    little-endian int32.  Without colors the file is what it was before colors existed, byte for byte."""
    v = np.ascontiguousarray(_host(vertices)[:, :3], "<f4")
    t = _host(triangles)
    if t.ndim != 2 or t.shape[1] != 3:
        raise ValueError("triangles must be [m, 3], got %s" % (t.shape,))
    t = np.ascontiguousarray(t).astype("<i4", copy=False) if t.dtype.itemsize != 4 else np.ascontiguousarray(t).view("<i4")
    props = ["x", "y", "z"]
    if normals is not None:
        nrm = np.ascontiguousarray(_host(normals)[:, :3], "<f4")
        if nrm.shape[0] != v.shape[0]:
            raise ValueError("%d normals for %d vertices" % (nrm.shape[0], v.shape[0]))
        v = np.ascontiguousarray(np.concatenate([v, nrm], 1))
        props += ["nx", "ny", "nz"]
    header = ["ply", "format binary_little_endian 1.0", "element vertex %d" % v.shape[0]]
    header += ["property float %s" % p for p in props]
    vertex_bytes = v.tobytes()
    if colors is not None:
        col = _host(colors)
        if col.dtype != np.uint8 or col.ndim != 2 or col.shape[1] not in (3, 4) or col.shape[0] != v.shape[0]:
            raise ValueError("colors must be uint8 [%d, 3 or 4], got %s %s" % (v.shape[0], col.dtype, col.shape))
        rec = np.empty(v.shape[0], dtype=[("f", "<f4", (v.shape[1],)), ("c", "u1", (3,))])
        rec["f"] = v
        rec["c"] = col[:, :3]
        vertex_bytes = rec.tobytes()
        header += ["property uchar %s" % p for p in ("red", "green", "blue")]
    header += ["element face %d" % t.shape[0], "property list uchar int vertex_indices", "end_header"]
    faces = np.empty(t.shape[0], dtype=[("n", "u1"), ("i", "<i4", (3,))])
    faces["n"] = 3
    faces["i"] = t
    with open(path, "wb") as f:
        f.write(("\n".join(header) + "\n").encode("ascii"))
        f.write(vertex_bytes)
        f.write(faces.tobytes())
