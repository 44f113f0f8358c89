"""Mesh files (numpy only).  write_ply: binary little-endian PLY of a triangle mesh, as TsdfVolume.fetchMesh returns it."""
import numpy as np


def _host(a):
    return a.detach().cpu().numpy() if hasattr(a, "detach") else np.asarray(a)


def write_ply(path, vertices, triangles, normals=None):
    """vertices [n, 3 or 4] float32 (a 4th column is dropped), triangles [m, 3] (u)int32 vertex indices, normals [n, 3 or 4] or None.
    Layout: per vertex 3 (6 with normals) little-endian f32; per face one byte 3 and three little-endian int32."""
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
    header += ["element face %d" % t.shape[0], "property list uchar int vertex_indices", "end_header"]
    faces = np.empty(t.shape[0], dtype=[("n", "u1"), ("i", "<i4", (3,))])
    faces["n"] = 3
    faces["i"] = t
    with open(path, "wb") as f:
        f.write(("\n".join(header) + "\n").encode("ascii"))
        f.write(v.tobytes())
        f.write(faces.tobytes())
