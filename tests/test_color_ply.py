"""mesh_io.write_ply with vertex colours: the file read back (header, byte layout, colours), and the files without colours, which stay
byte for byte what the writer produced before it knew colours."""
import hashlib

import numpy as np
import pytest

import mesh_ref as R
from dynamicfusion_amd import mesh_io


def read_ply(raw):
    head, body = raw.split(b"end_header\n", 1)
    lines = head.decode("ascii").split("\n")
    assert lines[0] == "ply" and lines[1] == "format binary_little_endian 1.0" and lines[-1] == ""
    nv = int([l for l in lines if l.startswith("element vertex")][0].split()[-1])
    nf = int([l for l in lines if l.startswith("element face")][0].split()[-1])
    i_face = lines.index("element face %d" % nf)
    props = [tuple(l.split()[1:]) for l in lines[3:i_face]]
    assert all(l.startswith("property ") for l in lines[3:i_face]) and lines[i_face + 1:-1] == ["property list uchar int vertex_indices"]
    return nv, nf, props, body


def legacy_write_ply(path, vertices, triangles, normals=None):
    """The writer as it was before colours (kept here so that the identity is checked against its output, not against a remembered hash alone)."""
    v = np.ascontiguousarray(np.asarray(vertices)[:, :3], "<f4")
    t = np.ascontiguousarray(np.asarray(triangles)).view("<i4")
    props = ["x", "y", "z"]
    if normals is not None:
        v = np.ascontiguousarray(np.concatenate([v, np.ascontiguousarray(np.asarray(normals)[:, :3], "<f4")], 1))
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


@pytest.mark.parametrize("with_normals", [False, True], ids=["xyz", "xyz+normals"])
@pytest.mark.parametrize("channels", [3, 4])
def test_coloured_file_reads_back(tmp_path, with_normals, channels):
    m = R.mesh_of("hand")
    n = len(m.vertices)
    rng = np.random.default_rng(2)
    colors = rng.integers(0, 256, (n, channels), dtype=np.uint8)
    nrm = np.arange(n * 4, dtype=np.float32).reshape(-1, 4) if with_normals else None
    path = tmp_path / "c.ply"
    mesh_io.write_ply(str(path), m.vertices, m.triangles, nrm, colors=colors)
    nv, nf, props, body = read_ply(path.read_bytes())
    floats = ["x", "y", "z"] + (["nx", "ny", "nz"] if with_normals else [])
    assert (nv, nf) == (n, len(m.triangles))
    assert props == [("float", p) for p in floats] + [("uchar", "red"), ("uchar", "green"), ("uchar", "blue")]
    stride = 4 * len(floats) + 3
    assert len(body) == nv * stride + nf * 13
    rec = np.frombuffer(body[:nv * stride], np.uint8).reshape(nv, stride)
    want_f = m.vertices[:, :3] if not with_normals else np.concatenate([m.vertices[:, :3], nrm[:, :3]], 1)
    assert np.ascontiguousarray(rec[:, :4 * len(floats)]).tobytes() == np.ascontiguousarray(want_f, "<f4").tobytes()
    assert np.array_equal(rec[:, 4 * len(floats):], colors[:, :3])                            # r, g, b as given; a 4th column is dropped
    faces = np.frombuffer(body[nv * stride:], np.uint8).reshape(nf, 13)
    assert (faces[:, 0] == 3).all() and np.ascontiguousarray(faces[:, 1:]).tobytes() == m.triangles.astype("<u4").tobytes()


def test_without_colours_the_file_is_what_it_was(tmp_path):
    m = R.mesh_of("hand")
    nrm = np.arange(len(m.vertices) * 4, dtype=np.float32).reshape(-1, 4)
    digests = []
    for i, normals in enumerate((None, nrm)):
        a, b, c = tmp_path / ("a%d.ply" % i), tmp_path / ("b%d.ply" % i), tmp_path / ("c%d.ply" % i)
        mesh_io.write_ply(str(a), m.vertices, m.triangles, normals)
        mesh_io.write_ply(str(b), m.vertices, m.triangles, normals, colors=None)
        legacy_write_ply(str(c), m.vertices, m.triangles, normals)
        assert a.read_bytes() == b.read_bytes() == c.read_bytes()
        assert b"uchar red" not in a.read_bytes().split(b"end_header\n")[0]
        digests.append(hashlib.sha256(a.read_bytes()).hexdigest())
    # the sha256 of the two files as the writer produced them before it took colours
    assert digests == ["4cd13492ea82c379bdc57caea623a526752189e02fe71031ace42e31ef2ace75", "344724a7fe10b6e8a97df4628981f802a402647152a186f01abf1fb398a5df37"]


def test_bad_colours_are_refused(tmp_path):
    m = R.mesh_of("hand")
    n = len(m.vertices)
    for bad in (np.zeros((n, 3), np.float32), np.zeros((n - 1, 3), np.uint8), np.zeros((n, 2), np.uint8), np.zeros(n * 3, np.uint8)):
        with pytest.raises(ValueError):
            mesh_io.write_ply(str(tmp_path / "x.ply"), m.vertices, m.triangles, colors=bad)
