"""numpy restatement of the mesh rasteriser's rule (include/dfusion.h dfusion_render_mesh): vertices snapped to
1/16 pixel, integer edge functions, inclusive coverage, a minimum over 64-bit {z bits, triangle} keys, the resolve.  f32 arithmetic in
the stated order (mesh_ref.fma32 / aff_mul restate the fused forms exactly), int64 for the integers.  Vectorised over triangles with a
loop over the box offsets; nothing is taken from the HIP source.  Also the test meshes: a latitude / longitude sphere."""
import numpy as np

from mesh_ref import aff_mul, fma32

F32 = np.float32
MISS_KEY = np.uint64(0xffffffffffffffff)
QNAN_BITS = np.uint32(0x7fffffff)


def project_vertices(vertices, world2cam, intr):
    """-> (valid bool [V], X int64 [V], Y int64 [V], iz f32 [V], pc f32 [V, 3])."""
    v = np.ascontiguousarray(np.asarray(vertices, F32)[:, :3])
    pc = aff_mul(world2cam, v) if world2cam is not None else v.copy()
    n = len(pc)
    fx, fy, cx, cy = (np.full(n, F32(p), F32) for p in intr)
    with np.errstate(all="ignore"):
        u = fma32(fx, pc[:, 0] / pc[:, 2], cx)
        w = fma32(fy, pc[:, 1] / pc[:, 2], cy)
        valid = np.isfinite(pc).all(1) & (pc[:, 2] > 0) & (np.abs(u) < F32(65536)) & (np.abs(w) < F32(65536))
        X = np.rint(F32(16) * np.where(valid, u, F32(0))).astype(np.int64)          # half-even; the product is exact
        Y = np.rint(F32(16) * np.where(valid, w, F32(0))).astype(np.int64)
        iz = (F32(1) / pc[:, 2]).astype(F32)
    return valid, X, Y, iz, pc


def _edges(X, Y, px, py):
    """X, Y [n, 3] (oriented), sample (px, py) in 1/16 pixel -> w0, w1, w2 int64."""
    w0 = (X[:, 2] - X[:, 1]) * (py - Y[:, 1]) - (Y[:, 2] - Y[:, 1]) * (px - X[:, 1])
    w1 = (X[:, 0] - X[:, 2]) * (py - Y[:, 2]) - (Y[:, 0] - Y[:, 2]) * (px - X[:, 2])
    w2 = (X[:, 1] - X[:, 0]) * (py - Y[:, 0]) - (Y[:, 1] - Y[:, 0]) * (px - X[:, 0])
    return w0, w1, w2


def _mix(c, a):
    """(c0 a0 + c1 a1) + c2 a2 ; c [n, 3] f32, a [n, 3] f32."""
    return ((c[:, 0] * a[:, 0] + c[:, 1] * a[:, 1]) + c[:, 2] * a[:, 2]).astype(F32)


def render(vertices, triangles, cols, rows, intr, world2cam=None, normals=None, attr=None, colors=None, max_extent=16):
    """-> dict: points / normals / attr uint32 bits [rows, cols, 4] (normals, attr: None without the input), colors uint8 [rows, cols, 4]
    or None, tri int32 [rows, cols], counts uint64 [6], status uint8 [T], keys uint64 [rows, cols]."""
    vertices = np.asarray(vertices, F32).reshape(-1, 4)
    tri = np.asarray(triangles).astype(np.int64).reshape(-1, 3)
    V, T = len(vertices), len(tri)
    npix = cols * rows
    keys = np.full(npix, MISS_KEY, np.uint64)
    counts = np.zeros(6, np.uint64)
    status = np.zeros(T, np.uint8)
    fx, fy, cx, cy = (F32(p) for p in intr)
    ext16 = 16 * int(max_extent)
    if V and T:
        valid, Xv, Yv, izv, _ = project_vertices(vertices, world2cam, intr)
        inb = (tri < V).all(1)
        ti = np.where(inb[:, None], tri, 0)
        bad = ~inb | ~valid[ti].all(1)
        X, Y, IZ = Xv[ti], Yv[ti], izv[ti]
        area2 = (X[:, 1] - X[:, 0]) * (Y[:, 2] - Y[:, 0]) - (X[:, 2] - X[:, 0]) * (Y[:, 1] - Y[:, 0])
        minX, maxX, minY, maxY = X.min(1), X.max(1), Y.min(1), Y.max(1)
        x0 = np.maximum(-((-minX) // 16), 0); x1 = np.minimum(maxX // 16, cols - 1)
        y0 = np.maximum(-((-minY) // 16), 0); y1 = np.minimum(maxY // 16, rows - 1)
        status[:] = np.select([bad, area2 == 0, (maxX - minX > ext16) | (maxY - minY > ext16), (x0 > x1) | (y0 > y1)], [1, 2, 3, 4], 0)
        counts[:5] = np.bincount(status, minlength=5)
        flip = area2 < 0
        order = np.where(flip[:, None], np.array([0, 2, 1]), np.array([0, 1, 2]))
        ti = np.take_along_axis(ti, order, 1); X = np.take_along_axis(X, order, 1); Y = np.take_along_axis(Y, order, 1)
        IZ = np.take_along_axis(IZ, order, 1)
        area2 = np.abs(area2)
        d = np.flatnonzero(status == 0)
        if len(d):
            Xd, Yd, IZd, fa = X[d], Y[d], IZ[d], area2[d].astype(F32)
            for dy in range(int((y1[d] - y0[d]).max()) + 1):
                for dx in range(int((x1[d] - x0[d]).max()) + 1):
                    x, y = x0[d] + dx, y0[d] + dy
                    w0, w1, w2 = _edges(Xd, Yd, 16 * x, 16 * y)
                    cov = (x <= x1[d]) & (y <= y1[d]) & (w0 >= 0) & (w1 >= 0) & (w2 >= 0)
                    with np.errstate(all="ignore"):
                        b0, b1, b2 = w0.astype(F32) / fa, w1.astype(F32) / fa, w2.astype(F32) / fa
                        iz = ((b0 * IZd[:, 0] + b1 * IZd[:, 1]) + b2 * IZd[:, 2]).astype(F32)
                        z = (F32(1) / iz).astype(F32)
                        cov &= (z > 0) & np.isfinite(z)
                    key = (z[cov].view(np.uint32).astype(np.uint64) << np.uint64(32)) | d[cov].astype(np.uint64)
                    np.minimum.at(keys, (y[cov] * cols + x[cov]), key)
    hit = np.flatnonzero(keys != MISS_KEY)
    counts[5] = len(hit)
    out = {"counts": counts, "status": status, "keys": keys.reshape(rows, cols)}
    points = np.full((npix, 4), QNAN_BITS, np.uint32)
    tri_out = np.full(npix, -1, np.int32)
    nrm_out = np.full((npix, 4), QNAN_BITS, np.uint32) if normals is not None else None
    att_out = np.full((npix, 4), QNAN_BITS, np.uint32) if attr is not None else None
    col_out = np.zeros((npix, 4), np.uint8) if colors is not None else None
    if len(hit):
        t = (keys[hit] & np.uint64(0xffffffff)).astype(np.int64)
        z = (keys[hit] >> np.uint64(32)).astype(np.uint32).view(F32)
        x, y = hit % cols, hit // cols
        w = np.stack(_edges(X[t], Y[t], 16 * x, 16 * y), 1)
        assert (w >= 0).all() and (w.sum(1) == area2[t]).all()
        b = (w.astype(F32) / area2[t].astype(F32)[:, None]).astype(F32)
        c = ((b * IZ[t]).astype(F32) * z[:, None]).astype(F32)
        p = np.zeros((len(hit), 4), F32)
        p[:, 0] = (x.astype(F32) - cx) / fx * z
        p[:, 1] = (y.astype(F32) - cy) / fy * z
        p[:, 2] = z
        points[hit] = p.view(np.uint32)
        tri_out[hit] = t.astype(np.uint32).view(np.int32)
        vi = ti[t]
        if attr is not None:
            a = np.asarray(attr, F32).reshape(-1, 4)
            o = np.zeros((len(hit), 4), F32)
            with np.errstate(all="ignore"):
                for ch in range(3):
                    o[:, ch] = _mix(c, a[vi, ch])
            att_out[hit] = o.view(np.uint32)
        if normals is not None:
            a = np.asarray(normals, F32).reshape(-1, 4)
            with np.errstate(all="ignore"):
                m = np.stack([_mix(c, a[vi, ch]) for ch in range(3)], 1)
                l2 = fma32(m[:, 0], m[:, 0], fma32(m[:, 1], m[:, 1], m[:, 2] * m[:, 2]))
                good = l2 > 0
                o = np.zeros((len(hit), 4), F32)
                o[:, :3] = m / np.sqrt(l2)[:, None]
            o = o.view(np.uint32)
            o[~good] = QNAN_BITS
            nrm_out[hit] = o
        if colors is not None:
            k = np.asarray(colors, np.uint8).reshape(-1, 4)
            o = np.full((len(hit), 4), 255, np.uint8)
            for ch in range(3):
                q = np.floor(_mix(c, k[vi, ch].astype(F32)) + F32(0.5))
                o[:, ch] = np.minimum(255, q.astype(np.int64)).astype(np.uint8)
            col_out[hit] = o
    out["points"] = points.reshape(rows, cols, 4)
    out["tri"] = tri_out.reshape(rows, cols)
    out["normals"] = None if nrm_out is None else nrm_out.reshape(rows, cols, 4)
    out["attr"] = None if att_out is None else att_out.reshape(rows, cols, 4)
    out["colors"] = None if col_out is None else col_out.reshape(rows, cols, 4)
    return out


# ------------------------------------------------------------------------------------------------ test meshes
def sphere_mesh(radius, centre, bands=48, segments=96, tilt=(0.5, 0.2)):
    """A latitude / longitude sphere: `bands` latitude bands of `segments` quads (the two pole bands: triangles), 2 segments (bands - 1)
    triangles, outward normals; the pole axis is turned by tilt[0] rad about x, then tilt[1] rad about z, off the optical axis.
    -> vertices f32 [V, 4] (w = 0), triangles uint32 [T, 3], normals f32 [V, 4]."""
    th = np.pi * np.arange(1, bands) / bands
    ph = 2 * np.pi * np.arange(segments) / segments
    ring = np.stack([np.sin(th)[:, None] * np.cos(ph)[None], np.sin(th)[:, None] * np.sin(ph)[None], np.repeat(np.cos(th)[:, None], segments, 1)], -1)
    n = np.concatenate([[[0.0, 0.0, 1.0]], ring.reshape(-1, 3), [[0.0, 0.0, -1.0]]])
    ca, sa, cb, sb = np.cos(tilt[0]), np.sin(tilt[0]), np.cos(tilt[1]), np.sin(tilt[1])
    R = np.array([[cb, -sb, 0], [sb, cb, 0], [0, 0, 1]]) @ np.array([[1, 0, 0], [0, ca, -sa], [0, sa, ca]])
    n = n @ R.T
    tris = []
    rid = lambda r, s: 1 + r * segments + (s % segments)
    south = 1 + (bands - 1) * segments
    for s in range(segments):
        tris.append((0, rid(0, s), rid(0, s + 1)))
        for r in range(bands - 2):
            tris.append((rid(r, s), rid(r + 1, s), rid(r + 1, s + 1)))
            tris.append((rid(r, s), rid(r + 1, s + 1), rid(r, s + 1)))
        tris.append((south, rid(bands - 2, s + 1), rid(bands - 2, s)))
    v4 = np.zeros((len(n), 4), F32); v4[:, :3] = (np.asarray(centre, np.float64) + radius * n).astype(F32)
    n4 = np.zeros((len(n), 4), F32); n4[:, :3] = n.astype(F32)
    return v4, np.array(tris, np.uint32), n4
