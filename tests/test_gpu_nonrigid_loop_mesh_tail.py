"""The mesh tail on the closed non-rigid loop's own data (tests/mesh_tail_loop.py): the colour loop (FAST: 64^3, 160 x 120, 7 frames,
extend inside) runs on the GPU backend and on the oracle backend, and on frames 3 and 6 the loop's volume, colour volume and warp-field
handle go through fetchMesh with normals, mesh_components, remove_small_components (25 triangles, and keep_largest) with the normals
as attribute, simplify_mesh (1.5 voxels, plain and keep_first), mesh_adjacency / mesh_topology, smooth_mesh (3 iterations, boundary fixed
and free), the one-call fetchMesh with all three options, warp + renderMesh of that mesh at the frame's pose and
renderLiveModelFiltered with the colour volume (and with keep_largest).  Every output of every step, the counts included, equals the
numpy restatement's on the oracle backend's state bit for bit; the one-call fetchMesh's normals are the oracle's at the SMOOTHED
vertices.

The conditions on the inputs are taken from the restatements alone and their figures are pinned (FIGURES): on both frames the mesh has
components either side of the threshold (sizes 2 6 6 6 34 4532 23834 and 2 2 4 8 8 38 5064 24290), vertices no triangle uses, boundary
and irregular edges, fins and duplicates at the chosen cell, vertices of every class, and more than 5 000 pixels hit."""
import pytest

import mesh_tail_loop as MT
import nonrigid_loop as NL

pytestmark = pytest.mark.gpu
CASE = NL.FAST
FIGURES = {
    3: dict(vertices=15184, triangles=28420, components=7, small=4, large=3, unused_vertices=320, filtered_triangles=28400, largest_triangles=23834,
            simplified_vertices=1938, simplified_triangles=3497, collapsed=24857, fin=38, duplicate=8, boundary_edges=401, irregular_edges=3,
            class1=1537, class2=395, class3=6, moved_fixed=1537, moved_free=1938, pixels_composed=9932, pixels_filtered=10331,
            normals_changed_by_smoothing=1448, pixels_changed_by_filter=8, pixels_changed_by_largest=2330),
    6: dict(vertices=15660, triangles=29416, components=8, small=5, large=3, unused_vertices=326, filtered_triangles=29392, largest_triangles=24290,
            simplified_vertices=1960, simplified_triangles=3550, collapsed=25816, fin=24, duplicate=2, boundary_edges=380, irregular_edges=2,
            class1=1582, class2=374, class3=4, moved_fixed=1582, moved_free=1960, pixels_composed=8630, pixels_filtered=10012,
            normals_changed_by_smoothing=1499, pixels_changed_by_filter=5, pixels_changed_by_largest=2317),
}


@pytest.fixture(scope="module")
def loops():
    """Each loop once: (the oracle's record and tails, the GPU's record and tails)."""
    want = MT.run(MT.TailOracleBackend(CASE), CASE, MT.oracle_tail)
    got = MT.run(MT.TailGpuBackend(CASE), CASE, MT.gpu_tail)
    return want, got


def test_the_inputs_deserve_the_test(loops):
    (rec, tails), _ = loops
    assert NL.nonvacuity(rec, CASE) == []
    assert sorted(tails) == list(MT.TAIL_FRAMES)
    for f in MT.TAIL_FRAMES:
        fig = MT.figures(tails[f])
        print("frame %d: %s" % (f, fig))
        assert MT.nonvacuity(fig) == [], "frame %d" % f
        assert fig == FIGURES[f], "frame %d: the figures moved" % f


def test_the_loops_are_in_the_same_state(loops):
    (want, _), (got, _) = loops
    msg = NL.first_difference(got, want)
    assert msg is None, "GPU against the restatement: " + msg


@pytest.mark.parametrize("frame", MT.TAIL_FRAMES)
def test_every_step_of_the_tail_equals_its_restatement(loops, frame):
    (_, want), (_, got) = loops
    assert sorted(got) == sorted(want) == list(MT.TAIL_FRAMES)
    msg = MT.first_difference(got[frame], want[frame])
    assert msg is None, "frame %d, GPU against the restatement: %s" % (frame, msg)
    g, w = got[frame], want[frame]
    # what the items above already say, spelled out: the gathered normals are the restatement's gather by vertex_src, and the one-call
    # mesh is the composition of the single steps as the GPU itself gave them
    assert (g["3.normals"] == w["1.normals"][w["3.vertex_src"]]).all() and (g["3L.normals"] == w["1.normals"][w["3L.vertex_src"]]).all()
    assert (g["7.vertices"] == g["6.fixed"]).all() and (g["7.triangles"] == g["4.triangles"]).all()
    assert (g["7.plain.vertices"] == g["7.vertices"]).all() and (g["7.plain.triangles"] == g["7.triangles"]).all()
    assert tuple(g["7.counts"]) == (FIGURES[frame]["vertices"], FIGURES[frame]["triangles"])
