"""The marching-cubes case table (nerfart_amd/mc_table.py -> csrc/mc_table.h): the committed header is what the generator builds, every case uses
exactly its sign-changing edges, the segments a case leaves on a cell face are a function of that face's corner signs alone (and the
neighbouring cell sees them reversed: no cracks, whatever made the table), and every case closes up on its own."""
import os
import re

import numpy as np
import pytest

from conftest import REPO
from nerfart_amd import mc_table
import mc_ref

TABLE = mc_table.build_table()


def _initialiser(src, name):
    body = re.search(name + r"\b[^=]*=\s*\{(.*?)\};", src, flags=re.S).group(1)
    return body


def test_committed_header_is_what_the_generator_builds():
    src = open(os.path.join(REPO, "nerfart_amd", "csrc", "mc_table.h")).read()
    assert src == mc_table.header_text(), "run python -m nerfart_amd.mc_table"
    src = re.sub(r"//[^\n]*", "", src)
    width = int(re.search(r"#define MC_MAX_TRIS (\d+)", src).group(1))
    assert width == max(len(t) for t in TABLE)
    rows = re.findall(r"\{([^{}]*)\}", _initialiser(src, "mc_tri_edges"))
    counts = [int(x, 0) for x in re.findall(r"[-\w]+", _initialiser(src, "mc_tri_count"))]
    masks = [int(x, 0) for x in re.findall(r"[-\w]+", _initialiser(src, "mc_edge_mask"))]
    assert len(rows) == len(counts) == len(masks) == 256
    for case in range(256):
        flat = [int(x) for x in rows[case].split(",")]
        assert len(flat) == 3 * width
        n = counts[case]
        assert n == len(TABLE[case])
        assert [tuple(flat[3 * k:3 * k + 3]) for k in range(n)] == TABLE[case], case
        assert all(e == -1 for e in flat[3 * n:])
        assert masks[case] == mc_table.edge_mask(TABLE[case])


def _sign_changing_edges(case):
    return {e for e in range(12) if len({(case >> c) & 1 for c in mc_table.edge_corners(e)}) == 2}


def test_every_case_uses_exactly_its_sign_changing_edges():
    for case in range(256):
        used = {e for t in TABLE[case] for e in t}
        assert used == _sign_changing_edges(case), case
        assert all(len(set(t)) == 3 for t in TABLE[case]), case


def _face_of_pair(e0, e1):
    """The cell face (axis, side) two different cube edges both lie on, or None."""
    def faces(e):
        p0, p1 = (mc_table.corner_xyz(c) for c in mc_table.edge_corners(e))
        return {(a, p0[a]) for a in range(3) if p0[a] == p1[a]}
    common = faces(e0) & faces(e1)
    assert len(common) <= 1
    return next(iter(common)) if common else None


def _edge_in_face_frame(e, axis):
    """A cube edge on a face of `axis`, as the pair of its end corners' (u, v) coordinates, u = axis + 1, v = axis + 2 (mod 3): the same for the
    two cells that share the face."""
    u, v = (axis + 1) % 3, (axis + 2) % 3
    return frozenset((mc_table.corner_xyz(c)[u], mc_table.corner_xyz(c)[v]) for c in mc_table.edge_corners(e))


def _boundary_segments(case):
    """{face: set of directed (edge, edge)}: the directed triangle edges of the case that are not cancelled by their reverse."""
    d = [(t[i], t[(i + 1) % 3]) for t in TABLE[case] for i in range(3)]
    assert len(set(d)) == len(d), case
    out = {}
    for a, b in d:
        if (b, a) in d:
            continue                                             # a diagonal inside the cell
        face = _face_of_pair(a, b)
        assert face is not None, (case, a, b)                    # the surface ends on the cell's faces only
        out.setdefault(face, set()).add((a, b))
    return out


def test_face_segments_depend_on_the_face_signs_only_and_reverse_for_the_neighbour():
    seen = {}                                                    # (axis, side, signs at (u, v) = (0,0) (1,0) (1,1) (0,1)) -> segments in the shared frame
    for case in range(256):
        segs = _boundary_segments(case)
        for axis in range(3):
            u, v = (axis + 1) % 3, (axis + 2) % 3
            for side in range(2):
                key = []
                for cu, cv in ((0, 0), (1, 0), (1, 1), (0, 1)):
                    p = [0, 0, 0]
                    p[axis], p[u], p[v] = side, cu, cv
                    key.append((case >> (p[0] + 2 * p[1] + 4 * p[2])) & 1)
                here = frozenset((_edge_in_face_frame(a, axis), _edge_in_face_frame(b, axis)) for a, b in segs.get((axis, side), ()))
                assert seen.setdefault((axis, side, tuple(key)), here) == here, (case, axis, side)
    assert len(seen) == 3 * 2 * 16
    for (axis, side, key), here in seen.items():
        there = seen[(axis, 1 - side, key)]                      # the neighbour across this face, same corner signs
        assert there == frozenset((b, a) for a, b in here), (axis, side, key)
        n_inside = sum(key)
        assert len(here) == (0 if n_inside in (0, 4) else 2 if key in ((1, 0, 1, 0), (0, 1, 0, 1)) else 1)


@pytest.mark.parametrize("padding", ["outside", "inside"])
def test_every_case_alone_gives_a_closed_oriented_surface(padding):
    """Case c (and with it 255 - c) as the middle cell of 3^3 cells, the rest of the volume all outside resp. all inside."""
    for case in range(256):
        vol = np.full((4, 4, 4), 1.0 if padding == "outside" else -1.0, dtype=np.float32)
        for c in range(8):
            dx, dy, dz = mc_table.corner_xyz(c)
            vol[1 + dx, 1 + dy, 1 + dz] = -1.0 if (case >> c) & 1 else 1.0
        assert mc_ref.cell_cases(vol)[1, 1, 1] == case
        verts, faces = mc_ref.marching_cubes(vol)
        assert mc_ref.is_closed(faces) and mc_ref.is_consistently_oriented(faces), (case, padding)
        if case not in (0, 255):
            assert len(faces) > 0
            vol_sign = mc_ref.signed_volume(verts, faces)
            n_in = int((vol < 0).sum())
            assert (vol_sign > 0) if n_in <= 32 else (vol_sign < 0), (case, padding)      # normals point away from the inside
