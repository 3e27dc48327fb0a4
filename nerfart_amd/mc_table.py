"""The marching-cubes case table of csrc/marching_cubes.hip, generated from a rule instead of typed in.

    python -m nerfart_amd.mc_table          # rewrites nerfart_amd/csrc/mc_table.h (committed; tests/test_mc_table.py holds it to build_table())

Numbering (the unit cell [0,1]^3, x slowest / z fastest like the volume):
  * corner c = dx + 2 dy + 4 dz sits at (dx, dy, dz); bit c of the case index is set iff that corner is INSIDE, value < level (strict).
  * edge e = 4 a + k runs along axis a = e >> 2 (0 x, 1 y, 2 z) from the corner whose other two coordinates, taken in ascending axis order, are
    (k & 1, k >> 1):   0..3  along x at (dy, dz) = (0,0) (1,0) (0,1) (1,1)
                       4..7  along y at (dx, dz) = (0,0) (1,0) (0,1) (1,1)
                       8..11 along z at (dx, dy) = (0,0) (1,0) (0,1) (1,1)
    so the grid point that OWNS the edge (its lower end) is the cell origin plus those two offsets, and the edge is that point's axis-a edge.

The rule.  On each of the six faces, walk the four corners counter-clockwise as seen from outside the cell.  Every maximal run of inside corners
(fewer than four) gives one segment: from the face edge entering the run to the face edge leaving it.  On the ambiguous face - two inside corners
on a diagonal - the runs have length one, i.e. each inside corner is cut off separately.  The segments of a face are thereby a function of that
face's four corner signs alone, and the neighbouring cell, which walks the same face the other way round, gets the same segments reversed: no
cracks.  Every sign-changing edge ends one segment and starts one (on its two faces), so the segments chain into closed loops, taken in order of
their lowest edge id.  Each loop is fan-triangulated from its lowest edge id - with one exception: a fan diagonal that joins two edges of the
same cube face lies IN that (ambiguous) face, and the neighbouring cell can produce the very same diagonal, which puts one mesh edge into four
triangles (a random volume does it within a few thousand cells).  So the apex is the lowest edge id of the loop whose fan has no such diagonal;
one exists for every loop of every case (build_table asserts it), and it is the lowest edge for all but 18 loops.  Diagonals then lie strictly
inside the cell, the only mesh edges on a cell face are the face's segments, and every mesh edge is in exactly two triangles.  With the segments
directed as above, the normal (v1 - v0) x (v2 - v0) of every triangle points to the outside (value >= level): outward for a signed distance.
"""
from __future__ import annotations

import os

HEADER = os.path.join(os.path.dirname(os.path.abspath(__file__)), "csrc", "mc_table.h")


def corner_xyz(c: int):
    return (c & 1, (c >> 1) & 1, (c >> 2) & 1)


def edge_corners(e: int):
    """(c0, c1): the two corners of edge e, c0 the lower one along the edge's axis (the owner's corner)."""
    a, k = e >> 2, e & 3
    o1, o2 = [ax for ax in range(3) if ax != a]
    p = [0, 0, 0]
    p[o1], p[o2] = k & 1, k >> 1
    c0 = p[0] + 2 * p[1] + 4 * p[2]
    return c0, c0 + (1 << a)


EDGE_OF = {frozenset(edge_corners(e)): e for e in range(12)}


def face_corners(axis: int, side: int):
    """The four corners of the face `coordinate axis == side`, counter-clockwise seen from outside the cell."""
    u, v = (axis + 1) % 3, (axis + 2) % 3                      # (u, v, axis) is right-handed: ccw seen from +axis
    ring = [(0, 0), (1, 0), (1, 1), (0, 1)]
    if side == 0:
        ring = ring[::-1]
    out = []
    for cu, cv in ring:
        p = [0, 0, 0]
        p[axis], p[u], p[v] = side, cu, cv
        out.append(p[0] + 2 * p[1] + 4 * p[2])
    return out


FACES = [(a, s) for a in range(3) for s in range(2)]


def edge_faces(e: int):
    """The two faces (axis, side) edge e lies on."""
    p0, p1 = (corner_xyz(c) for c in edge_corners(e))
    return {(a, p0[a]) for a in range(3) if p0[a] == p1[a]}


def face_segments(case: int, axis: int, side: int):
    """Directed segments (edge_from, edge_to) the case leaves on one face."""
    q = face_corners(axis, side)
    ins = [(case >> c) & 1 for c in q]
    if sum(ins) in (0, 4):
        return []
    f = [EDGE_OF[frozenset((q[i], q[(i + 1) % 4]))] for i in range(4)]      # f[i] joins q[i] and q[i + 1]
    segs = []
    for i in range(4):
        if ins[i] and not ins[i - 1]:                            # a run of inside corners starts at q[i]
            j = i
            while ins[(j + 1) % 4]:
                j += 1
            segs.append((f[(i - 1) % 4], f[j % 4]))
    return segs


def case_loops(case: int):
    nxt = {}
    for a, s in FACES:
        for e0, e1 in face_segments(case, a, s):
            assert e0 not in nxt
            nxt[e0] = e1
    assert sorted(nxt) == sorted(nxt.values())
    loops, seen = [], set()
    for e in sorted(nxt):
        if e in seen:
            continue
        loop = [e]
        seen.add(e)
        while nxt[loop[-1]] != e:
            loop.append(nxt[loop[-1]])
            seen.add(loop[-1])
        loops.append(loop)                                       # starts at its lowest edge: `e` ascends and is the first of its loop seen
    return loops


def fan(loop):
    """The loop rotated to its fan apex: the lowest edge id from which no fan diagonal joins two edges of one cube face."""
    n = len(loop)
    for apex in sorted(loop):
        r = loop.index(apex)
        rot = loop[r:] + loop[:r]
        if all(not (edge_faces(rot[0]) & edge_faces(rot[i])) for i in range(2, n - 1)):
            return rot
    raise AssertionError(f"no fan without an in-face diagonal for loop {loop}")


def build_table():
    """table[case] = [(e0, e1, e2), ...]: the triangles of each of the 256 cases as cube-edge ids."""
    table = []
    for case in range(256):
        tris = []
        for loop in case_loops(case):
            assert len(loop) >= 3
            rot = fan(loop)
            tris += [(rot[0], rot[i], rot[i + 1]) for i in range(1, len(rot) - 1)]
        table.append(tris)
    assert table[1] == [(0, 4, 8)]                               # corner 0 inside: x edge -> y edge -> z edge, normal along (1, 1, 1)
    return table


def edge_mask(tris) -> int:
    m = 0
    for t in tris:
        for e in t:
            m |= 1 << e
    return m


def header_text() -> str:
    table = build_table()
    width = max(len(t) for t in table)
    lines = ["// mc_table.h - GENERATED by `python -m nerfart_amd.mc_table` (nerfart_amd/mc_table.py documents the corner / edge numbering and the rule);",
             "// do not edit: tests/test_mc_table.py holds this file to build_table() entry for entry.",
             "#pragma once",
             "#ifndef MC_TABLE_DECL",
             "#define MC_TABLE_DECL static const",
             "#endif",
             f"#define MC_MAX_TRIS {width}",
             "// triangles of each case as cube-edge ids, three per triangle, padded with -1",
             "MC_TABLE_DECL signed char mc_tri_edges[256][MC_MAX_TRIS * 3] = {"]
    for tris in table:
        flat = [e for t in tris for e in t] + [-1] * (3 * (width - len(tris)))
        lines.append("    {" + ", ".join(f"{e:2d}" for e in flat) + "},")
    lines += ["};", "// triangles per case", "MC_TABLE_DECL unsigned char mc_tri_count[256] = {"]
    for r in range(0, 256, 32):
        lines.append("    " + ", ".join(str(len(t)) for t in table[r:r + 32]) + ",")
    lines += ["};", "// bit e set iff cube edge e carries a vertex in this case", "MC_TABLE_DECL unsigned short mc_edge_mask[256] = {"]
    for r in range(0, 256, 16):
        lines.append("    " + ", ".join(f"0x{edge_mask(t):03x}" for t in table[r:r + 16]) + ",")
    lines += ["};", ""]
    return "\n".join(lines)


if __name__ == "__main__":
    with open(HEADER, "w") as f:
        f.write(header_text())
    print(HEADER)
