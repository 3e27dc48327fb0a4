"""Manifold repair of an indexed triangle mesh - cut and stitch of non-manifold edges - in plain numpy / Python: the statement
tests/test_gpu_mesh_repair.py holds csrc/mesh_repair.hip to, bit for bit (include/nerfart_hip.h has the rules).  Written from the rules - dicts,
sorted lists, an explicit union-find -, not from the kernels:

  0. bad and degenerate faces (mesh_topology_ref.classify) are dropped;
  1. CANCEL: of the proper faces with one vertex set, p of one orientation and q of the other, the first |p - q| of the majority survive;
  2. PAIRING: the half-edges of every edge {a < b} with 2 < n <= 64 are ordered around d = v_b - v_a by the direction of their apex (fp64, every
     operation rounded once; position = the number of half-edges that compare before it, ties to the smaller id) and matched as brackets over the
     cycle - wedge "void": forward opens, backward closes; wedge "solid": backward opens, forward closes; an edge with n > 64 is WIDE: unpaired;
  3. CLASSES: across every edge with n == 2 and every pair the two faces' corners at a are united, and their corners at b; every class is one
     output vertex, numbered ascending by (original vertex, smallest corner id);
  4. MULTI-EDGES: the UNITS of an edge with 2 < n <= 64 - its pairs and its unpaired half-edges - are grouped by (class at a, class at b); the
     unit holding the group's smallest half-edge id keeps the edge, every other unit is subdivided;
  5. SUBDIVISION: one new vertex (v_a + v_b) * 0.5f (fp32) per subdivided unit, after the class vertices, ordered by the unit's smallest half-edge
     id; a face with k subdivided half-edges becomes the fan of its polygon from the midpoint of its lowest subdivided half-edge: k + 1 faces,
     the first in the face's place, the others after all surviving faces in (face, fan) order;
  6. the surviving faces in input order, then the appended ones.

`_bug` injects one known mistake (tests/test_mesh_repair_ref.py shows that a named assertion catches each): "pair_by_id" orders the half-edges
of an edge by id instead of by angle; "skip_multi_edge" subdivides nothing; "unite_unpaired" unites the corners of every unpaired half-edge with
those of the edge's smallest half-edge."""
import numpy as np

import mesh_topology_ref as topo

INFO = ("dropped_bad", "dropped_degenerate", "dropped_cancelled", "nonmanifold_edges", "edges_paired", "unpaired_half_edges", "wide_edges",
        "vertices_split", "pairs_subdivided", "sort_ties", "overflow")
WIDE = 64
WEDGES = ("void", "solid")


def cancel(faces, V):
    """(alive [F] bool, dropped (bad, degenerate, cancelled)): rule 0 and rule 1."""
    f = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    proper, degenerate, bad = topo.classify(f, V)
    groups = {}
    for i in np.nonzero(proper)[0].tolist():
        t = f[i].tolist()
        j = t.index(min(t))
        even = t[(j + 1) % 3] < t[(j + 2) % 3]                               # the rotation with the smallest first is the sorted triple
        groups.setdefault(tuple(sorted(t)), ([], []))[0 if even else 1].append(i)
    alive = np.zeros(len(f), dtype=bool)
    for p, q in groups.values():
        major = p if len(p) > len(q) else q
        alive[major[:abs(len(p) - len(q))]] = True                            # the lists are in input order
    return alive, (int(bad.sum()), int(degenerate.sum()), int(proper.sum() - alive.sum()))


def _sub(p, q):
    return (p[0] - q[0], p[1] - q[1], p[2] - q[2])


def _cross(p, q):
    return (p[1] * q[2] - p[2] * q[1], p[2] * q[0] - p[0] * q[2], p[0] * q[1] - p[1] * q[0])


def _dot(p, q):
    return (p[0] * q[0] + p[1] * q[1]) + p[2] * q[2]


def radial_order(v64, a, b, hes, apex):
    """(the half-edges `hes` (ascending ids) of edge {a < b} in angular order around v_b - v_a, starting with the smallest id; ties met).  Python
    floats are fp64 and every operation below is rounded once."""
    va = tuple(v64[a].tolist())
    d = _sub(tuple(v64[b].tolist()), va)
    w = [_sub(tuple(v64[apex[h]].tolist()), va) for h in hes]
    u1 = _cross(d, w[0])
    u2 = _cross(d, u1)
    xy = [(1.0, 0.0)] + [(-_dot(wi, u2), _dot(wi, u1)) for wi in w[1:]]
    second = [y < 0.0 or (y == 0.0 and x < 0.0) for x, y in xy]
    ties = 0

    def before(i, j):                                                          # hes is ascending: i < j is the order of the ids
        nonlocal ties
        if second[i] != second[j]:
            return second[j]
        c = xy[i][0] * xy[j][1] - xy[j][0] * xy[i][1]
        if c > 0.0:
            return True
        if c < 0.0:
            return False
        ties += i < j                                                          # once per unordered pair
        return i < j

    n = len(hes)
    rank = [sum(before(j, i) for j in range(n) if j != i) for i in range(n)]
    order = sorted(range(n), key=lambda i: (rank[i], i))
    return [hes[i] for i in order], ties


def bracket_pairs(seq, opens):
    """[(opener, closer)] of the cyclic sequence: openers are pushed, a closer pops; two turns."""
    n, stack, matched, pairs = len(seq), [], set(), []
    for t in range(2 * n):
        h = seq[t % n]
        if h in matched:
            continue
        if opens[h]:
            if t < n:
                stack.append(h)
        elif stack:
            o = stack.pop()
            matched.update((o, h))
            pairs.append((o, h))
    return pairs


def repair(verts, faces, wedge="void", _bug=None):
    """dict: verts [V', 3] float32, faces [F', 3] int32, src_vertex [V'] int32, mid_ends [M, 2] int32, info [16] uint32 (INFO names the first
    eleven), alive [F] bool (the faces that survive rules 0 and 1), splits [F] (the subdivided half-edges of every face)."""
    if wedge not in WEDGES:
        raise ValueError(f"wedge must be one of {WEDGES}")
    v32 = np.asarray(verts, dtype=np.float32).reshape(-1, 3)
    v64 = v32.astype(np.float64)
    f = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    V, F = len(v32), len(f)
    alive, dropped = cancel(f, V)
    fa = np.where(alive[:, None], f, -1)                                       # a dead face is a bad one: half-edge ids stay
    flat = fa.reshape(-1)
    e = topo.edges(fa, V)
    he, edge, n = e["he"], e["edge"], e["n_fwd"] + e["n_bwd"]
    fwd = dict(zip(he.tolist(), e["fwd"].tolist()))
    nxt = lambda h: h - 2 if h % 3 == 2 else h + 1
    corner = lambda h, v: h if flat[h] == v else nxt(h)
    apex = lambda h: int(flat[nxt(nxt(h))])
    order = np.argsort(edge, kind="stable")
    start = np.concatenate([[0], np.cumsum(n)])
    uf = topo.UnionFind(3 * F)

    def unite(h1, h2, a, b):
        uf.unite(corner(h1, a), corner(h2, a))
        uf.unite(corner(h1, b), corner(h2, b))

    met = paired = unpaired = wide = ties = 0
    units_of = {}                                                              # edge -> [unit: tuple of half-edges, smallest first]
    for k in range(len(n)):
        hes = he[order[start[k]:start[k + 1]]].tolist()
        a, b = (int(x) for x in e["key"][k])
        if n[k] == 2:
            unite(hes[0], hes[1], a, b)
        if n[k] <= 2:
            continue
        met += 1
        if n[k] > WIDE:
            wide += 1
            unpaired += int(n[k])
            continue
        if _bug == "pair_by_id":
            seq = hes
        else:
            seq, t = radial_order(v64, a, b, hes, {h: apex(h) for h in hes})
            ties += t
        opens = {h: fwd[h] == (wedge == "void") for h in hes}
        pairs = bracket_pairs(seq, opens)
        single = sorted(set(hes) - {h for p in pairs for h in p})
        paired += bool(pairs)
        unpaired += len(single)
        for o, c in pairs:
            unite(o, c, a, b)
        if _bug == "unite_unpaired":
            for h in single:
                unite(hes[0], h, a, b)
        units_of[k] = sorted([tuple(sorted(p)) for p in pairs] + [(h,) for h in single])

    roots = sorted({(int(flat[h]), uf.find(h)) for h in he.tolist()})          # ascending (original vertex, smallest corner id)
    cls = {r: i for i, (_, r) in enumerate(roots)}
    V1 = len(roots)
    new = lambda h: cls[uf.find(h)]                                            # the output vertex of corner h
    src = [v for v, _ in roots]

    sub_units = []
    if _bug != "skip_multi_edge":
        for k, units in units_of.items():
            a, b = (int(x) for x in e["key"][k])
            seen = set()
            for u in units:                                                    # ascending smallest id: the first of a group keeps the edge
                key = (new(corner(u[0], a)), new(corner(u[0], b)))
                if key in seen:
                    sub_units.append((u, key))
                seen.add(key)
    sub_units.sort()
    mid = {}
    for i, (u, _) in enumerate(sub_units):
        for h in u:
            mid[h] = V1 + i
    mid_ends = np.array([key for _, key in sub_units], dtype=np.int32).reshape(-1, 2)
    out_v = np.zeros((V1 + len(sub_units), 3), dtype=np.float32)
    if V1:
        out_v[:V1] = v32[src]
    for i, (ca, cb) in enumerate(mid_ends.tolist()):
        out_v[V1 + i] = (v32[src[ca]] + v32[src[cb]]) * np.float32(0.5)        # fp32: add, then multiply

    first, extra, splits = [], [], np.zeros(F, dtype=np.int64)
    for face in np.nonzero(alive)[0].tolist():
        poly, at = [], None
        for i in range(3):
            h = 3 * face + i
            poly.append(new(h))
            if h in mid:
                if at is None:
                    at = len(poly)
                poly.append(mid[h])
        splits[face] = len(poly) - 3
        if at is None:
            first.append(poly)
            continue
        poly = poly[at:] + poly[:at]                                           # starts at the midpoint of the lowest subdivided half-edge
        fan = [[poly[0], poly[j], poly[j + 1]] for j in range(1, len(poly) - 1)]
        first.append(fan[0])
        extra += fan[1:]
    out_f = np.array(first + extra, dtype=np.int32).reshape(-1, 3)
    info = np.zeros(16, dtype=np.uint32)
    referenced = len({v for v, _ in roots})
    info[:11] = list(dropped) + [met, paired, unpaired, wide, V1 - referenced, len(sub_units), ties, 0]
    return {"verts": out_v, "faces": out_f, "src_vertex": np.array(src + [-1] * len(sub_units), dtype=np.int32), "mid_ends": mid_ends, "info": info,
            "alive": alive, "splits": splits}


def info_dict(info):
    return {k: int(x) for k, x in zip(INFO, info)}


# ---- the meshes the tests share -----------------------------------------------------------------------------------------------------------------

def outward_tetrahedron(verts, q):
    """The four faces of the tetrahedron over the vertices q [4], outward for their positions; None when it is flat."""
    q = np.asarray(q)
    p = np.asarray(verts)[q].astype(np.float64)
    vol = np.dot(np.cross(p[1] - p[0], p[2] - p[0]), p[3] - p[0])
    if vol == 0.0:
        return None
    a, b, c, d = (int(x) for x in (q if vol > 0 else q[[0, 2, 1, 3]]))         # now (b - a) x (c - a) . (d - a) > 0
    return [[a, c, b], [a, b, d], [a, d, c], [b, c, d]]


def tetrahedron_soup(K, n_verts, seed, lattice=None):
    """(verts [n_verts, 3] float32, faces [4 K, 3] int32): K tetrahedra over random 4-subsets of the vertices, each oriented outward for its own
    positions: every edge is balanced.  lattice = L puts the vertices on distinct points of {0 .. L - 1}^3 (exact coplanarity, exact fp64)."""
    rng = np.random.default_rng(seed)
    if lattice is None:
        verts = rng.uniform(-1.0, 1.0, size=(n_verts, 3)).astype(np.float32)
    else:
        verts = np.stack(np.unravel_index(rng.choice(lattice ** 3, size=n_verts, replace=False), (lattice,) * 3), axis=1).astype(np.float32)
    faces = []
    while len(faces) < 4 * K:
        tet = outward_tetrahedron(verts, rng.choice(n_verts, size=4, replace=False))
        faces += tet or []                                                     # a flat tetrahedron has no outside
    return verts, np.array(faces, dtype=np.int32)
