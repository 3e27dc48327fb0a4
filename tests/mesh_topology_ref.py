"""Half-edge adjacency, manifold checks and per-component measures of an indexed triangle mesh in plain numpy / Python - the statement
tests/test_gpu_mesh_topology.py holds csrc/mesh_topology.hip to, integer for integer (include/nerfart_hip.h has the definitions).  Written from
the definitions - sort / unique for the edges, an explicit union-find for fans and boundary loops - not from the kernels:

  * a face is bad if an index lies outside [0, V), degenerate if it is good but two indices are equal, otherwise proper; only proper faces count;
  * half-edge h = 3 f + i runs from faces[f][i] to faces[f][(i + 1) % 3] and is the corner of face f at faces[f][i];
  * for the undirected edge {a < b}, n_fwd / n_bwd count the proper half-edges a -> b / b -> a, n = n_fwd + n_bwd: boundary n == 1, manifold
    n_fwd == n_bwd == 1, flipped n == 2 otherwise, non-manifold n > 2;
  * fans: across every edge with n == 2 the two faces' corners at a are united, and their corners at b; vertex_fans[v] = corner classes at v;
  * boundary loops: boundary edges sharing a vertex are joined; a loop's size is its number of edges;
  * components are mesh_components_ref.components' labels; an edge / a face belongs to the component of its first vertex.

`_bug` injects one known mistake (tests/test_mesh_topology_ref.py shows that a named assertion catches each): "reversed_key" keys an edge by
(origin, destination) instead of (min, max); "per_half_edge" tallies the edge counts once per half-edge instead of once per edge;
"fans_across_nonmanifold" unites corners across every edge, whatever its n."""
import math

import numpy as np

import mesh_components_ref

INFO = ("proper_faces", "degenerate_faces", "bad_faces", "referenced_vertices", "edges", "boundary_edges", "flipped_edges", "nonmanifold_edges",
        "bowtie_vertices", "boundary_loops", "longest_loop", "overflow")
COUNTS = ("vertices", "edges", "faces", "boundary_edges", "flipped_edges", "nonmanifold_edges")


def classify(faces, V):
    """(proper, degenerate, bad) [F] bool"""
    f = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    bad = ((f < 0) | (f >= V)).any(axis=1)
    degenerate = ~bad & ((f[:, 0] == f[:, 1]) | (f[:, 1] == f[:, 2]) | (f[:, 0] == f[:, 2]))
    return ~bad & ~degenerate, degenerate, bad


class UnionFind:
    def __init__(self, n):
        self.parent = list(range(n))

    def find(self, v):
        root = v
        while self.parent[root] != root:
            root = self.parent[root]
        while self.parent[v] != root:
            self.parent[v], v = root, self.parent[v]
        return root

    def unite(self, a, b):
        a, b = self.find(a), self.find(b)
        if a != b:
            self.parent[max(a, b)] = min(a, b)


def edges(faces, V, _bug=None):
    """dict over the proper half-edges: he [H] their ids, a / b [H] the edge's vertices (a < b), fwd [H] bool (runs a -> b), edge [H] the index
    of the half-edge's edge among the E distinct ones (ascending (a, b)), and per edge n_fwd, n_bwd, key [E, 2]."""
    f = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    proper = classify(f, V)[0]
    he = np.nonzero(np.repeat(proper, 3))[0]
    src, dst = f.reshape(-1)[he], f[:, [1, 2, 0]].reshape(-1)[he]
    if _bug == "reversed_key":
        a, b, fwd = src, dst, np.ones(len(he), dtype=bool)
    else:
        a, b, fwd = np.minimum(src, dst), np.maximum(src, dst), src < dst
    if len(he):
        key, edge = np.unique(np.stack([a, b], axis=1), axis=0, return_inverse=True)
        edge = edge.reshape(-1)
    else:
        key, edge = np.zeros((0, 2), dtype=np.int64), np.zeros(0, dtype=np.int64)
    E = len(key)
    return {"he": he, "a": a, "b": b, "fwd": fwd, "edge": edge, "key": key,
            "n_fwd": np.bincount(edge[fwd], minlength=E), "n_bwd": np.bincount(edge[~fwd], minlength=E)}


def topology(faces, V, _bug=None):
    """dict: twin [3 F] int32, edge_uses [3 F] uint32, vertex_fans [V] uint32, info [16] uint32 (the header's indices, INFO names the first
    twelve), loop_sizes (sorted, descending: one per boundary loop)."""
    f = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    F = len(f)
    proper, degenerate, bad = classify(f, V)
    flat = f.reshape(-1)
    e = edges(f, V, _bug)
    he, edge, n_fwd, n_bwd = e["he"], e["edge"], e["n_fwd"], e["n_bwd"]
    n = n_fwd + n_bwd
    boundary, manifold = n == 1, (n_fwd == 1) & (n_bwd == 1)
    flipped, nonmanifold = (n == 2) & ~manifold, n > 2
    twin = np.full(3 * F, -4, dtype=np.int32)
    uses = np.zeros(3 * F, dtype=np.uint32)
    uses[he] = n[edge]
    twin[he] = np.select([boundary[edge], flipped[edge], nonmanifold[edge]], [-1, -2, -3], default=0)
    order = np.argsort(edge, kind="stable")                          # the half-edges of every edge, side by side
    start = np.concatenate([[0], np.cumsum(n)])[:-1]
    pairs = np.nonzero(n == 2)[0]
    h1, h2 = he[order[start[pairs]]], he[order[start[pairs] + 1]]
    m = manifold[pairs]
    twin[h1[m]], twin[h2[m]] = h2[m], h1[m]

    nxt = lambda h: h - 2 if h % 3 == 2 else h + 1
    corner = lambda h, v: h if flat[h] == v else nxt(h)              # the corner at v of the face of half-edge h (v is one of its two ends)
    fans = UnionFind(3 * F)
    if _bug == "fans_across_nonmanifold":
        groups = [(he[order[start[k]:start[k] + n[k]]], e["key"][k]) for k in np.nonzero(n >= 2)[0]]
    else:
        groups = [((p, q), e["key"][k]) for p, q, k in zip(h1.tolist(), h2.tolist(), pairs.tolist())]
    for hs, (a, b) in groups:
        for q in hs[1:]:
            fans.unite(corner(int(hs[0]), a), corner(int(q), a))
            fans.unite(corner(int(hs[0]), b), corner(int(q), b))
    roots = np.array([h for h in he.tolist() if fans.find(h) == h], dtype=np.int64)
    vertex_fans = np.bincount(flat[roots], minlength=V).astype(np.uint32) if V else np.zeros(0, dtype=np.uint32)

    loops = UnionFind(V)
    bkeys = e["key"][boundary]
    for a, b in bkeys.tolist():
        loops.unite(a, b)
    loop_sizes = np.bincount([loops.find(a) for a in bkeys[:, 0].tolist()], minlength=max(V, 1))
    loop_sizes = np.sort(loop_sizes[loop_sizes > 0])[::-1]

    per = (lambda mask: int(n[mask].sum())) if _bug == "per_half_edge" else (lambda mask: int(mask.sum()))
    info = np.zeros(16, dtype=np.uint32)
    info[:12] = [proper.sum(), degenerate.sum(), bad.sum(), (vertex_fans > 0).sum(), per(n > 0), per(boundary), per(flipped), per(nonmanifold),
                 (vertex_fans > 1).sum(), len(loop_sizes), loop_sizes[0] if len(loop_sizes) else 0, 0]
    return {"twin": twin, "edge_uses": uses, "vertex_fans": vertex_fans, "info": info, "loop_sizes": loop_sizes}


def face_terms(verts, faces):
    """(area terms, volume terms) [F] float64 of the faces given (all proper), vertices promoted from float32, in the header's operation order;
    numpy rounds every elementwise operation once."""
    v = np.asarray(verts, dtype=np.float32).astype(np.float64).reshape(-1, 3)
    f = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    a, b, c = v[f[:, 0]], v[f[:, 1]], v[f[:, 2]]
    u, w = b - a, c - a
    nx, ny, nz = u[:, 1] * w[:, 2] - u[:, 2] * w[:, 1], u[:, 2] * w[:, 0] - u[:, 0] * w[:, 2], u[:, 0] * w[:, 1] - u[:, 1] * w[:, 0]
    area = 0.5 * np.sqrt((nx * nx + ny * ny) + nz * nz)
    mx, my, mz = b[:, 1] * c[:, 2] - b[:, 2] * c[:, 1], b[:, 2] * c[:, 0] - b[:, 0] * c[:, 2], b[:, 0] * c[:, 1] - b[:, 1] * c[:, 0]
    volume = ((a[:, 0] * mx + a[:, 1] * my) + a[:, 2] * mz) / 6.0
    return area, volume


def component_stats(verts, faces, V, label):
    """dict: counts [V, 6] uint32 by label (COUNTS names the columns), measure [V, 2] float64 by label - math.fsum of the component's terms, the
    correctly rounded exact sum -, abs_sum [V, 2] - fsum of |term| - and faces [V]: what the summation bound m 2^-53 sum|term| is made of."""
    f = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    label = np.asarray(label, dtype=np.int64)
    proper = classify(f, V)[0]
    t = topology(f, V)
    e = edges(f, V)
    n = e["n_fwd"] + e["n_bwd"]
    manifold = (e["n_fwd"] == 1) & (e["n_bwd"] == 1)
    counts = np.zeros((V, 6), dtype=np.uint32)
    elab = label[e["key"][:, 0]]
    for col, lab in ((0, label[t["vertex_fans"] > 0]), (1, elab), (2, label[f[proper, 0]]), (3, elab[n == 1]), (4, elab[(n == 2) & ~manifold]),
                     (5, elab[n > 2])):
        counts[:, col] = np.bincount(lab, minlength=V)[:V] if V else 0
    area, volume = face_terms(verts, f[proper])
    flab = label[f[proper, 0]]
    measure, abs_sum = np.zeros((V, 2)), np.zeros((V, 2))
    for r in np.unique(flab).tolist():
        for col, term in ((0, area[flab == r]), (1, volume[flab == r])):
            measure[r, col], abs_sum[r, col] = math.fsum(term.tolist()), math.fsum(np.abs(term).tolist())
    return {"counts": counts, "measure": measure, "abs_sum": abs_sum, "faces": counts[:, 2].astype(np.int64)}


def summary(info):
    """The dict mesh_util.mesh_topology returns without its components: the counts by name and the verdicts."""
    d = {k: int(x) for k, x in zip(INFO, info)}
    d["euler"] = d["referenced_vertices"] - d["edges"] + d["proper_faces"]
    d["closed"] = d["boundary_edges"] == 0
    d["oriented"] = d["flipped_edges"] == 0
    d["manifold"] = d["nonmanifold_edges"] == 0 and d["bowtie_vertices"] == 0
    d["watertight"] = d["closed"] and d["oriented"] and d["manifold"] and d["bad_faces"] == 0 and d["degenerate_faces"] == 0
    return d


def report(verts, faces):
    """mesh_util.mesh_topology(verts, faces, components=True) without its tensors: summary(...) plus "components", one dict per label in
    mesh_components_ref.ranked's order."""
    V = len(verts)
    t = topology(faces, V)
    label, n_faces, _ = mesh_components_ref.components(faces, V)
    s = component_stats(verts, faces, V, label)
    bow = np.bincount(label[t["vertex_fans"] > 1], minlength=max(V, 1))
    out = summary(t["info"])
    out["components"] = []
    for r in mesh_components_ref.ranked(label, n_faces)[0].tolist():
        v, e, f, b, fl, nm = (int(x) for x in s["counts"][r])
        euler = v - e + f
        ok = b == 0 and fl == 0 and nm == 0 and bow[r] == 0
        out["components"].append({"label": r, "vertices": v, "edges": e, "faces": f, "boundary_edges": b, "flipped_edges": fl, "nonmanifold_edges": nm,
                                  "bowtie_vertices": int(bow[r]), "euler": euler, "closed": b == 0, "area": float(s["measure"][r, 0]),
                                  "volume": float(s["measure"][r, 1]), "genus": (2 - euler) // 2 if ok else None})
    return out


# ---- the hand meshes the tests share -----------------------------------------------------------------------------------------------------------

TETRAHEDRON = np.array([[0, 2, 1], [0, 1, 3], [0, 3, 2], [1, 2, 3]], dtype=np.int32)       # outward for vertices 0, e_x, e_y, e_z


def grid_faces(n, m, wrap_u=False, wrap_v=False):
    """(V, faces): an n x m grid of quads, each cut into two triangles with one orientation; wrap_u / wrap_v glue the opposite sides (both: a
    torus, one: an annulus, none: a sheet)."""
    nu, nv = (n if wrap_u else n + 1), (m if wrap_v else m + 1)
    idx = lambda i, j: (i % nu) * nv + (j % nv)
    faces = []
    for i in range(n):
        for j in range(m):
            p, q, r, s = idx(i, j), idx(i + 1, j), idx(i + 1, j + 1), idx(i, j + 1)
            faces += [[p, q, r], [p, r, s]]
    return nu * nv, np.array(faces, dtype=np.int32)


def moebius_faces(n):
    """(V, faces): a band of n quads over two rows of n vertices, closed with a half twist."""
    faces = []
    for i in range(n):
        p, s = i, n + i
        q, r = (i + 1, n + i + 1) if i + 1 < n else (n, 0)                                # the twist: the last quad meets the first row swapped
        faces += [[p, q, r], [p, r, s]]
    return 2 * n, np.array(faces, dtype=np.int32)
