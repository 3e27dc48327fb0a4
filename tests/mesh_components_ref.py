"""Connected components of an indexed triangle mesh and the compaction that drops some of them, in plain numpy / Python - the statement
tests/test_gpu_mesh_components.py holds csrc/mesh_components.hip to, integer for integer (include/nerfart_hip.h has the rule):

  * two vertices are connected when a face contains both (vertex connectivity: triangles sharing one vertex are one component); a vertex in no
    face is its own component; label[v] = the smallest vertex index of v's component (a union-find that links the larger root under the smaller);
  * a face with an index outside [0, V) is bad: it joins nothing, is counted nowhere, never survives, and sets the flag;
  * rank: face count descending, ties broken by the smaller label;
  * a component survives iff (keep_largest is None or rank < keep_largest) and (min_faces is None or its face count >= min_faces);
  * compaction: vertex v survives iff keep[label[v]], face f iff it is good and keep[label[faces[f][0]]]; both keep their old order, face
    indices are replaced by the number of surviving vertices before them.
"""
import numpy as np


def good_faces(faces, V):
    """[F] bool: every index of the face in [0, V)."""
    f = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    return ((f >= 0) & (f < V)).all(axis=1)


def components(faces, V):
    """(label [V] int32, n_faces [V] uint32 - at index r the face count of the component labelled r, 0 elsewhere -,
    info [3] = (components, components with at least one face, bad))."""
    f = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    good = good_faces(f, V)
    parent = list(range(V))

    def find(v):
        root = v
        while parent[root] != root:
            root = parent[root]
        while parent[v] != root:
            parent[v], v = root, parent[v]
        return root

    def unite(a, b):
        a, b = find(a), find(b)
        if a != b:
            parent[max(a, b)] = min(a, b)

    for a, b, c in f[good].tolist():
        unite(a, b)
        unite(a, c)
    label = np.array([find(v) for v in range(V)], dtype=np.int32).reshape(V)
    n_faces = np.bincount(label[f[good][:, 0]], minlength=V).astype(np.uint32) if V else np.zeros(0, dtype=np.uint32)
    n_comp = int((label == np.arange(V)).sum())
    info = np.array([n_comp, int((n_faces > 0).sum()), int(not good.all())], dtype=np.uint32)
    return label, n_faces, info


def ranked(label, n_faces):
    """(roots [C] int32 in rank order, their face counts [C] int32)."""
    roots = np.nonzero(label == np.arange(len(label)))[0]
    order = sorted(range(len(roots)), key=lambda i: (-int(n_faces[roots[i]]), int(roots[i])))
    roots = roots[order]
    return roots.astype(np.int32), n_faces[roots].astype(np.int32)


def keep_mask(label, n_faces, keep_largest=None, min_faces=None):
    """keep [V] uint8, indexed by label."""
    roots, count = ranked(label, n_faces)
    ok = np.ones(len(roots), dtype=bool)
    if keep_largest is not None:
        ok &= np.arange(len(roots)) < keep_largest
    if min_faces is not None:
        ok &= count >= min_faces
    keep = np.zeros(len(label), dtype=np.uint8)
    keep[roots[ok]] = 1
    return keep


def compact(label, keep, faces, V):
    """(src_vertex [V'] int32, faces_out [F', 3] int32)."""
    f = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    vkeep = keep[label].astype(bool) if V else np.zeros(0, dtype=bool)
    fkeep = good_faces(f, V)
    fkeep[fkeep] = vkeep[f[fkeep][:, 0]]
    new = np.cumsum(vkeep) - vkeep                     # surviving vertices before v
    return np.nonzero(vkeep)[0].astype(np.int32), new[f[fkeep]].astype(np.int32).reshape(-1, 3)


def filter_components(n_verts, faces, keep_largest=None, min_faces=None):
    """(src_vertex, faces_out) of the mesh with the components that do not survive dropped."""
    label, n_faces, _ = components(faces, n_verts)
    return compact(label, keep_mask(label, n_faces, keep_largest, min_faces), faces, n_verts)


# ---- the meshes the tests share ---------------------------------------------------------------------------------------------------------------

def three_spheres():
    """min of three sphere SDFs on a 20^3 grid over [-1, 1]^3, float32."""
    g = np.linspace(-1.0, 1.0, 20, dtype=np.float32)
    X, Y, Z = np.meshgrid(g, g, g, indexing="ij")
    vol = None
    for (cx, cy, cz), r in (((-0.35, 0.0, 0.0), 0.4), ((0.55, 0.5, 0.5), 0.25), ((0.6, -0.6, -0.6), 0.12)):
        d = np.sqrt((X - np.float32(cx)) ** 2 + (Y - np.float32(cy)) ** 2 + (Z - np.float32(cz)) ** 2) - np.float32(r)
        vol = d if vol is None else np.minimum(vol, d)
    return vol.astype(np.float32)


def triangle_strip(n_faces):
    """Faces (i, i + 1, i + 2), i < n_faces, over n_faces + 2 vertices: one component, parent chains as long as the mesh."""
    i = np.arange(n_faces, dtype=np.int32)
    return np.stack([i, i + 1, i + 2], axis=1)
