"""The three rules of the mesh-vertex entry points (include/nerfart_hip.h: nerfart_mc_emit_edges, nerfart_mesh_edge_points,
nerfart_mesh_edge_refine_step) stated in numpy - the reference tests/test_gpu_mesh_vertices.py holds csrc/marching_cubes.hip and
csrc/mesh_vertices.hip to - plus the analytic fields the refinement is measured on and a PLY reader that understands the optional vertex
properties write_ply can add.  Every fp32 operation is a numpy float32 operation (one rounding, in the documented order); a one-rounding fma is
the float64 expression rounded once to float32 (the products here are exact in float64: a 24-bit significand times an index or another 24-bit
significand)."""
import numpy as np

F32 = np.float32


def bits(a):
    """The bit patterns of a float32 / integer array (what `equal bit for bit` compares: NaN and -0 included)."""
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


# ---- rule 1: edge records and the initial state -----------------------------------------------------------------------------------------------

def edge_records(vol, level=0.0):
    """vol [nx, ny, nz] float32 -> (edge [V] uint32, bracket [V, 4], t [V], best [V, 2], side [V] uint8), in marching cubes' vertex order: points
    in linear order, per point its sign-changing owned edges in axis order x, y, z (a corner is inside iff value < level)."""
    v = np.ascontiguousarray(vol, dtype=F32)
    nx, ny, nz = v.shape
    lvl = F32(level)
    inside = v < lvl
    flag = np.zeros((3, nx, ny, nz), dtype=bool)
    flag[0, :-1] = inside[:-1] != inside[1:]
    flag[1, :, :-1] = inside[:, :-1] != inside[:, 1:]
    flag[2, :, :, :-1] = inside[:, :, :-1] != inside[:, :, 1:]
    ax, ix, iy, iz = np.nonzero(flag)
    p = (ix * ny + iy) * nz + iz
    order = np.lexsort((ax, p))
    ax, p = ax[order], p[order]
    stride = np.array([ny * nz, nz, 1])
    flat = v.reshape(-1)
    a, b = flat[p], flat[p + stride[ax]]
    V = len(p)
    with np.errstate(all="ignore"):
        t = ((lvl - a) / (b - a)).astype(F32)
    bracket = np.stack([np.zeros(V, F32), a - lvl, np.ones(V, F32), b - lvl], -1).astype(F32)
    best = np.stack([t, np.full(V, np.inf, F32)], -1).astype(F32)
    return (3 * p + ax).astype(np.uint32), bracket, t, best, np.zeros(V, np.uint8)


# ---- rule 2: the point on the edge --------------------------------------------------------------------------------------------------------------

def fma32(a, b, c):
    """fmaf on float32 arrays: the float64 a * b + c, rounded once."""
    return (np.asarray(a, F32).astype(np.float64) * np.asarray(b, F32).astype(np.float64) + np.asarray(c, F32).astype(np.float64)).astype(F32)


def edge_points(edge, t, dims, origin, spacing):
    """[V, 3] float32: pa[c] = fma(idx[c], spacing[c], origin[c]); on the edge's axis pb = fma(idx + 1, spacing, origin) and
    q = fma(t, pb - pa, pa).  Every edge must be one of the volume's."""
    nx, ny, nz = (int(d) for d in dims)
    e = np.asarray(edge).astype(np.int64)
    p, ax = e // 3, e % 3
    idx = np.stack([p // (ny * nz), (p // nz) % ny, p % nz], -1)
    assert (p < nx * ny * nz).all() and (idx[np.arange(len(p)), ax] + 1 < np.array([nx, ny, nz])[ax]).all()
    o, s = np.asarray(origin, F32), np.asarray(spacing, F32)
    pa = fma32(idx.astype(F32), s[None, :], o[None, :])
    r = np.arange(len(p))
    pb = fma32((idx[r, ax] + 1).astype(F32), s[ax], o[ax])
    out = pa.copy()
    out[r, ax] = fma32(np.asarray(t, F32), pb - pa[r, ax], pa[r, ax])
    return out


# ---- rule 3: one refinement step ------------------------------------------------------------------------------------------------------------------

def refine_step(f, level, bracket, t, best, side):
    """One step of bracket-keeping false position with the Illinois modification, in float32: new (bracket, t, best, side), the inputs untouched."""
    f, lvl = np.asarray(f, F32), F32(level)
    br, t, bs, sd = (np.array(bracket, F32), np.array(t, F32), np.array(best, F32), np.array(side, np.uint8))
    with np.errstate(all="ignore"):
        g = f - lvl
        win = np.abs(g) < np.abs(bs[:, 1])                             # 1 (false for NaN)
        bs[win, 0], bs[win, 1] = t[win], g[win]
        nan = np.isnan(g)                                              # 2
        zero = g == 0                                                  # 3
        br[zero] = np.stack([t, np.zeros_like(t), t, np.zeros_like(t)], -1)[zero]
        sd[zero] = 0
        live = ~nan & ~zero
        t0, g0, t1, g1 = (br[:, k].copy() for k in range(4))
        same = live & ((g < 0) == (g0 < 0))                            # 4
        other = live & ~same
        h1, h0 = same & (sd == 1), other & (sd == 2)
        g1[h1] = g1[h1] * F32(0.5)
        g0[h0] = g0[h0] * F32(0.5)
        t0[same], g0[same], sd[same] = t[same], g[same], 1
        t1[other], g1[other], sd[other] = t[other], g[other], 2
        tn = t0 - (g0 * (t1 - t0)) / (g1 - g0)                         # 5
        mid = F32(0.5) * (t0 + t1)
        tn = np.where(np.isfinite(tn), tn, mid)
        tn = np.minimum(np.maximum(tn, np.minimum(t0, t1)), np.maximum(t0, t1))
    br[live] = np.stack([t0, g0, t1, g1], -1)[live]
    t[live] = tn[live]
    return br, t, bs, sd


def next_t64(bracket):
    """Step 5 on an updated bracket in float64: (t, q, finite) - the unclamped estimate t0 - q, q = g0 (t1 - t0) / (g1 - g0), and where it is finite."""
    b = np.asarray(bracket, F32).astype(np.float64)
    with np.errstate(all="ignore"):
        q = b[:, 1] * (b[:, 2] - b[:, 0]) / (b[:, 3] - b[:, 1])
        tn = b[:, 0] - q
    return tn, q, np.isfinite(tn)


def refine_loop(vol, level, origin, spacing, field, n_evals, records=edge_records, points=edge_points, step=refine_step, host=np.asarray):
    """The loop of mesh_util.refine_vertices with the three stages as arguments (numpy here, the kernels in the GPU test) and an analytic
    `field(x, y, z)` (float64 in, float64 out; rounded to float32: the SDF the step is handed); host: state array -> numpy.  Returns (t_best [V], history [n_evals, V] of
    |g_best| after each evaluation)."""
    edge, bracket, t, best, side = records(vol, level)
    hist = []
    for _ in range(n_evals):
        q = np.asarray(points(edge, t, vol.shape, origin, spacing)).astype(np.float64)
        f = field(q[:, 0], q[:, 1], q[:, 2]).astype(F32)
        bracket, t, best, side = step(f, level, bracket, t, best, side)
        hist.append(np.abs(host(best)[:, 1]).copy())
    return host(best)[:, 0].copy(), np.stack(hist)


# ---- analytic fields: name -> (field, grid points per axis over [-1, 1]^3) ---------------------------------------------------------------------

def sphere(x, y, z):
    return np.sqrt(x * x + y * y + z * z) - 0.6


def torus(x, y, z):
    return np.sqrt((np.sqrt(x * x + y * y) - 0.5) ** 2 + z * z) - 0.2


def bumpy_sphere(x, y, z):
    return np.sqrt(x * x + y * y + z * z) - 0.6 + 0.05 * np.sin(9 * x) * np.sin(7 * y) * np.cos(8 * z)


FIELDS = {"sphere": (sphere, 33), "torus": (torus, 49), "bumpy_sphere": (bumpy_sphere, 33)}


def field_volume(name):
    """(vol [N, N, N] float32, origin, spacing): the field on the N^3 grid over [-1, 1]^3, evaluated in float64 and rounded."""
    field, N = FIELDS[name]
    g = np.linspace(-1.0, 1.0, N)
    X, Y, Z = np.meshgrid(g, g, g, indexing="ij")
    return field(X, Y, Z).astype(F32), [-1.0] * 3, [2.0 / (N - 1)] * 3


def check_refinement(name, t_best, hist):
    """The three demands on a 5-evaluation refinement of an analytic field; returns (max |g_best| after 1 evaluation, after the last)."""
    assert hist.shape[0] == 5 and hist.shape[1] == len(t_best) > 0
    assert ((t_best >= 0) & (t_best <= 1)).all(), name
    assert (hist[1:] <= hist[:-1]).all(), name
    first, last = float(hist[0].max()), float(hist[-1].max())
    print(f"[refine] {name}: V = {len(t_best)}, max |g_best| after 1 evaluation {first:.3e}, after 5 {last:.3e}, ratio {first / max(last, 1e-300):.3g}")
    assert last <= first / 100.0, (name, first, last)
    return first, last


# ---- PLY -------------------------------------------------------------------------------------------------------------------------------------------

def read_ply(path):
    """A binary little-endian PLY as mesh_util.write_ply writes it -> dict(header, verts [V, 3] float32, faces [F, 3] int32, normals [V, 3]
    float32 or None, colors [V, 3] uint8 or None).  Vertex properties: x y z, then optionally nx ny nz (float), then optionally red green blue
    (uchar); anything else is an AssertionError."""
    raw = open(path, "rb").read()
    end = raw.index(b"end_header\n") + len(b"end_header\n")
    header = raw[:end].decode("ascii")
    lines = header.split("\n")
    assert lines[0] == "ply" and lines[1] == "format binary_little_endian 1.0" and lines[2].startswith("element vertex "), header
    V = int(lines[2].split()[-1])
    k = 3
    props = []
    while lines[k].startswith("property "):
        props.append(lines[k])
        k += 1
    xyz = ["property float x", "property float y", "property float z"]
    nrm = ["property float nx", "property float ny", "property float nz"]
    col = ["property uchar red", "property uchar green", "property uchar blue"]
    assert props[:3] == xyz, header
    rest, fields = props[3:], [("p", "<f4", (3,))]
    if rest[:3] == nrm:
        fields.append(("n", "<f4", (3,)))
        rest = rest[3:]
    if rest[:3] == col:
        fields.append(("c", "u1", (3,)))
        rest = rest[3:]
    assert rest == [], header
    assert lines[k].startswith("element face ") and lines[k + 1:] == ["property list uchar int vertex_indices", "end_header", ""], header
    F = int(lines[k].split()[-1])
    vdt, fdt = np.dtype(fields), np.dtype([("n", "u1"), ("i", "<i4", (3,))])
    payload = raw[end:]
    assert len(payload) == V * vdt.itemsize + F * fdt.itemsize, (len(payload), V, F)
    vrec = np.frombuffer(payload, dtype=vdt, count=V)
    frec = np.frombuffer(payload, dtype=fdt, count=F, offset=V * vdt.itemsize)
    assert (frec["n"] == 3).all()
    names = vrec.dtype.names
    return dict(header=header, verts=vrec["p"].copy(), faces=frec["i"].astype(np.int32),
                normals=vrec["n"].copy() if "n" in names else None, colors=vrec["c"].copy() if "c" in names else None)
