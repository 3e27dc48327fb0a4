"""The marching-cubes entry points' argument checks and workspace size (host arithmetic: nothing is launched, no GPU needed)."""
import ctypes as C

import pytest


def _total(sizes):
    return sum((b + 255) // 256 * 256 for b in sizes)


def _levels(n, block=512):
    """Lengths of the block-sum levels that live in the workspace: ceil(n / 512), ceil(that / 512), ... while above 1."""
    out, m = [], -(-n // block)
    while m > 1:
        out.append(m)
        m = -(-m // block)
    return out


def test_workspace_is_the_sum_of_its_documented_buffers():
    from nerfart_amd import hip
    for nx, ny, nz in ((2, 2, 2), (8, 8, 8), (5, 7, 70), (70, 70, 70), (512, 512, 512), (2, 2, 178956970)):
        n = nx * ny * nz
        want = _total([n, n, 8 * n] + [8 * m for m in _levels(n)])            # flags, cases, (vertex, triangle) offsets, block sums per level
        assert hip.lib.nerfart_mc_workspace_bytes(nx, ny, nz) == want, (nx, ny, nz)
    assert _levels(8) == [] and _levels(70 ** 3) == [670, 2] and _levels(512 ** 3) == [262144, 512]


def test_bad_arguments_are_refused_before_any_launch():
    from nerfart_amd import hip
    lib, null, one = hip.lib, C.c_void_p(0), C.c_void_p(256)       # `one`: non-null, aligned, never dereferenced - the checks come first

    def err():
        return lib.nerfart_last_error().decode()

    for dims in ((1, 8, 8), (8, 1, 8), (8, 8, 1), (0, 8, 8), (-4, 8, 8)):
        assert lib.nerfart_mc_workspace_bytes(*dims) == 0 and ">= 2" in err()
        assert lib.nerfart_mc_count(one, *dims, 0.0, one, 1 << 30, one, null) == 2 and ">= 2" in err()
        assert lib.nerfart_mc_emit(one, *dims, 0.0, one, one, one, 1 << 30, one, one, 3, 1, null) == 2 and ">= 2" in err()
    for dims in ((1024, 1024, 1024), (2, 2, 178956971), (65536, 65536, 2)):       # 3 n >= 2^31
        assert lib.nerfart_mc_workspace_bytes(*dims) == 0 and "2^31" in err()
        assert lib.nerfart_mc_count(one, *dims, 0.0, one, 1 << 40, one, null) == 2 and "2^31" in err()
    assert lib.nerfart_mc_workspace_bytes(2, 2, 178956970) > 0                    # 3 n = 2^31 - 8
    # below the size limit, but long in x and thin in y / z: one block per (x, 4 rows, 64 points along z) would be more blocks than a launch takes
    for dims in ((178956970, 2, 2), (16777216, 4, 8), (2, 178956970, 2)):
        assert lib.nerfart_mc_workspace_bytes(*dims) == 0 and "2^24" in err()
        assert lib.nerfart_mc_count(one, *dims, 0.0, one, 1 << 40, one, null) == 2 and "2^24" in err()
        assert lib.nerfart_mc_emit(one, *dims, 0.0, one, one, one, 1 << 40, one, one, 3, 1, null) == 2 and "2^24" in err()
    assert lib.nerfart_mc_workspace_bytes(16777215, 4, 8) > 0
    need = lib.nerfart_mc_workspace_bytes(8, 8, 8)
    for args in ((null, 8, 8, 8, 0.0, one, need, one, null), (one, 8, 8, 8, 0.0, null, need, one, null), (one, 8, 8, 8, 0.0, one, need, null, null)):
        assert lib.nerfart_mc_count(*args) == 2 and "null" in err()
    assert lib.nerfart_mc_count(one, 8, 8, 8, 0.0, one, need - 1, one, null) == 2 and "workspace" in err()
    assert lib.nerfart_mc_count(one, 8, 8, 8, 0.0, C.c_void_p(260), need, one, null) == 2 and "aligned" in err()
    assert lib.nerfart_mc_count(one, 8, 8, 8, 0.0, one, need, C.c_void_p(260), null) == 2 and "aligned" in err()
    emit = lambda **kw: lib.nerfart_mc_emit(*[kw.get(k, d) for k, d in (("vol", one), ("nx", 8), ("ny", 8), ("nz", 8), ("level", 0.0), ("origin", one),
                                                                       ("spacing", one), ("ws", one), ("ws_bytes", need), ("verts", one), ("faces", one),
                                                                       ("V", 3), ("F", 1), ("stream", null))])
    for k in ("vol", "origin", "spacing", "ws", "verts", "faces"):
        assert emit(**{k: null}) == 2 and "null" in err(), k
    assert emit(ws_bytes=need - 1) == 2 and "workspace" in err()
    assert emit(V=0, vol=null) == 0 and emit(F=0, vol=null) == 0                  # an empty mesh launches nothing and succeeds


def test_python_front_refuses_cpu_tensors():
    import torch
    from nerfart_amd import hip, mesh_util
    with pytest.raises(hip.NerfartHipError, match="GPU"):
        mesh_util.marching_cubes(torch.ones(4, 4, 4))
    with pytest.raises(hip.NerfartHipError):
        mesh_util.marching_cubes(torch.ones(4, 4))
