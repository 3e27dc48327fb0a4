"""The six kernels of csrc/pass2_operands.hip on the GPU - nerfart_ray_points, nerfart_volsdf_pass2_cotangents and the four nerfart_wgrad_operand_* -
against the fp64 references, intervals and allowances of tests/pass2_operand_ref.py, on the sizes tests/test_pass2_operand_ref.py runs the
stand-ins and their mutants through on the CPU.  Called through hip.lib and ctypes on buffers of the test's own: every output pre-filled with 0xFF
bytes and followed by a 4096-byte guard tail that must come back untouched; every call runs twice and must give the same bits.  Bit equality, with
no allowance: view = NULL and d4 = NULL against the full call, the empty launches, every padding row and column (0x0000), pts, view, the exact
operand columns, sbar (0.0 or the bits of g_sdf).

The zero-nabla case: three exact-zero nablas and three with |n| = 1e-15 among ordinary ones, w = 0.1.  nbar and eik_ray must be finite and within
the allowance of torch's fp64 autograd, which gives a zero subgradient at n = 0: the eikonal share of nbar is exactly 0 there and eik_ray counts
(0 - 1)^2.  Nablas whose squares underflow fp32 are out of scope.

OBSERVED on an MI355X (gfx950), worst observed / allowed over all sizes; for the bf16 operands the figure is the smallest fraction of E that explains
every hi and lo entry (0 = every entry is the rounding of the fp64 value itself).  In brackets: what the fp32 stand-in reaches on the CPU.  Every
case passed, and every exact check - guard tails, two runs, NULL view / d4, empty launches, padding, refusals - held bit for bit.
  nerfart_wgrad_operand_embed_pair   exact columns and multires < 0: bit-equal;  value 0.125 (0.000: its sin / cos are correctly rounded)
                                     tangent 0.191 (0.098) - both at the widths with a lo half (multires 1 and 4); hi alone (5, 6, 10): 0.000
  nerfart_wgrad_operand_inputs       0.117 at (2, 1), 0.082 at (-1, 3) (0.000); 0.000 at the widths without a lo half
  nerfart_wgrad_operand_rgb_delta    operand against the returned d4: bit-equal;  d4 0.779 (0.633: the same three roundings; the bound is their
                                     count, not FACTOR times it);  block_sums 0.027 (0.022)
  nerfart_wgrad_operand_sbar_ones    bit-equal
  nerfart_ray_points                 pts and view bit-equal (a fused o + d t would differ on 30 to 35 % of the elements of these cases)
  nerfart_volsdf_pass2_cotangents    sbar: every element an allowed 0.0 or the allowed bits of g_sdf, R_bg = 0 included;
                                     nbar 0.221 (0.221), against the first allowance A1 0.735 (0.735);  eik_ray 0.195 (0.195), 0.163 at P = 65 (0.102)
  zero nablas                        nbar 0.137, against A1 0.380;  eik_ray 0.195 (the same on the CPU)
  FINDING: the zero-nabla case WAS a bug.  With the kernel as it stood (k = 2 w coef (|n| - 1) / |n|, then fmaf(k, n, b)) the three samples with
  n = 0 gave nbar = (NaN, NaN, NaN), 9 non-finite elements in every call of the case, and nothing else in this file failed; with the guard
  (k = 0 at |n| = 0) the case passes and every other figure above is unchanged, bit for bit where the check is one.  The samples with |n| = 1e-15
  were finite before and after.
  No sin / cos value fell outside 4 ulp + 2^-31, at any octave up to 2^9 |x|, |x| <= 2.2.
"""
import functools

import numpy as np
import pytest
import torch

import pass2_operand_ref as P

pytestmark = pytest.mark.gpu
DEV = "cuda"
GUARD = 4096


# ---- plumbing --------------------------------------------------------------------------------------------------------------------------
def _lib():
    from nerfart_amd import hip
    return hip.lib


def _st():
    return torch.cuda.current_stream().cuda_stream


class Buf:
    """nbytes of the test's own + a guard tail, all 0xFF."""

    def __init__(self, nbytes):
        self.n = int(nbytes)
        self.t = torch.full((self.n + GUARD,), P.FILL, dtype=torch.uint8, device=DEV)

    @property
    def ptr(self):
        return self.t.data_ptr()

    def u16(self, *shape):
        return self.t[: self.n].cpu().numpy().view(np.uint16).reshape(*shape)

    def f32(self, *shape):
        return self.t[: self.n].cpu().numpy().view(np.float32).reshape(*shape)

    def guard_ok(self):
        return bool((self.t[self.n:] == P.FILL).all())

    def untouched(self):
        return bool((self.t == P.FILL).all())


@functools.lru_cache(maxsize=None)
def _dev(key, name):
    """A case's input on the device (the cases are cached by the reference module; key = (maker name, args))."""
    make, args = key
    return torch.from_numpy(np.ascontiguousarray(getattr(P, make)(*args)[name])).to(DEV)


def _p(t):
    return None if t is None else t.data_ptr()


def _twice(call, bufs):
    """call(bufs()) twice on fresh buffers -> the first run's buffers; the two runs agree in every byte and the guards hold."""
    runs = []
    for _ in range(2):
        b = bufs()
        rc = call(b)
        assert rc == 0, (rc, _lib().nerfart_last_error().decode())
        torch.cuda.synchronize()
        assert all(v.guard_ok() for v in b.values() if v is not None), "a kernel wrote past the end of an output"
        runs.append(b)
    for k in runs[0]:
        if runs[0][k] is not None:
            assert torch.equal(runs[0][k].t, runs[1][k].t), f"two runs differ in {k}"
    return runs[0]


WORST = {}


def _note(entry, ratio):
    for k, v in ratio.items():
        WORST[entry, k] = max(WORST.get((entry, k), 0.0), v)


def _summary(entry):
    return f"\n{entry}: worst observed / allowed  " + "  ".join(f"{k} {v:.3f}" for (e, k), v in WORST.items() if e == entry)


# ---- the operand kernels -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("multires", P.EMBED_MULTIRES)
def test_embed_pair(multires):
    lib = _lib()
    for M in P.M_SIZES:
        c, key = P.embed_case(M, multires), ("embed_case", (M, multires))
        x, d = _dev(key, "pts"), _dev(key, "dir")
        for rp in P.rows_pads(M):
            b = _twice(lambda b: lib.nerfart_wgrad_operand_embed_pair(x.data_ptr(), d.data_ptr(), M, rp, multires, b["out"].ptr, _st()), lambda: dict(out=Buf(2 * rp * 128)))
            viol, ratio = P.check_embed_pair(c, rp, b["out"].u16(2 * rp, 64))
            assert not viol, viol
            _note(f"embed_pair[{multires}]", ratio)
    print(_summary(f"embed_pair[{multires}]"))


@pytest.mark.parametrize("mx,mv", P.INPUT_MULTIRES)
def test_inputs(mx, mv):
    lib = _lib()
    for M in P.M_SIZES:
        c, key = P.inputs_case(M, mx, mv), ("inputs_case", (M, mx, mv))
        x, v, n = _dev(key, "x"), _dev(key, "view"), _dev(key, "normals")
        for rp in P.rows_pads(M):
            b = _twice(lambda b: lib.nerfart_wgrad_operand_inputs(x.data_ptr(), mx, v.data_ptr(), mv, n.data_ptr(), M, rp, b["out"].ptr, _st()), lambda: dict(out=Buf(rp * 128)))
            viol, ratio = P.check_inputs(c, rp, b["out"].u16(rp, 64))
            assert not viol, viol
            _note(f"inputs[{mx},{mv}]", ratio)
    print(_summary(f"inputs[{mx},{mv}]"))


def test_rgb_delta():
    lib = _lib()
    for M in P.M_SIZES:
        c, key = P.rgb_case(M), ("rgb_case", (M,))
        rgb, g = _dev(key, "rgb")[:M].contiguous(), _dev(key, "g_rgb")[:M].contiguous()
        for rp in P.rows_pads(M):
            nb = (rp + 31) // 32
            full = _twice(lambda b: lib.nerfart_wgrad_operand_rgb_delta(rgb.data_ptr(), g.data_ptr(), M, rp, b["out"].ptr, b["d4"].ptr, b["sums"].ptr, _st()),
                          lambda: dict(out=Buf(rp * 128), d4=Buf(M * 12), sums=Buf(nb * 12)))
            viol, ratio = P.check_rgb_delta(c, rp, full["out"].u16(rp, 64), full["d4"].f32(M, 3), full["sums"].f32(nb, 3))
            assert not viol, viol
            _note("rgb_delta", ratio)
            nod4 = _twice(lambda b: lib.nerfart_wgrad_operand_rgb_delta(rgb.data_ptr(), g.data_ptr(), M, rp, b["out"].ptr, None, b["sums"].ptr, _st()),
                          lambda: dict(out=Buf(rp * 128), sums=Buf(nb * 12)))
            assert torch.equal(nod4["out"].t, full["out"].t) and torch.equal(nod4["sums"].t, full["sums"].t), "d4 = NULL changes the other outputs"
    print(_summary("rgb_delta"))


def test_sbar_ones():
    lib = _lib()
    for M in P.M_SIZES:
        c, key = P.sbar_case(M), ("sbar_case", (M,))
        s = _dev(key, "sbar")
        for rp in P.rows_pads(M):
            b = _twice(lambda b: lib.nerfart_wgrad_operand_sbar_ones(s.data_ptr(), M, rp, b["out"].ptr, _st()), lambda: dict(out=Buf(2 * rp * 128)))
            viol, ratio = P.check_sbar_ones(c, rp, b["out"].u16(2 * rp, 64))
            assert not viol, viol
            _note("sbar_ones", ratio)
    print(_summary("sbar_ones"))


# ---- ray points and cotangents ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("R,Pn", P.RAY_SIZES)
def test_ray_points(R, Pn):
    lib = _lib()
    c, key = P.ray_case(R, Pn), ("ray_case", (R, Pn))
    o, dn, t = _dev(key, "o"), _dev(key, "dn"), _dev(key, "depth")
    M = R * Pn
    full = _twice(lambda b: lib.nerfart_ray_points(o.data_ptr(), dn.data_ptr(), t.data_ptr(), R, Pn, b["pts"].ptr, b["view"].ptr, _st()),
                  lambda: dict(pts=Buf(M * 12), view=Buf(M * 12)))
    viol, ratio = P.check_ray_points(c, full["pts"].f32(M, 3), full["view"].f32(M, 3))
    assert not viol, viol
    nov = _twice(lambda b: lib.nerfart_ray_points(o.data_ptr(), dn.data_ptr(), t.data_ptr(), R, Pn, b["pts"].ptr, None, _st()), lambda: dict(pts=Buf(M * 12)))
    assert torch.equal(nov["pts"].t, full["pts"].t), "view = NULL changes pts"


def _cot_call(lib, d, c, call, b):
    group, w, gn, ge, rb = call
    return lib.nerfart_volsdf_pass2_cotangents(d["pts"].data_ptr(), d["sdf"].data_ptr(), d["g_sdf"].data_ptr(), d["nabla"].data_ptr(), _p(d["g_n"] if gn else None),
                                               _p(d["g_n_extra"] if ge else None), c["R"], c["P"], rb, w, group, b["sbar"].ptr, b["nbar"].ptr, b["eik"].ptr, _st())


def _cot_bufs(c):
    M = c["R"] * c["P"]
    return lambda: dict(sbar=Buf(M * 4), nbar=Buf(M * 12), eik=Buf(c["R"] * 4))


@pytest.mark.parametrize("R,Pn", P.RAY_SIZES)
def test_cotangents(R, Pn):
    lib = _lib()
    c, key = P.cot_case(R, Pn), ("cot_case", (R, Pn))
    d = {k: _dev(key, k) for k in ("pts", "sdf", "g_sdf", "nabla", "g_n", "g_n_extra")}
    M = R * Pn
    for call in P.cot_calls(R):
        b = _twice(lambda b: _cot_call(lib, d, c, call, b), _cot_bufs(c))
        viol, ratio = P.check_cotangents(c, *call, b["sbar"].f32(M), b["nbar"].f32(M, 3), b["eik"].f32(R))
        assert not viol, viol
        _note(f"cotangents[{R}x{Pn}]", ratio)
    print(_summary(f"cotangents[{R}x{Pn}]"))


def test_zero_nabla():
    lib = _lib()
    c = P.zero_nabla_case()
    d = {k: torch.from_numpy(np.ascontiguousarray(c[k])).to(DEV) for k in ("pts", "sdf", "g_sdf", "nabla", "g_n", "g_n_extra")}
    R, M = c["R"], c["R"] * c["P"]
    for group in (0, 2):
        for gn in (True, False):
            call = (group, 0.1, gn, gn, 3.0)
            b = _twice(lambda b: _cot_call(lib, d, c, call, b), _cot_bufs(c))
            sbar, nbar, eik = b["sbar"].f32(M), b["nbar"].f32(M, 3), b["eik"].f32(R)
            assert bool(np.isfinite(nbar).all()) and bool(np.isfinite(eik).all()), f"{int((~np.isfinite(nbar)).sum())} non-finite nbar elements: the eikonal term at n = 0"
            viol, ratio = P.check_cotangents(c, *call, sbar, nbar, eik)
            assert not viol, viol
            _note("zero_nabla", ratio)
            if not gn:
                assert bool((nbar[c["zero_rows"]].view(np.uint32) << 1 == 0).all()), "the eikonal share of nbar at n = 0 is not exactly 0"
    print(_summary("zero_nabla"))


# ---- empty launches and refusals ---------------------------------------------------------------------------------------------------------------
def test_empty_launches():
    lib = _lib()
    rp = 64
    for name, call, rows in (("embed_pair", lambda o: lib.nerfart_wgrad_operand_embed_pair(None, None, 0, rp, 6, o.ptr, _st()), 2 * rp),
                             ("inputs", lambda o: lib.nerfart_wgrad_operand_inputs(None, -1, None, 4, None, 0, rp, o.ptr, _st()), rp)):
        o = Buf(rows * 128)
        assert call(o) == 0, name
        torch.cuda.synchronize()
        assert o.guard_ok() and not o.u16(rows, 64).any(), f"{name}: M = 0 must give an all-zero operand"
    o, sums = Buf(rp * 128), Buf(2 * 12)
    assert lib.nerfart_wgrad_operand_rgb_delta(None, None, 0, rp, o.ptr, None, sums.ptr, _st()) == 0
    torch.cuda.synchronize()
    assert o.guard_ok() and sums.guard_ok() and not o.u16(rp, 64).any() and not sums.f32(2, 3).view(np.uint32).any()
    o = Buf(2 * rp * 128)
    assert lib.nerfart_wgrad_operand_sbar_ones(None, 0, rp, o.ptr, _st()) == 0
    torch.cuda.synchronize()
    got, ones = o.u16(2 * rp, 64), np.zeros((rp, 64), np.uint16)
    ones[:, 0] = 0x3F80
    assert o.guard_ok() and not got[:rp].any() and np.array_equal(got[rp:], ones)
    # nothing to do at all: rows_pad = 0, n_rays = 0 - no launch, every buffer keeps its fill
    z = torch.zeros(3, device=DEV)
    bufs = [Buf(256) for _ in range(3)]
    assert lib.nerfart_wgrad_operand_embed_pair(z.data_ptr(), z.data_ptr(), 0, 0, 6, bufs[0].ptr, _st()) == 0
    assert lib.nerfart_wgrad_operand_inputs(z.data_ptr(), -1, z.data_ptr(), -1, z.data_ptr(), 0, 0, bufs[0].ptr, _st()) == 0
    assert lib.nerfart_wgrad_operand_rgb_delta(z.data_ptr(), z.data_ptr(), 0, 0, bufs[0].ptr, bufs[1].ptr, bufs[2].ptr, _st()) == 0
    assert lib.nerfart_wgrad_operand_sbar_ones(z.data_ptr(), 0, 0, bufs[0].ptr, _st()) == 0
    assert lib.nerfart_ray_points(z.data_ptr(), z.data_ptr(), z.data_ptr(), 0, 192, bufs[0].ptr, bufs[1].ptr, _st()) == 0
    assert lib.nerfart_volsdf_pass2_cotangents(z.data_ptr(), z.data_ptr(), z.data_ptr(), z.data_ptr(), None, None, 0, 192, 3.0, 0.1, 0, bufs[0].ptr, bufs[1].ptr,
                                               bufs[2].ptr, _st()) == 0
    torch.cuda.synchronize()
    assert all(b.untouched() for b in bufs)


def test_refusals():
    """Refused before any launch: non-zero, nerfart_last_error names the entry point, the 0xFF fill intact.  Tiny buffers do."""
    lib = _lib()
    z = torch.zeros(64, device=DEV)
    zp = z.data_ptr()
    o = [Buf(256) for _ in range(3)]
    o0, o1, o2 = (b.ptr for b in o)
    st = _st()
    big = 1 << 28
    calls = {
        "wgrad_operand_embed_pair": [lambda: lib.nerfart_wgrad_operand_embed_pair(zp, zp, 10, 8, 6, o0, st), lambda: lib.nerfart_wgrad_operand_embed_pair(zp, zp, 1, big, 6, o0, st),
                                     lambda: lib.nerfart_wgrad_operand_embed_pair(zp, zp, 1, 64, 11, o0, st), lambda: lib.nerfart_wgrad_operand_embed_pair(None, zp, 1, 64, 6, o0, st),
                                     lambda: lib.nerfart_wgrad_operand_embed_pair(zp, None, 1, 64, 6, o0, st), lambda: lib.nerfart_wgrad_operand_embed_pair(zp, zp, 1, 64, 6, None, st)],
        "wgrad_operand_inputs": [lambda: lib.nerfart_wgrad_operand_inputs(zp, -1, zp, -1, zp, 10, 8, o0, st), lambda: lib.nerfart_wgrad_operand_inputs(zp, -1, zp, -1, zp, 1, big, o0, st),
                                 lambda: lib.nerfart_wgrad_operand_inputs(zp, 10, zp, -1, zp, 1, 64, o0, st),           # 63 + 3 + 3 = 69 columns
                                 lambda: lib.nerfart_wgrad_operand_inputs(None, -1, zp, -1, zp, 1, 64, o0, st), lambda: lib.nerfart_wgrad_operand_inputs(zp, -1, None, -1, zp, 1, 64, o0, st),
                                 lambda: lib.nerfart_wgrad_operand_inputs(zp, -1, zp, -1, None, 1, 64, o0, st), lambda: lib.nerfart_wgrad_operand_inputs(zp, -1, zp, -1, zp, 1, 64, None, st)],
        "wgrad_operand_rgb_delta": [lambda: lib.nerfart_wgrad_operand_rgb_delta(zp, zp, 10, 8, o0, o1, o2, st), lambda: lib.nerfart_wgrad_operand_rgb_delta(zp, zp, 1, big, o0, o1, o2, st),
                                    lambda: lib.nerfart_wgrad_operand_rgb_delta(None, zp, 1, 64, o0, o1, o2, st), lambda: lib.nerfart_wgrad_operand_rgb_delta(zp, None, 1, 64, o0, o1, o2, st),
                                    lambda: lib.nerfart_wgrad_operand_rgb_delta(zp, zp, 1, 64, None, o1, o2, st), lambda: lib.nerfart_wgrad_operand_rgb_delta(zp, zp, 1, 64, o0, o1, None, st)],
        "wgrad_operand_sbar_ones": [lambda: lib.nerfart_wgrad_operand_sbar_ones(zp, 10, 8, o0, st), lambda: lib.nerfart_wgrad_operand_sbar_ones(zp, 1, big, o0, st),
                                    lambda: lib.nerfart_wgrad_operand_sbar_ones(None, 1, 64, o0, st), lambda: lib.nerfart_wgrad_operand_sbar_ones(zp, 1, 64, None, st)],
        "ray_points": [lambda: lib.nerfart_ray_points(zp, zp, zp, 1 << 20, 1 << 11, o0, o1, st), lambda: lib.nerfart_ray_points(None, zp, zp, 1, 1, o0, o1, st),
                       lambda: lib.nerfart_ray_points(zp, None, zp, 1, 1, o0, o1, st), lambda: lib.nerfart_ray_points(zp, zp, None, 1, 1, o0, o1, st),
                       lambda: lib.nerfart_ray_points(zp, zp, zp, 1, 1, None, o1, st)],
        "pass2_cotangents": [lambda: lib.nerfart_volsdf_pass2_cotangents(zp, zp, zp, zp, zp, zp, 1 << 20, 1 << 11, 3.0, 0.1, 0, o0, o1, o2, st)]
        + [(lambda a: (lambda: lib.nerfart_volsdf_pass2_cotangents(a[0], a[1], a[2], a[3], zp, zp, 1, 1, 3.0, 0.1, 0, a[4], a[5], a[6], st)))(
            [None if i == k else v for i, v in enumerate((zp, zp, zp, zp, o0, o1, o2))]) for k in range(7)],
    }
    for who, cs in calls.items():
        for i, call in enumerate(cs):
            prime = lib.nerfart_ray_points(None, zp, zp, 1, 1, o0, o1, st) if who != "ray_points" else lib.nerfart_wgrad_operand_sbar_ones(zp, 10, 8, o0, st)
            assert prime != 0 and who not in lib.nerfart_last_error().decode()      # another entry point's refusal in between: the message below is this call's
            rc = call()
            assert rc != 0, f"{who} refusal {i}: accepted"
            assert who in lib.nerfart_last_error().decode(), (who, i, lib.nerfart_last_error().decode())
    torch.cuda.synchronize()
    assert all(b.untouched() for b in o), "a refused call wrote to an output"
