"""The per-sample backward entry points - nerfart_sdf_fwd2 -> nerfart_sdf_bwd2 and nerfart_radiance_fwd_dump -> nerfart_radiance_bwd - against the
fp64 references and the allowances of tests/mlp_bwd_ref.py, on the case matrix tests/test_mlp_bwd_ref.py runs the stand-in and its mutants through
on the CPU.  Called through hip.lib and ctypes with local helpers: every dump and output buffer is the test's own, pre-filled with 0xFF bytes (NaN as
bf16 and as fp32) and followed by a guard tail that must come back untouched.  Each pair runs twice on the same inputs and must give the same bits.
One line per case: the worst observed / allowed ratio per output (1.00 = the allowance).

Worst observed / allowed ratio per output over the whole matrix on an MI355X (gfx950; every case passed, every exact check - padded rows, zero
cotangents, the fill of the never-written rows, guard tails, two runs - held bit for bit).  A bf16 element rounded to nearest lies up to half an
ulp from the reference by itself, which is the first term of its allowance: the dump ratios sit just under 1.00 by construction, and what
they bound is the arithmetic error on top (A, FACTOR = 4 times the stand-in's).  The fp32 outputs, the softplus' slots and the aggregates carry no
such term: there 0.25 is the stand-in's own error.
  nerfart_sdf_fwd2           a_l 0.99  adot_l 0.97  softplus' 0.59  mean of softplus' 0.72
  nerfart_sdf_bwd2           zbar_l 1.00  t_l d_l 1.00
  surf_param_bwd's products  dW_1..7 0.26  db 0.26  dW_0 / dW_4 encoding columns 0.25  the sdf row of the last layer 0.28
  nerfart_radiance_fwd_dump  f 1.00  r_l 0.99  rgb 0.45 (nerfart_radiance_fwd: 0.45, the same bits in every case)  ReLU signs outside the allowance 0
  nerfart_radiance_bwd       delta_l 1.00  g_f 0.98  g_h7 0.36  g_n 0.30
  rad_param_bwd's products   W8[1:] rows 0.26 (bias 0.29)  dR_0..3 0.26  db 0.26  [x | v | n] columns 0.25
"""
import functools

import pytest
import torch

import mlp_bwd_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
GUARD = 4096


@functools.lru_cache(maxsize=None)
def _scene(fw):
    """(surf_blob, rad_blob, view_tiles, reference weights on the CPU, the same on the device)."""
    from nerfart_amd import scene
    model, _, _ = scene.build_model(fw, seed=0, beta=0.01 if fw == "VolSDF" else None, device=DEV, precision="bf16x3")
    surf_blob, rad_blob = model.packed()
    nets = R.Nets({k: v.detach().cpu() for k, v in model.state_dict().items()})
    assert nets.view_tiles == model.view_tiles
    return surf_blob, rad_blob, model.view_tiles, nets, nets.to(DEV)


def _buf(nbytes):
    return torch.full((nbytes + GUARD,), R.FILL, dtype=torch.uint8, device=DEV)


def _f32(buf, *shape):
    n = 4
    for s in shape:
        n *= s
    return buf[:n].view(torch.float32).view(*shape)


def _guards_ok(bufs, sizes):
    return [k for k, b in bufs.items() if bool((b[sizes[k]:] != R.FILL).any())]


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _rc(lib, rc, who):
    assert rc == 0, (who, rc, lib.nerfart_last_error().decode())


def _run_sdf(c, surf_blob):
    from nerfart_amd import hip
    lib, M = hip.lib, c["M"]
    inp = {k: c[k].to(DEV).contiguous() for k in ("pts", "dir", "gbar_h7", "gbar_sdf")}
    sizes = dict(f2=int(lib.nerfart_sdf_fwd2_dump_bytes(M)), r2=int(lib.nerfart_sdf_bwd2_dump_bytes(M)))
    assert sizes == dict(f2=R.f2_bytes(M), r2=R.r2_bytes(M))
    bufs = {k: _buf(n) for k, n in sizes.items()}
    _rc(lib, lib.nerfart_sdf_fwd2(surf_blob.data_ptr(), inp["pts"].data_ptr(), inp["dir"].data_ptr(), M, bufs["f2"].data_ptr(), _stream()), "sdf_fwd2")
    _rc(lib, lib.nerfart_sdf_bwd2(surf_blob.data_ptr(), M, inp["gbar_h7"].data_ptr(), inp["gbar_sdf"].data_ptr(), bufs["f2"].data_ptr(),
                                  bufs["r2"].data_ptr(), _stream()), "sdf_bwd2")
    torch.cuda.synchronize()
    return {k: bufs[k][: sizes[k]] for k in bufs}, _guards_ok(bufs, sizes)


def _run_rad(c, rad_blob, view_tiles):
    from nerfart_amd import hip
    lib, M = hip.lib, c["M"]
    inp = {k: c[k].to(DEV).contiguous() for k in ("pts", "view", "nabla", "h7", "g_rgb")}
    nd = int(lib.nerfart_radiance_dump_bytes(M))
    assert nd == R.rad_bytes(M)
    sizes = dict(rgb=M * 12, fdump=nd, bdump=nd, g_h7=M * 1024, g_n=M * 12, rgb_plain=M * 12)
    bufs = {k: _buf(n) for k, n in sizes.items()}
    _rc(lib, lib.nerfart_radiance_fwd_dump(rad_blob.data_ptr(), view_tiles, inp["pts"].data_ptr(), inp["view"].data_ptr(), M, inp["nabla"].data_ptr(),
                                           inp["h7"].data_ptr(), bufs["rgb"].data_ptr(), bufs["fdump"].data_ptr(), _stream()), "radiance_fwd_dump")
    _rc(lib, lib.nerfart_radiance_bwd(rad_blob.data_ptr(), M, bufs["rgb"].data_ptr(), inp["g_rgb"].data_ptr(), bufs["fdump"].data_ptr(),
                                      bufs["bdump"].data_ptr(), bufs["g_h7"].data_ptr(), bufs["g_n"].data_ptr(), _stream()), "radiance_bwd")
    _rc(lib, lib.nerfart_radiance_fwd(rad_blob.data_ptr(), 1, view_tiles, inp["pts"].data_ptr(), inp["view"].data_ptr(), M, inp["nabla"].data_ptr(),
                                      inp["h7"].data_ptr(), bufs["rgb_plain"].data_ptr(), _stream()), "radiance_fwd")
    torch.cuda.synchronize()
    out = dict(fdump=bufs["fdump"][:nd], bdump=bufs["bdump"][:nd], rgb=_f32(bufs["rgb"], M, 3), g_h7=_f32(bufs["g_h7"], M, 256),
               g_n=_f32(bufs["g_n"], M, 3), rgb_plain=_f32(bufs["rgb_plain"], M, 3))
    return out, _guards_ok(bufs, sizes)


@pytest.mark.parametrize("spec", R.specs(), ids=R.spec_id)
def test_backward_pair_matches_fp64(spec):
    kind, fw, M = spec
    surf_blob, rad_blob, view_tiles, nets_cpu, nets_dev = _scene(fw)
    wrap = M > 4096                                    # the two grid-wrapping cases: reference and stand-in in torch on the device
    c = R.make_case(spec, nets_dev if wrap else nets_cpu)
    run = (lambda: _run_sdf(c, surf_blob)) if kind == "sdf" else (lambda: _run_rad(c, rad_blob, view_tiles))
    out, bad_guards = run()
    again, _ = run()
    assert not bad_guards, f"{c['id']}: written past the end of {bad_guards}"
    for k in out:
        assert torch.equal(out[k].view(torch.uint8), again[k].view(torch.uint8)), f"{c['id']}: {k} differs between two runs on the same inputs"
    viol, worst = R.check(c, out)
    extra = ""
    if kind == "rad":
        extra = f"  max |rgb(fwd_dump) - rgb(fwd)| = {float((out['rgb'] - out['rgb_plain']).abs().max()):.2e}"
    print(f"\n{c['id']}: " + "  ".join(f"{k} {v:.2f}" for k, v in worst.items()) + extra)
    assert not viol, "\n".join(viol[:20])
