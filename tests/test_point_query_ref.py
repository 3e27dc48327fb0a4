"""CPU checks of tests/point_query_ref.py: the trained-like states meet their conditions, the fp64 references equal torch's fp64 autograd of a plain
nn.functional model, the comparator accepts every tier's stand-in summed in another order and rejects every mutant at every tier, and the seeded
scene_state() cannot see the hidden-bias mutants at all (the blind spot the new state exists for)."""
import functools
import math

import pytest
import torch
import torch.nn.functional as F

import point_query_ref as Q

N = 400           # rows of the point set the CPU cases use: the edge rows (origin, clamp ties, largest |x|) and 4 ragged 16-point groups past 256


@functools.lru_cache(maxsize=None)
def _state(fw, name):
    """name 'A': the trained-like state; 'B': the one with BIG_BIAS_LAYER's biases at 0.2 (the fp16 tiers'); 'scene': the seeded scene_state()."""
    if name == "scene":
        sd = Q._base_state(fw)
    else:
        sd = Q.trained_like_state(fw, 0, Q.BIG_BIAS_LAYER if name == "B" else None)
    nets = Q.Nets(sd)
    pts, view = Q.case_points(nets, fw, N)
    return sd, nets, pts, view, {}


def state_of_tier(tier):
    return "B" if tier.startswith("fp16") else "A"


@functools.lru_cache(maxsize=None)
def _case(kind, fw, precision, R_bg, name):
    sd, nets, pts, view, share = _state(fw, name)
    c = Q.make_case(kind, fw, precision, nets, pts, view, R_bg=R_bg, sd=sd, share=share.setdefault("ref", {}))
    Q.allowances(c)
    return c


@pytest.mark.parametrize("fw,name", [("VolSDF", "A"), ("VolSDF", "B"), ("NeuS", "A")])
def test_state_conditions(fw, name):
    sd = _state(fw, name)[0]
    bad, fig = Q.check_state(sd, fw)
    print(f"\n{fw} state {name}: " + "  ".join(f"{k} {v:.4g}" for k, v in fig.items()))
    assert not bad, bad
    base = Q._base_state(fw)
    assert set(sd) == set(base) and all(sd[k].shape == base[k].shape and sd[k].dtype == base[k].dtype for k in sd)
    again = Q.trained_like_state(fw, 0, Q.BIG_BIAS_LAYER if name == "B" else None)
    assert all(torch.equal(sd[k], again[k]) for k in sd), "the state is a function of (framework, seed) alone"


def test_case_points_hold_the_edge_rows():
    sd, nets, pts, _, _ = _state("VolSDF", "A")
    assert bool((pts[0] == 0).all())
    r = Q.ref_surface(nets, pts)
    gap = ((3.0 - pts.double().norm(dim=-1)) - r["raw"]).abs()
    A32 = _case("sdf", "VolSDF", 0, 3.0, "A")["A"]["sdf"]
    assert float(gap[1: 1 + Q.N_TIES].max()) < A32, "rows on the tie of the clamp: closer than the smallest allowance of any tier"
    assert abs(32.0 * float(pts[1 + Q.N_TIES].abs().max()) - 170.0) < 1.0
    out = pts.norm(dim=-1) > 3.0
    assert int(out.sum()) >= 20 and bool(((3.0 - pts.double().norm(dim=-1)) < r["raw"])[out].any()), "points where the clamp goes negative"
    assert bool(((3.0 - pts.double().norm(dim=-1)) < r["raw"]).any()) and bool(((3.0 - pts.double().norm(dim=-1)) > r["raw"]).any())


# ---- the references against a plain nn.functional model under fp64 autograd ---------------------------------------------------------------------
def _plain_model(sd, x, view, multires_view):
    fold = lambda stem, l: sd[f"{stem}.{l}.weight_g"].double() * sd[f"{stem}.{l}.weight_v"].double() / sd[f"{stem}.{l}.weight_v"].double().norm(dim=1, keepdim=True)
    emb = lambda t, L: torch.cat([t] + [fn(t * 2.0 ** k) for k in range(L) for fn in (torch.sin, torch.cos)], -1)
    x = x.double().requires_grad_(True)
    e = emb(x, 6)
    h = e
    for l in range(8):
        if l == 4:
            h = torch.cat([h, e], -1) / math.sqrt(2.0)
        h = F.softplus(F.linear(h, fold(Q.S, l), sd[f"{Q.S}.{l}.bias"].double()), beta=100.0, threshold=1e9)
    out = F.linear(h, fold(Q.S, 8), sd[f"{Q.S}.8.bias"].double())
    sdf, feat = out[:, 0], out[:, 1:]
    nabla = torch.autograd.grad(sdf.sum(), x)[0]
    v = view.double()
    r = torch.cat([x, v if multires_view < 0 else emb(v, multires_view), nabla, feat], -1)
    for l in range(5):
        r = F.linear(r, fold(Q.R, l), sd[f"{Q.R}.{l}.bias"].double())
        r = torch.sigmoid(r) if l == 4 else torch.relu(r)
    return sdf.detach(), nabla, h.detach(), r.detach()


@pytest.mark.parametrize("fw", ["VolSDF", "NeuS"])
def test_references_equal_fp64_autograd(fw):
    sd, nets, pts, view, _ = _state(fw, "A")
    sdf, nabla, h7, rgb = _plain_model(sd, pts, view, nets.multires_view)
    Rb = 3.0 if fw == "VolSDF" else 1.0
    ref = Q.ref_surface(nets, pts, Rb)
    assert float((ref["raw"] - sdf).abs().max()) < 1e-12 and float((ref["nabla"] - nabla).abs().max()) < 1e-12
    assert float((ref["h7"] - h7).abs().max()) < 1e-12
    assert torch.equal(ref["sdf"], torch.minimum(ref["raw"], Rb - pts.double().norm(dim=-1))) and not torch.equal(ref["sdf"], ref["raw"])
    assert torch.equal(Q.ref_surface(nets, pts, 0.0)["sdf"], ref["raw"]) and torch.equal(Q.ref_surface(nets, pts, -1.0)["sdf"], ref["raw"])
    assert torch.equal(Q.ref_surface(nets, pts, 0.0)["nabla"], ref["nabla"]), "the clamp never replaces nabla"
    got = Q.ref_radiance(nets, pts.double(), view.double(), ref["nabla"], ref["h7"])
    assert float((got - rgb).abs().max()) < 1e-12


def test_nets_keep_both_folds_when_moved():
    sd, nets, pts, _, _ = _state("VolSDF", "A")
    moved = nets.to("cpu")
    assert type(moved) is Q.Nets and moved.kernel_view().W[3] is moved.Wf[3] and torch.equal(moved.W[3], nets.W[3])
    assert not torch.equal(nets.W[3], nets.Wf[3]) and float((nets.W[3] - nets.Wf[3]).abs().max()) < 1e-7, "fp64 fold for the references, fp32 fold for the stand-ins"


def test_ray_points():
    g = torch.Generator().manual_seed(1)
    o, d, depth = torch.randn(7, 3, generator=g), torch.randn(7, 3, generator=g), torch.rand(4, 8, generator=g)
    idx = torch.tensor([5, 0, 6, 2], dtype=torch.int32)
    x, v = Q.ray_points(o, d, idx, depth, 5)
    assert x.shape == (20, 3) and v.shape == (20, 3)
    for s in range(4):
        for k in range(5):
            assert torch.equal(x[5 * s + k], o[idx[s]].double() + d[idx[s]].double() * depth[s, k].double()) and torch.equal(v[5 * s + k], d[idx[s]].double())
    x32, _ = Q.ray_points(o, d, idx, depth, 5, torch.float32)
    assert torch.equal(x32[7], o[0] + d[0] * depth[1, 2])


# ---- the comparator accepts every stand-in and rejects every mutant -------------------------------------------------------------------------------
CASES = [("sdf", p) for p in Q.SDF_PRECISIONS] + [("nabla", p) for p in Q.NABLA_PRECISIONS] + [("rad", p) for p in Q.RAD_PRECISIONS]


def _setups(kind, precision):
    """The cases of one entry point and precision: VolSDF with and without the sphere clamp, NeuS (its radiance net embeds the view direction)."""
    name = state_of_tier(Q.PRECISION[precision][0])
    s = [_case(kind, "VolSDF", precision, 3.0, name)]
    if kind != "rad":
        s.append(_case(kind, "VolSDF", precision, 0.0, name))
    else:
        s.append(_case(kind, "NeuS", precision, 0.0, "A"))
    return s


@pytest.mark.parametrize("kind,precision", CASES)
def test_standin_summed_in_another_order_is_accepted(kind, precision):
    for c in _setups(kind, precision):
        for seed in (1, 2):
            out = Q.standin(c, kperm=seed)
            assert any(not torch.equal(out[k], Q.standin(c)[k]) for k in out), "the permutation of k changed nothing: no other summation order was tried"
            viol, ratio = Q.check(c, out)
            print(f"\n{c['id']} (k permuted, seed {seed}): {Q.fmt(ratio)}")
            assert not viol, viol
            assert max(ratio.values()) < 0.6, "another order moves the stand-in's error by a small part of A"
        viol, ratio = Q.check(c, Q.reference(c))
        assert not viol and max(ratio.values()) == 0.0


def _applies(mut, c):
    if mut in ("view_band_order", "feat_bias_row"):
        return c["kind"] == "rad" and (mut == "feat_bias_row" or c["nets"].view_tiles == 3)
    if c["kind"] == "rad":
        return mut == "tile_shift"
    if mut in ("tangent_bias", "clamp_nabla", "h7_unit_order") and c["kind"] != "nabla":
        return False
    if mut == "clamp_nabla":
        return c["R_bg"] > 0
    if mut == "clamp_no_radius":
        return c["R_bg"] <= 0
    return True


@pytest.mark.parametrize("kind,precision", CASES)
@pytest.mark.parametrize("mut", Q.MUTANTS)
def test_mutant_is_rejected(mut, kind, precision):
    cases = [c for c in _setups(kind, precision) if _applies(mut, c)]
    if not cases:
        assert not any(_applies(mut, c) for c in _setups(kind, precision))
        return                      # the entry point has no output this mutant touches (fp16x1: sdf only; the radiance net has no bias of the SDF net ...)
    for c in cases:
        out = Q.standin(c, mut)
        viol, ratio = Q.check(c, out)
        touched = [k for k in Q.TOUCHES.get(mut, ("sdf", "nabla", "h7")) if k in ratio]
        print(f"\n{c['id']} {mut}: {Q.fmt(ratio)}")
        assert touched and viol, f"{mut} passes at {c['id']}: {ratio}"
        assert all(ratio[k] > 1.0 for k in touched), f"{mut} at {c['id']}: an output it touches stays within A: {ratio}"


@pytest.mark.parametrize("mut", Q.WEIGHT_MUTANTS)
def test_mutated_state_is_the_mutated_net(mut):
    """mutate_state (what the GPU test packs a blob from, to see the real kernels' outputs rejected) is the fault mutate_nets injects into the stand-in."""
    sd, nets, _, _, _ = _state("VolSDF", "A")
    a, b = Q.Nets(Q.mutate_state(sd, mut)), Q.mutate_nets(nets, sd, mut)
    for x, y in zip(a.W + a.b + a.R + a.rb, b.W + b.b + b.R + b.rb):
        assert float((x - y).abs().max()) < 1e-6 * max(1.0, float(y.abs().max()))     # the state dict is fp32: g |v'| / |v| rounds once more
    assert any(not torch.equal(x, y) for x, y in zip(a.W + a.b, nets.W + nets.b))


def test_every_mutant_is_rejected_at_every_tier_that_has_its_output():
    """The matrix of the test above, stated once: which (mutant, entry point, precision) pairs it holds."""
    held = {(m, k, p) for m in Q.MUTANTS for k, p in CASES if any(_applies(m, c) for c in _setups(k, p))}
    for m in Q.MUTANTS:
        tiers = {Q.PRECISION[p][0] for (mm, k, p) in held if mm == m}
        want = set(Q.TIERS) if "sdf" in Q.TOUCHES.get(m, ("sdf",)) else {"fp32", "bf16x3", "fp16x2"}
        assert tiers == want, (m, tiers)


# ---- the blind spot of the seeded scene state --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", Q.NABLA_PRECISIONS)
def test_scene_state_cannot_see_the_hidden_bias_mutants(precision):
    """On scene_state() every hidden bias is exactly 0: rolling them, or exchanging two, changes no output by a single bit, and the same comparator
    with the same allowance rule accepts both mutants there.  On the trained-like state it rejects them (test_mutant_is_rejected)."""
    sd = Q._base_state("VolSDF")
    assert all(bool((sd[f"{Q.S}.{l}.bias"] == 0).all()) for l in range(8))
    c = _case("nabla", "VolSDF", precision, 3.0, "scene")
    clean = Q.standin(c)
    for mut in ("bias_roll", "bias_swap"):
        out = Q.standin(c, mut)
        assert all(torch.equal(out[k], clean[k]) for k in out), f"{mut}: effect on the seeded scene state is not exactly 0"
        viol, ratio = Q.check(c, out)
        assert not viol and abs(max(ratio.values()) - 1.0 / Q.FACTOR) < 1e-12
    mnets = Q.mutate_nets(c["nets"], c["sd"], "bias_roll")
    ref, mref = Q.ref_surface(c["nets"], c["x64"]), Q.ref_surface(mnets, c["x64"])
    assert all(torch.equal(ref[k], mref[k]) for k in ref), "the fp64 reference itself does not move"
