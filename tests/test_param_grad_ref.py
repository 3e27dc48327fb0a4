"""tests/param_grad_ref.py on the CPU: the fp64 parameter-gradient model against plain fp64 autograd (weight_norm, double backward, ReLU signs its
own), the fold model's input, and the comparator - it accepts a model of the library route (the stand-in's dumps of tests/mlp_bwd_ref.py, fp32
products in another summation order, the fold in float32, the chain rule in float32) on every size tests/test_gpu_param_grads.py runs on the GPU,
and rejects every mutant of that route by name, each at the smallest size at which it can show (EXPECT)."""
import math

import numpy as np
import pytest
import torch

import mlp_bwd_ref as R
import param_grad_ref as G
from conftest import scene_state

F32, F64 = torch.float32, torch.float64


@pytest.fixture(scope="module")
def states():
    return {fw: scene_state(fw, 0.01 if fw == "VolSDF" else None)[0] for fw in ("VolSDF", "NeuS")}


@pytest.fixture(scope="module")
def nets(states):
    return {fw: R.Nets(sd) for fw, sd in states.items()}


def _rel(a, b):
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-300))


# ---- the route model -----------------------------------------------------------------------------------------------------------------
def wn32(dW, v, g):
    return tuple(torch.as_tensor(np.asarray(t, dtype=np.float64)) for t in G.wn_bwd32_pairwise(dW.numpy(), v.numpy(), g.numpy()))


def model_raw(case, mut=None, **kw):
    """Stand-in dumps -> operands -> the sections one call adds, reduced in fp32 (torch's blocked matmul: another order than any fp64 sum)."""
    dumps = R.run_standin(case)
    op = G.standin_operands(case, dumps)
    return dumps, op, G.assemble(G.reduce_sections(op, dtype=F32, mut=mut, **kw), dtype=F32)


def model_grads(raw32, sd, case, fold_mut=None, no_projection=False):
    mv = case["nets"].multires_view
    fold = lambda r: G.fold_model(r, 6, mv, fold_mut)
    wn = (lambda dW, v, g: G.wn_bwd64(dW, v, g, no_projection=True)) if no_projection else wn32
    return G.grads_from_raw(raw32, sd, case["kind"], mv, fold=fold, wn=wn)


def part1(case, op, raw32, extra=0, op_all=None):
    rep = G.new_report(case["id"])
    ref_op = op_all or op
    worst = G.check_raw(rep, raw32, G.reduce_sections(ref_op), G.reduce_sections(ref_op, absolute=True), G.additions(case["kind"], case["M"]), extra)
    return rep.viol, worst


def part4(case, sd, dumps, got):
    rep = G.new_report(case["id"])
    masks = G.dump_masks(dumps["fdump"], case["M"]) if case["kind"] == "rad" else None
    ref = G.ref_param_grads(sd, case, masks)
    sim, acc = G.sim_param_grads(sd, case)
    worst = G.check_param_grads(rep, got, ref, sim, acc)
    return rep.viol, worst, ref, sim


# ---- the references against plain autograd -------------------------------------------------------------------------------------------
def _plain_leaves(sd):
    return {k: v.detach().double().clone().requires_grad_(True) for k, v in sd.items() if k.startswith((G.S_STEM, G.R_STEM))}


def _plain_W(p, stem, l):
    return torch._weight_norm(p[f"{stem}.{l}.weight_v"], p[f"{stem}.{l}.weight_g"], 0)


@pytest.mark.parametrize("fw", ["VolSDF", "NeuS"])
def test_sdf_model_matches_the_fp64_double_backward(states, nets, fw):
    sd = states[fw]
    c = R.make_case(("sdf", fw, 37), nets[fw])
    p = _plain_leaves(sd)
    x = c["pts"].double().requires_grad_(True)
    e, _ = R.embed_pair(x, torch.zeros_like(x))
    h = e
    for l in range(8):
        if l == 4:
            h = torch.cat([h, e], -1) / math.sqrt(2.0)
        h = R.softplus100(h @ _plain_W(p, G.S_STEM, l).T + p[f"{G.S_STEM}.{l}.bias"])
    sdf = h @ _plain_W(p, G.S_STEM, 8)[0] + p[f"{G.S_STEM}.8.bias"][0]
    nabla = torch.autograd.grad(sdf.sum(), x, create_graph=True)[0]
    phi = (c["gbar_sdf"].double() * sdf).sum() + (c["gbar_h7"].double() * h).sum() + (c["dir"].double() * nabla).sum()
    phi.backward()
    got = G.ref_param_grads(sd, c)
    assert len(got) == 27
    for name, stem, l in G.param_names("sdf"):
        for k in ("weight_g", "weight_v", "bias"):
            assert _rel(got[f"{name}.{k}"], p[f"{stem}.{l}.{k}"].grad) < 1e-10, (name, k)
    assert bool((got["sdf.8.weight_v"][1:] == 0).all()) and bool((got["sdf.8.bias"][1:] == 0).all())


@pytest.mark.parametrize("fw", ["VolSDF", "NeuS"])
def test_radiance_model_matches_fp64_autograd(states, nets, fw):
    from oracle import nets as onets
    sd, n = states[fw], nets[fw]
    c = R.make_case(("rad", fw, 41), n)
    p = _plain_leaves(sd)
    f = c["h7"].double() @ _plain_W(p, G.S_STEM, 8)[1:].T + p[f"{G.S_STEM}.8.bias"][1:]
    h = torch.cat([c["pts"].double(), onets.embed(c["view"].double(), n.multires_view), c["nabla"].double(), f], -1)
    masks = []
    for l in range(4):
        z = h @ _plain_W(p, G.R_STEM, l).T + p[f"{G.R_STEM}.{l}.bias"]
        masks.append(z.detach() > 0)
        h = torch.relu(z)
    rgb = torch.sigmoid(h @ _plain_W(p, G.R_STEM, 4).T + p[f"{G.R_STEM}.4.bias"])
    (rgb * c["g_rgb"].double()).sum().backward()
    got = G.ref_param_grads(sd, c, masks)
    assert len(got) == 18
    for name, stem, l in G.param_names("rad"):
        for k in ("weight_g", "weight_v", "bias"):
            assert _rel(got[f"{name}.{k}"], p[f"{stem}.{l}.{k}"].grad) < 1e-10, (name, k)
    assert bool((got["sdf.8.weight_v"][0] == 0).all()) and float(got["sdf.8.weight_g"][0]) == 0.0 and float(got["sdf.8.bias"][0]) == 0.0


def test_weight_norm_reference_matches_autograd():
    g_ = torch.Generator().manual_seed(0)
    for out_f, in_f in ((5, 39), (1, 1), (2, 65)):
        v = torch.randn(out_f, in_f, generator=g_, dtype=F64).requires_grad_(True)
        g = (torch.rand(out_f, 1, generator=g_, dtype=F64) + 0.5).requires_grad_(True)
        dW = torch.randn(out_f, in_f, generator=g_, dtype=F64)
        torch._weight_norm(v, g, 0).backward(dW)
        g_g, g_v = G.wn_bwd64(dW, v.detach(), g.detach())
        scale = float((g.detach() / v.detach().norm(dim=1, keepdim=True) * dW.abs()).max())       # (1, 1): g_v is pure cancellation, exactly 0 here
        assert _rel(g_g, g.grad.reshape(-1)) < 1e-13 and float((g_v - v.grad).abs().max()) < 1e-13 * scale
        p_g, p_v = G.wn_bwd32_pairwise(dW.numpy(), v.detach().numpy(), g.detach().numpy())
        assert p_g.dtype == np.float32 and float((torch.as_tensor(p_v).double() - v.grad).abs().max()) < 1e-5 * scale
        e_g, e_v = G.wn_abs(torch.ones_like(dW) * 1e-6, v.detach(), g.detach())
        d_g, d_v = G.wn_bwd64(dW + 1e-6 * torch.sign(v.detach()), v.detach(), g.detach())
        assert bool(((d_g - g_g).abs() <= e_g * (1 + 1e-9)).all()) and bool(((d_v - g_v).abs() <= e_v * (1 + 1e-9)).all())


# ---- layouts and the fold's test input -----------------------------------------------------------------------------------------------
def test_layouts_and_the_distinct_raw_buffer():
    offs, total = G.raw_offsets()
    assert total == 7 * 65536 + 2 * 16384 + 512 + 1792 + 16384 + 4 + 4 * 65536 + 1280 + 16384 + 4 + 16384 + 65536 + 4
    assert all(o % 4 == 0 for o in offs.values())
    raw = np.arange(total, dtype=np.float32) * np.float32(1e-3) + np.float32(1.0)
    assert np.unique(raw).size == total                      # arange * 1e-3 + 1 stays distinct in fp32 over the whole buffer
    for mv, nex in ((-1, 9), (4, 33)):
        lay = G.folded_layout(6, mv)
        assert len(lay) == 28 and lay[0][1] == (256, 39) and lay[6][1] == (217, 256) and lay[16][1] == (257, 256) and lay[18][1] == (256, nex + 256)
        assert G.folded_offsets(6, mv)[-1] == sum(G.numel(s) for _, s in lay)
        pieces = G.fold_model(raw, 6, mv)
        unread = G.fold_unread(6, mv)
        # every raw slot is read at most once, the unread ones never: a folded value identifies its slot(s)
        poisoned = raw.copy()
        poisoned[unread] = np.nan
        again = G.fold_model(poisoned, 6, mv)
        for k in pieces:
            assert pieces[k].dtype == np.float32 and np.array_equal(pieces[k], again[k]), k
        # ... and every other slot IS read: NaN there reaches some piece
        read = np.zeros(total, dtype=bool)
        for name in G.SECTIONS[:12]:
            for probe in (0, G.numel(G.SHAPES[name]) // 2 + 1, G.numel(G.SHAPES[name]) - 1):
                i = offs[name] + probe
                if unread[i]:
                    continue
                t = raw.copy()
                t[i] = np.nan
                assert any(np.isnan(v).any() for v in G.fold_model(t, 6, mv).values()), (name, probe)
                read[i] = True
        assert read.any()


def test_narrow_operand_model_and_unit_order():
    x = torch.tensor([[1.0 + 2.0 ** -9, -3.0, 0.1]])
    v = G.units(G.narrow_bytes(x, 2), 2, 64)
    assert v[0, 0] == 1.0 and v[0, 32] == 2.0 ** -9 and v[0, 1] == -3.0 and v[0, 33] == 0.0 and bool((v[1] == 0).all()) and bool((v[0, 3:32] == 0).all())
    assert abs(float(v[0, 2] + v[0, 34]) - float(torch.tensor(0.1))) < 2.0 ** -18
    wide = G.units(G.narrow_bytes(torch.ones(1, 33), 1), 1, 64)
    assert bool((wide[0, :33] == 1).all()) and bool((wide[0, 33:] == 0).all())       # 33 columns: no lo half
    h7 = torch.arange(256, dtype=F32)[None] + 0.0
    a7 = G.units(G.a7_bytes(h7, 1), 64, 256)
    assert torch.equal(a7[0], R.PERM.double()) and bool((a7[1:] == 0).all())


# ---- the comparator accepts the route model -------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def cases(nets):
    return {R.spec_id(s): R.make_case(s, nets[s[1]]) for s in G.specs()}


@pytest.mark.parametrize("cid", [R.spec_id(s) for s in G.specs()])
def test_the_route_model_passes(states, cases, cid):
    c = cases[cid]
    sd = states[c["fw"]]
    dumps, op, raw32 = model_raw(c)
    viol, w1 = part1(c, op, raw32)
    assert not viol, "\n".join(viol[:20])
    viol, w4, ref, sim = part4(c, sd, dumps, model_grads(raw32, sd, c))
    print(f"\n{cid}: part 1 " + "  ".join(f"{k} {v:.3f}" for k, v in w1.items()) + "\n   part 4 " + "  ".join(f"{k} {v:.3f}" for k, v in w4.items()))
    assert not viol, "\n".join(viol[:20])
    # the stand-in route is a route to the right gradients at all (fold model, section layout, chain rule): a few bf16 ulps from fp64 autograd
    for k, r in ref.items():
        if float(r.norm()) > 0:
            assert float((sim[k].reshape(r.shape) - r).norm() / r.norm()) < 2e-2, k


def test_train_radiance_0_reduces_two_sections_only(cases):
    c = cases["rad-VolSDF-129"]
    op = G.standin_operands(c, R.run_standin(c))
    on, off = G.reduce_sections(op), G.reduce_sections(op, train_radiance=False)
    assert set(off) == {"RAD_WH7", "RAD_CS"} and torch.equal(off["RAD_WH7"], on["RAD_WH7"]) and torch.equal(off["RAD_CS"][4], on["RAD_CS"][4])
    assert bool((off["RAD_CS"][:4] == 0).all())
    # row 4 of RAD_CS is summed over up(M, 64) rows, rows 0..3 over up(M, 128): its allowance counts its own rows
    assert G.additions("rad", 1)["RAD_CS"].reshape(-1).tolist() == [129.0] * 4 + [65.0] and G.additions("rad", 1)["RAD_WH7"] == 65
    assert G.additions("rad", 520)["RAD_CS"].reshape(-1).tolist() == [642.0] * 4 + [578.0]


# ---- the comparator rejects the mutants ------------------------------------------------------------------------------------------------
EXPECT = {          # mutant -> (part that rejects it, the smallest case at which it can show, what the violation must name)
    "transposed": (1, "sdf-VolSDF-1", "raw.SURF_WW"),                  # one point: an outer product z a^T is not symmetric
    "act_same_layer": (1, "sdf-VolSDF-1", "raw.SURF_WW"),
    "no_tangent_rows": (1, "sdf-VolSDF-1", "raw.SURF_WW"),             # point 0 has a non-zero direction
    "cs_all_rows": (1, "sdf-VolSDF-1", "raw.SURF_CS17"),
    "ragged_row_dropped": (1, "sdf-VolSDF-1", "raw.SURF_WW"),          # any M that is no multiple of 64; it cannot show at M = 64 (below)
    "narrow_lo_dropped": (1, "sdf-VolSDF-1", "raw.SURF_W8"),
    "w8_no_adot_sums": (1, "sdf-VolSDF-1", "raw.SURF_W8"),
    "no_65535": (2, None, "fold.sdf.0.dW"),                            # the fold has no size: a raw buffer with a distinct value per slot
    "no_rsqrt2_skip": (2, None, "fold.sdf.4.dW"),
    "skip_enc_from_we0": (2, None, "fold.sdf.4.dW"),
    "bias_neighbour_row": (2, None, "fold.sdf.5.db"),
    "unperm_one_axis": (2, None, "fold.sdf.1.dW"),
    "fold_lo_dropped": (2, None, "fold.rad.4.dW"),
    "wn_no_projection": (4, "sdf-VolSDF-1", "grad.sdf.1.weight_v"),
    "accumulate_overwrites": (1, "sdf-VolSDF-2", "raw.SURF_WW"),       # two points: one per call
}


def test_every_mutant_is_listed():
    assert set(EXPECT) == set(G.REDUCE_MUTANTS) | set(G.FOLD_MUTANTS) | {"wn_no_projection", "accumulate_overwrites"}


def _case(nets, cid):
    kind, fw, M = cid.split("-")
    return R.make_case((kind, fw, int(M)), nets[fw])


@pytest.mark.parametrize("mut", G.REDUCE_MUTANTS)
def test_part_1_rejects_the_reduction_mutant(nets, mut):
    _, cid, name = EXPECT[mut]
    c = _case(nets, cid)
    _, op, raw32 = model_raw(c, mut)
    viol, _ = part1(c, op, raw32)
    hits = [v for v in viol if f" {name}" in v]
    assert hits, f"check_raw accepted '{mut}' at {cid} (it must name {name}): {viol[:3]}"
    print(f"\n{mut}: {hits[0][:200]}")


def test_the_ragged_row_mutant_shows_at_65_and_cannot_at_64(nets):
    c = _case(nets, "sdf-VolSDF-65")
    _, op, raw32 = model_raw(c, "ragged_row_dropped")
    assert any(" raw.SURF_WW" in v for v in part1(c, op, raw32)[0])
    c = _case(nets, "sdf-VolSDF-64")
    _, op, a = model_raw(c, "ragged_row_dropped")
    _, _, b = model_raw(c)
    assert torch.equal(a, b) and not part1(c, op, a)[0]
    c = _case(nets, "rad-VolSDF-129")
    _, op, raw32 = model_raw(c, "ragged_row_dropped")
    assert any(" raw.RAD_W" in v for v in part1(c, op, raw32)[0])


def _halves(c):
    """The case split into two calls over disjoint halves of its points."""
    h = c["M"] // 2
    out = []
    for sl in (slice(0, h), slice(h, c["M"])):
        d = dict(c)
        for k in ("pts", "dir", "gbar_sdf", "gbar_h7", "view", "nabla", "h7", "g_rgb"):
            if k in c:
                d[k] = c[k][sl].contiguous()
        d["M"] = d["pts"].shape[0]
        out.append(d)
    return out


@pytest.mark.parametrize("cid", ["sdf-VolSDF-2", "sdf-VolSDF-65", "rad-NeuS-129"])
def test_two_calls_accumulate_and_overwriting_is_rejected(nets, cid):
    c = _case(nets, cid)
    _, op_all, _ = model_raw(c)
    a, b = _halves(c)
    (_, _, ra), (_, _, rb) = model_raw(a), model_raw(b)
    n = {k: v + G.additions(c["kind"], b["M"])[k] for k, v in G.additions(c["kind"], a["M"]).items()}
    P, S = G.reduce_sections(op_all), G.reduce_sections(op_all, absolute=True)
    rep = G.new_report(cid)
    G.check_raw(rep, ra + rb, P, S, n, extra=1)
    assert not rep.viol, "\n".join(rep.viol[:10])
    rep = G.new_report(cid)
    G.check_raw(rep, rb, P, S, n, extra=1)                           # the second call overwrote the first
    assert any(" raw." in v for v in rep.viol)
    if cid == EXPECT["accumulate_overwrites"][1]:
        assert any(f" {EXPECT['accumulate_overwrites'][2]}" in v for v in rep.viol)


@pytest.mark.parametrize("mv", [-1, 4])
@pytest.mark.parametrize("mut", G.FOLD_MUTANTS)
def test_part_2_rejects_the_fold_mutant(mut, mv):
    _, total = G.raw_offsets()
    raw = np.arange(total, dtype=np.float32) * np.float32(1e-3) + np.float32(1.0)
    want = G.fold_model(raw, 6, mv)
    rep = G.new_report(f"fold({mv})")
    assert G.check_fold(rep, G.fold_model(raw, 6, mv), want) == 0 and not rep.viol
    G.check_fold(rep, G.fold_model(raw, 6, mv, mut), want)
    name = EXPECT[mut][2]
    assert any(f" {name}" in v for v in rep.viol), f"check_fold accepted '{mut}' (it must name {name}): {rep.viol[:3]}"
    one = {k: v.copy() for k, v in want.items()}
    one["rad.2.dW"][5, 7] = np.nextafter(one["rad.2.dW"][5, 7], np.float32(np.inf))
    rep = G.new_report("1 ulp")
    assert G.check_fold(rep, one, want) == 1 and not rep.viol
    one["rad.2.dW"][5, 7] = np.nextafter(one["rad.2.dW"][5, 7], np.float32(np.inf))
    assert G.check_fold(rep, one, want) == 2 and any(" fold.rad.2.dW" in v for v in rep.viol)


def test_part_4_rejects_a_missing_projection_term(states, nets):
    _, cid, name = EXPECT["wn_no_projection"]
    c = _case(nets, cid)
    sd = states[c["fw"]]
    dumps, _, raw32 = model_raw(c)
    viol = part4(c, sd, dumps, model_grads(raw32, sd, c, no_projection=True))[0]
    assert any(f" {name}" in v for v in viol), viol[:3]


# what the whole-tensor norm ratios of tests/test_gpu_render_bwd.py let through: part 4 names each of them
@pytest.mark.parametrize("mut,cid,name", [("bias_neighbour_row", "sdf-VolSDF-65", "grad.sdf.5.bias"), ("skip_enc_from_we0", "sdf-VolSDF-65", "grad.sdf.4.weight_v"),
                                          ("no_rsqrt2_skip", "sdf-VolSDF-65", "grad.sdf.4.weight_v"), ("w8_no_adot_sums", "sdf-VolSDF-65", "grad.sdf.8.weight_v"),
                                          ("ragged_row_dropped", "sdf-VolSDF-65", "grad.sdf.")])
def test_part_4_also_names_what_the_norm_ratios_let_through(states, nets, mut, cid, name):
    """(A lost lo half, 2^-9 of an element, stays inside the bf16 noise of the dumps that part 4's allowance is made of: parts 1 and 2 hold the lo
    columns where they lie.)"""
    c = _case(nets, cid)
    sd = states[c["fw"]]
    dumps, _, raw32 = model_raw(c, mut if mut in G.REDUCE_MUTANTS else None)
    got = model_grads(raw32, sd, c, fold_mut=mut if mut in G.FOLD_MUTANTS else None)
    viol = part4(c, sd, dumps, got)[0]
    assert any(f" {name}" in v for v in viol), f"check_param_grads accepted '{mut}': {viol[:3]}"
