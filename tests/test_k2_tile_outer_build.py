"""Compile-time facts of the tile-outer K2 (csrc/mlp_k2_f16x1_to.hip), from hipcc's resource report and the ISA (no GPU): no scratch, no spills, two
waves per SIMD; the audit of tools/audit_asm_loads.py (no instruction touches an asm load's destination before a sufficient counted wait, no control
flow inside a counted window, MFMA results left alone long enough); and the instruction counts the layout implies."""
import importlib.util
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "nerfart_amd", "csrc", "mlp_k2_f16x1_to.hip")


@pytest.fixture(scope="module")
def compiled(tmp_path_factory):
    from nerfart_amd import build
    out = str(tmp_path_factory.mktemp("k2to") / "k.s")
    r = subprocess.run([build._hipcc()] + build.FLAGS + ["--offload-device-only", "-S", "-Rpass-analysis=kernel-resource-usage", SRC, "-o", out],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    text = open(out).read().split("\n")
    a = next(i for i, l in enumerate(text) if re.match(r"^_ZN7nerfart5f16x113k_sdf_only_to\w+:", l))
    b = next(i for i in range(a, len(text)) if text[i].startswith(".Lfunc_end"))
    return r.stderr, text[a:b]


pytestmark = pytest.mark.skipif(shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"), reason="needs hipcc (cross-compiles gfx950 without a GPU)")


def test_no_scratch_no_spills_two_waves_per_simd(compiled):
    report, _ = compiled
    assert "k_sdf_only_to" in report
    facts = {k: int(v) for k, v in re.findall(r"remark:\s+(ScratchSize \[bytes/lane\]|SGPRs Spill|VGPRs Spill|Occupancy \[waves/SIMD\]|VGPRs): (\d+)", report)}
    print("  ", facts)
    assert facts["ScratchSize [bytes/lane]"] == 0 and facts["SGPRs Spill"] == 0 and facts["VGPRs Spill"] == 0
    assert facts["Occupancy [waves/SIMD]"] == 2 and facts["VGPRs"] <= 256


def test_isa_audit_and_instruction_counts(compiled):
    _, body = compiled
    spec = importlib.util.spec_from_file_location("audit_asm_loads", os.path.join(ROOT, "tools", "audit_asm_loads.py"))
    audit = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(audit)
    n, p = audit.audit(body, "k_sdf_only_to")
    n2, p2 = audit.audit_mfma(body, "k_sdf_only_to")
    assert not p and not p2, (p + p2)[:10]
    code = [l.strip() for l in body]
    count = lambda op: sum(1 for l in code if l.startswith(op))
    # four layer bodies (layer 0, a hidden layer, the skip layer, layer 7), 8 pairs each, two point groups per fragment:
    #   MFMAs      layer 0: 32 items x 6; hidden and layer 7: 128 items x 2; skip: 8 pairs x (14 items x 2 + 4 items x 6)
    assert count("v_mfma_f32_16x16x32_f16") == 192 + 256 + 416 + 256
    #   asm reads  fragments 64 + 128 + 8 x (14 + 4 x 2) + 128; biases 16 + 16 + 16 + 14; the sdf row 16; + the 2 plain bias reads of a tile's first pair
    assert count("ds_read_b128") == (64 + 128 + 176 + 128) + (16 + 16 + 16 + 14) + 16 + 2
    assert n >= 64 + 128 + 176 + 128 and n2 > 0
    #   LDS-DMA    the burst 8; during layer 0: 4; hidden: 3 x 4 + 8 (the next layer may be the skip layer); skip: 3 x 8 + 4; layer 7: 3 x 4 + 8
    assert count("global_load_lds_dwordx4") == 8 + 4 + 20 + 28 + 20
    #   barriers   one per chunk (1 + 4 + 4 + 4) + the table load
    assert count("s_barrier") == 14
    assert not any("scratch_" in l for l in code)
