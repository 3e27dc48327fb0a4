"""tools/extract_surface.py up to the GPU: its command line goes through nerfart_amd.config like the reference's tools, and the config it loads
builds the model whose implicit surface extract_mesh sweeps."""
import importlib.util
import os

import yaml

from conftest import REPO


def _tool():
    spec = importlib.util.spec_from_file_location("extract_surface", os.path.join(REPO, "tools", "extract_surface.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_command_line_and_config(tmp_path):
    from nerfart_amd import scene, frameworks
    d = scene.synthetic_config("NeuS").to_dict()
    d["expname"] = "mesh"
    d.setdefault("training", {})["log_root_dir"] = str(tmp_path)
    path = tmp_path / "neus.yaml"
    path.write_text(yaml.dump(d))
    tool = _tool()
    args, conf = tool.parse(["--config", str(path), "--load_pt", "ckpt.pt", "--N", "64", "--volume_size", "3.0", "--out", str(tmp_path / "m.ply"),
                             "--model:framework", "NeuS"])
    assert (args.N, args.volume_size, args.level, args.chunk, args.load_pt) == (64, 3.0, 0.0, 1 << 24, "ckpt.pt")
    assert conf.model.framework == "NeuS" and conf.N == 64 and conf.out.endswith("m.ply")
    assert conf.training.exp_dir == os.path.join(str(tmp_path), "mesh")
    model = frameworks.get_model(conf)[0]
    assert hasattr(model, "implicit_surface") and sum(p.numel() for p in model.implicit_surface.parameters()) > 0
    args, _ = tool.parse(["--config", str(path)])
    assert (args.N, args.volume_size, args.out, args.load_pt) == (512, 2.0, "surface.ply", None)
