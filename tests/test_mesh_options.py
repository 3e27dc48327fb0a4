"""Which calls mesh_util.extract_mesh refuses, with which message, and in which order of precedence - over the full product of its switches, on
the CPU, with no surface and no library.  The expectation is an ordered list of (predicate on the options, message prefix): the first rule
that matches names the ValueError; a call no rule matches must get past validation, i.e. fail on the missing surface or library with something
that is not a ValueError.  Nothing may be written by any of the calls.

The matrix gives 1,436 refusals and 100 calls past validation.  It reaches 12 distinct messages: every rule of the list, which is every refusal
extract_mesh's argument checks make except refine_evals < 0 (no value of the matrix is negative; it has its own test)."""
import itertools
import os
import types

import pytest

BACKENDS = ("native", "skimage", "other")
TEXTURE = ("off", "ply", "obj", "obj_patch0")

edges = lambda o: bool(o.refine_evals or o.vertex_normals or o.color_model is not None or o.simplify_factor is not None or o.texture)
RULES = [
    (lambda o: o.texture and not o.filepath.endswith(".obj"), "extract_mesh: texture_model writes OBJ + MTL + PNG: filepath must end in .obj (got 'x.ply')"),
    (lambda o: o.texture and o.color_model is not None, "extract_mesh: texture_model and color_model exclude each other"),
    (lambda o: o.texture and o.reference_shear, "extract_mesh: texture_model needs the regular grid"),
    (lambda o: o.texture and o.backend == "skimage", "extract_mesh: texture_model needs backend='native'"),
    (lambda o: o.texture and o.texture_patch < 1, "extract_mesh: texture_patch must be >= 1 and texture_project >= 0 (got 0, 0)"),
    (lambda o: o.simplify_factor is not None and o.reference_shear, "extract_mesh: simplify_factor needs the regular grid"),
    (lambda o: o.simplify_factor is not None and o.backend == "skimage", "extract_mesh: simplify_factor needs backend='native'"),
    (lambda o: o.narrow_band and o.reference_shear, "extract_mesh: narrow_band needs the regular grid"),
    (lambda o: o.narrow_band and o.backend == "skimage", "extract_mesh: narrow_band needs backend='native'"),
    (lambda o: o.keep_largest is not None and o.backend != "native", "extract_mesh: keep_largest / min_component_faces need backend='native'"),
    (lambda o: edges(o) and (o.reference_shear or o.backend != "native"),
     "extract_mesh: refine_evals / vertex_normals / color_model need backend='native' and the regular grid"),
    (lambda o: o.backend not in ("native", "skimage"), "extract_mesh: backend must be 'native' or 'skimage' (got 'other')"),
]


def options():
    """The 3 * 2^7 * 4 = 1,536 combinations: (what the rules read, the keyword arguments of the call)."""
    for backend, shear, refine, normals, colour, keep, band, simplify, texture in itertools.product(
            BACKENDS, (False, True), (0, 2), (False, True), (None, object()), (None, 1), (False, True), (None, 2), TEXTURE):
        kw = dict(backend=backend, reference_shear=shear, refine_evals=refine, vertex_normals=normals, color_model=colour, keep_largest=keep,
                  narrow_band=band, simplify_factor=simplify, filepath="x.ply" if texture in ("off", "ply") else "x.obj")
        if texture != "off":
            kw.update(texture_model=object(), texture_patch=0 if texture == "obj_patch0" else 4)
        yield types.SimpleNamespace(texture=texture != "off", **{"texture_patch": 4, **kw}), kw


def test_every_combination_is_refused_by_the_first_rule_it_breaks_or_passes_validation(tmp_path, monkeypatch):
    from nerfart_amd import mesh_util
    monkeypatch.chdir(tmp_path)
    refused, passed, messages, hits = 0, 0, set(), [0] * len(RULES)
    for o, kw in options():
        rule = next((k for k, (broken, _) in enumerate(RULES) if broken(o)), None)
        try:
            mesh_util.extract_mesh(None, N=8, **kw)
            raise AssertionError(f"{kw}: a call without a surface returned")
        except ValueError as e:
            assert rule is not None, f"{kw}: refused ({e}), no rule says so"
            assert str(e).startswith(RULES[rule][1]), f"{kw}: expected {RULES[rule][1]!r}, got {str(e)!r}"
            refused, hits[rule] = refused + 1, hits[rule] + 1
            messages.add(str(e))
        except (ImportError, AttributeError) as e:                 # past validation: no library, or with it no surface
            assert rule is None, f"{kw}: expected {RULES[rule][1]!r}, got past validation ({type(e).__name__}: {e})"
            passed += 1
    assert (refused, passed, len(messages)) == (1436, 100, 12) and all(hits), (refused, passed, len(messages), hits)
    assert os.listdir(tmp_path) == []


def test_a_negative_refine_evals_is_refused(tmp_path, monkeypatch):
    """On an otherwise valid call.  Where extract_mesh still has its private _extract_mesh_with_vertex_data this check sits behind the import of the
    library, so there - and only there - a machine without the library sees the ImportError first."""
    from nerfart_amd import mesh_util
    monkeypatch.chdir(tmp_path)
    try:
        from nerfart_amd import hip  # noqa: F401
        library = True
    except ImportError:
        library = False
    if library or not hasattr(mesh_util, "_extract_mesh_with_vertex_data"):
        with pytest.raises(ValueError, match="extract_mesh: refine_evals must be >= 0 \\(got -1\\)"):
            mesh_util.extract_mesh(None, N=8, refine_evals=-1)
    else:
        with pytest.raises(ImportError):
            mesh_util.extract_mesh(None, N=8, refine_evals=-1)
    assert os.listdir(tmp_path) == []
