"""B3, checked against the reference's scripts (CPU).  What is needed of them is recorded in tests/golden/compat_verbatim.json
(tests/golden/make_golden_compat.py writes it from a checkout of the reference), so the tests run without that checkout:

* the driver functions the GPU tests execute (tests/test_compat_gpu.py, tests/test_compat_instantid_gpu.py: ``sample_image``,
  ``build_model_sd``, ``prepare_text``) have the SAME syntax tree as the reference's (docstrings aside; compared by a SHA-256 of the
  canonical tree) — "transcribed verbatim" is checked, not claimed;
* the import statements of their ORIGINAL import blocks (everything in front of the first function: inference_lora.py:1-35,
  inference_instantid.py:1-40, the imports inside the try / except blocks around the optional detectors still guarded) execute under
  ``omg_amd.compat.install()`` and bind the names of the hot path to this package's classes.
"""
import ast
import hashlib
import json
import os
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "compat_verbatim.json")


def _tree(path):
    with open(path) as f:
        return ast.parse(f.read(), filename=path)


def _no_docstring(fn):
    if fn.body and isinstance(fn.body[0], ast.Expr) and isinstance(getattr(fn.body[0], "value", None), ast.Constant) and isinstance(fn.body[0].value.value, str):
        fn.body = fn.body[1:]
    return fn


def _functions(path):
    """top-level functions, docstrings dropped (a transcription need not carry the reference's prose)"""
    return {n.name: _no_docstring(n) for n in _tree(path).body if isinstance(n, ast.FunctionDef)}


def _import_block(path):
    body = []
    for n in _tree(path).body:
        if isinstance(n, ast.FunctionDef):
            break
        body.append(n)
    assert all(isinstance(n, (ast.Import, ast.ImportFrom, ast.Try)) for n in body), [type(n).__name__ for n in body]
    return body


def _canon(node):
    """every field of every node, positions left out: the same text for the same tree on any Python version (ast.dump's is not)"""
    if isinstance(node, ast.AST):
        return [type(node).__name__] + [[f, _canon(getattr(node, f, None))] for f in node._fields]
    if isinstance(node, list):
        return [_canon(n) for n in node]
    return repr(node)


def tree_sha256(node):
    return hashlib.sha256(json.dumps(_canon(node)).encode()).hexdigest()


def _import_entries(stmt, guarded):
    names = [[a.name, a.asname] for a in stmt.names]
    if isinstance(stmt, ast.Import):
        return [{"module": None, "level": 0, "names": names, "guarded": guarded}]
    return [{"module": stmt.module, "level": stmt.level, "names": names, "guarded": guarded}]


def import_manifest(block):
    """the import statements of an import block, in order, as data: a try / except block becomes a guarded group"""
    out = []
    for g, n in enumerate(block):
        if isinstance(n, ast.Try):
            assert all(isinstance(s, (ast.Import, ast.ImportFrom)) for s in n.body), [type(s).__name__ for s in n.body]
            out += [e for s in n.body for e in _import_entries(s, g)]
        else:
            out += _import_entries(n, None)
    return out


def _statement(e):
    alias = [ast.alias(name=n, asname=a) for n, a in e["names"]]
    return ast.Import(names=alias) if e["module"] is None and e["level"] == 0 else ast.ImportFrom(module=e["module"], names=alias, level=e["level"])


def _manifest_module(entries):
    """the manifest back as statements; a guarded group runs inside try / except as in the script"""
    body, groups = [], {}
    for e in entries:
        if e["guarded"] is None:
            body.append(_statement(e))
            continue
        if e["guarded"] not in groups:
            groups[e["guarded"]] = ast.Try(body=[], handlers=[ast.ExceptHandler(type=None, name=None, body=[ast.Pass()])], orelse=[], finalbody=[])
            body.append(groups[e["guarded"]])
        groups[e["guarded"]].body.append(_statement(e))
    return ast.fix_missing_locations(ast.Module(body=body, type_ignores=[]))


def _golden(script):
    with open(GOLDEN) as f:
        return json.load(f)[script]


@pytest.mark.parametrize("script,ours,names", [
    ("inference_lora.py", "test_compat_gpu.py", ("sample_image", "build_model_sd")),
    ("inference_instantid.py", "test_compat_instantid_gpu.py", ("sample_image", "build_model_sd", "prepare_text")),
])
def test_the_driver_functions_the_gpu_tests_run_are_the_references_own(script, ours, names):
    ref, mine = _golden(script)["functions"], _functions(os.path.join(HERE, ours))
    for n in names:
        assert tree_sha256(mine[n]) == ref[n], f"{ours}:{n} differs from {script}:{n}"


@pytest.mark.parametrize("script,hot", [
    ("inference_lora.py", ("LoraMultiConceptPipeline", "AttentionReplace", "ControlNetModel", "StableDiffusionXLPipeline",
                           "revise_regionally_controlnet_forward", "save_image")),
    ("inference_instantid.py", ("InstantidMultiConceptPipeline", "InstantidSingleConceptPipeline", "AttentionReplace", "ControlNetModel",
                                "StableDiffusionXLPipeline", "revise_regionally_controlnet_forward", "FaceAnalysis", "cv2")),
])
def test_the_original_import_block_executes_under_compat_install(script, hot, capsys):
    from omg_amd import compat
    saved_path = list(sys.path)
    try:
        compat.install()
        ns = {}
        exec(compile(_manifest_module(_golden(script)["imports"]), script, "exec"), ns)
        for n in hot:
            assert n in ns, n
        mod = lambda o: getattr(o, "__module__", "") or ""
        for n in hot:
            if n in ("save_image", "FaceAnalysis", "cv2"):
                continue                        # third-party, outside the hot path: the real package where installed, a stand-in otherwise
            assert mod(ns[n]).startswith("omg_amd."), (n, mod(ns[n]))
        # the hot-path names resolve to the classes the GPU tests exercise
        assert ns["AttentionReplace"] is __import__("omg_amd.controller", fromlist=["x"]).AttentionReplace
        assert ns["ControlNetModel"] is compat.ControlNetModel
    finally:
        compat.uninstall()
        sys.path[:] = saved_path
    assert "diffusers" not in sys.modules or not vars(sys.modules["diffusers"]).get("__omg_amd_alias__", False)
