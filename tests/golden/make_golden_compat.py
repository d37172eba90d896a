"""Record what tests/test_compat_verbatim.py needs of the reference's two scripts in compat_verbatim.json, next to this file.

    python tests/golden/make_golden_compat.py <checkout of the reference>

Per script: the SHA-256 of the canonical syntax tree of every top-level function (docstring dropped) and the import statements of the
import block in front of the first function, as data (module, names, and the try / except group a statement is guarded by).
"""
import ast
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from tests.test_compat_verbatim import _canon, _functions, _import_block, _manifest_module, import_manifest, tree_sha256  # noqa: E402

SCRIPTS = ("inference_lora.py", "inference_instantid.py")


def _imports_only(block):
    """the block with every except handler reduced to `pass`: what the manifest can give back"""
    out = []
    for n in block:
        if isinstance(n, ast.Try):
            n = ast.Try(body=n.body, handlers=[ast.ExceptHandler(type=h.type, name=h.name, body=[ast.Pass()]) for h in n.handlers],
                        orelse=n.orelse, finalbody=n.finalbody)
        out.append(n)
    return out


def main(ref):
    out = {}
    for script in SCRIPTS:
        path = os.path.join(ref, script)
        block = _import_block(path)
        manifest = import_manifest(block)
        assert _canon(_manifest_module(manifest).body) == _canon(_imports_only(block)), f"{script}: the manifest does not give the import block back"
        out[script] = {"functions": {name: tree_sha256(fn) for name, fn in sorted(_functions(path).items())}, "imports": manifest}
    with open(os.path.join(HERE, "compat_verbatim.json"), "w") as f:          # one function / one import statement per line
        f.write("{\n" + ",\n".join(
            f' {json.dumps(s)}: {{\n  "functions": {{\n' + ",\n".join(f"   {json.dumps(k)}: {json.dumps(v)}" for k, v in d["functions"].items())
            + '\n  },\n  "imports": [\n' + ",\n".join(f"   {json.dumps(e)}" for e in d["imports"]) + "\n  ]\n }"
            for s, d in out.items()) + "\n}\n")


if __name__ == "__main__":
    if len(sys.argv) != 2:
        raise SystemExit(__doc__)
    main(sys.argv[1])
