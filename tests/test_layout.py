"""CPU tests (-m "not gpu"): repository contracts — the C-ABI library loads and exports every symbol that
include/omg_hip.h declares, the product never imports the oracle, and the product refuses to compute on CPU."""
import ast
import os
import re
import subprocess
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def header_symbols():
    src = open(os.path.join(ROOT, "include", "omg_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(omg_[a-z0-9_]+)\s*\(", src)))


def test_library_exports_every_declared_symbol():
    from omg_amd import _lib
    lib = _lib.lib()                       # raises if libomg_hip.so is missing or stale
    declared = header_symbols()
    assert len(declared) >= 18
    assert declared == sorted(_lib.SYMBOLS), "the bindings are the header's prototypes, no more and no fewer"
    for name in declared:
        assert hasattr(lib, name), f"{name} declared in include/omg_hip.h but not exported"
    nm = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True).stdout
    for name in declared:
        assert re.search(rf"\bT {name}\b", nm), f"{name} is not a defined text symbol"
    for name in re.findall(r"\bT (omg_\w+)$", nm, flags=re.M):
        assert name in declared, f"{name} is exported but include/omg_hip.h does not declare it"
    assert lib.omg_abi_version() == 6 == _lib.OMG_ABI_VERSION


def c_layout(header_dir, structs):
    """{struct: [sizeof, (offsetof, sizeof) of every field ...]} as gcc lays them out, from ONE compiled program."""
    lines = []
    for name, cls in structs.items():
        lines.append(f'printf("{name} %zu", sizeof({name}));')
        lines += [f'printf(" %zu %zu", offsetof({name}, {f}), sizeof((({name}*)0)->{f}));' for f, _ in cls._fields_]
        lines.append('printf("\\n");')
    code = '#include <stdio.h>\n#include <stddef.h>\n#include "omg_hip.h"\nint main(){\n' + "\n".join(lines) + "\nreturn 0;}\n"
    exe = os.path.join(ROOT, "tests", "_layout.out")
    subprocess.run(["gcc", "-x", "c", "-I", header_dir, "-o", exe, "-"], input=code.encode(), check=True)
    try:
        out = subprocess.check_output([exe], text=True)
    finally:
        os.remove(exe)
    return {row[0]: [int(v) for v in row[1:]] for row in (line.split() for line in out.splitlines())}


def test_struct_layouts_match_the_header():
    """Every generated ctypes.Structure has the size, and every field the offset and size, that the C compiler gives the header's struct."""
    import ctypes
    from omg_amd import _lib
    assert len(_lib.STRUCTS) >= 13
    want = c_layout(os.path.join(ROOT, "include"), _lib.STRUCTS)
    assert sorted(want) == sorted(_lib.STRUCTS)
    for name, cls in _lib.STRUCTS.items():
        got = [ctypes.sizeof(cls)]
        for f, _ in cls._fields_:
            got += [getattr(cls, f).offset, getattr(cls, f).size]
        assert got == want[name], name


SYNTHETIC = """
/* a comment with int omg_not_a_prototype(void); inside */
#ifndef T_H
#define T_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif
#define T_N 3
enum { T_A = 0, T_B = -2 };
typedef struct { int32_t a; const void* p; float f[T_N], g; } t_inner;
typedef struct { uint8_t tag; t_inner in[2]; int64_t n; const t_inner* q; } t_outer;
const char* omg_name(void);
void omg_set(int v);
int64_t omg_run(const t_outer* a, const int32_t* idx, long long* ts, float s, void* stream);
#ifdef __cplusplus
}
#endif
#endif
"""


def test_the_header_parser_on_synthetic_text():
    import ctypes
    from omg_amd import _lib
    structs, symbols, consts = _lib.parse_header(SYNTHETIC)
    assert consts == {"T_N": 3, "T_A": 0, "T_B": -2}                       # the include guard defines no value
    inner, outer = structs["t_inner"], structs["t_outer"]
    assert [f for f, _ in inner._fields_] == ["a", "p", "f", "g"] and [f for f, _ in outer._fields_] == ["tag", "in", "n", "q"]
    assert ctypes.sizeof(inner) == 32 and inner.f.offset == 16 and inner.f.size == 12 and inner.g.offset == 28      # array sized by the #define
    assert ctypes.sizeof(outer) == 88 and getattr(outer, "in").offset == 8 and outer.n.offset == 72                 # nested by value, 8-aligned
    assert outer.q.size == 8 and dict(outer._fields_)["q"] is ctypes.c_void_p
    assert symbols == {"omg_name": (ctypes.c_char_p, []), "omg_set": (None, [ctypes.c_int32]),
                       "omg_run": (ctypes.c_int64, [ctypes.POINTER(outer), ctypes.c_void_p, ctypes.c_void_p, ctypes.c_float, ctypes.c_void_p])}
    bad = {"unknown type 'double'": "int omg_f(double x);",
           "unknown type 'size_t'": "typedef struct { size_t n; } t_s;",
           "unknown type 't_later\\*'": "int omg_f(const t_later* a);",
           "unknown return type 'void\\*'": "void* omg_f(int x);",
           "not understood: 'typedef union": "typedef union { int a; float b; } t_u;",
           "not understood: 'int omg_f": "int omg_f(int (*cb)(int));",
           "unknown type 'int a :'": "typedef struct { int a : 3; } t_b;",
           "not understood: '#if T_N": "#if T_N > 2\nint omg_f(void);\n#endif",
           "not understood: 'static int x": "int omg_f(void);\nstatic int x;",
           "not an integer constant: 'T_MISSING'": "typedef struct { int a[T_MISSING]; } t_a;"}
    for message, text in bad.items():
        with pytest.raises(_lib.OmgHipError, match=message):
            _lib.parse_header(text)


def test_product_never_imports_the_oracle():
    bad = []
    for dirpath, _, files in os.walk(os.path.join(ROOT, "omg_amd")):
        for f in files:
            if not f.endswith(".py"):
                continue
            tree = ast.parse(open(os.path.join(dirpath, f)).read())
            for node in ast.walk(tree):
                names = []
                if isinstance(node, ast.Import):
                    names = [a.name for a in node.names]
                elif isinstance(node, ast.ImportFrom):
                    names = [node.module or ""]
                if any(n == "oracle" or n.startswith("oracle.") for n in names):
                    bad.append(os.path.join(dirpath, f))
    assert not bad, f"product files import the oracle: {bad}"


def test_no_cpu_fallback():
    from omg_amd import _lib, ops
    x = torch.zeros(8, 8, dtype=torch.float16)
    with pytest.raises(_lib.OmgHipError):
        ops.gemm(x, x)
    with pytest.raises(_lib.OmgHipError):
        ops.layernorm(x, x[0], x[0], 1e-5)
    from omg_amd.unet import UNet2DConditionModel, UNetConfig
    u = UNet2DConditionModel(UNetConfig.tiny(), device="meta")
    with pytest.raises(_lib.OmgHipError):
        u(torch.zeros(1, 4, 16, 16), 1, encoder_hidden_states=torch.zeros(1, 77, 128))


def test_reference_is_not_needed_at_runtime():
    """Nothing under omg_amd/, bench.py or __graft_entry__.py may read /root/reference (absent on the GPU box)."""
    for path in ["bench.py", "__graft_entry__.py"] + [os.path.join("omg_amd", f) for f in os.listdir(os.path.join(ROOT, "omg_amd")) if f.endswith(".py")]:
        src = open(os.path.join(ROOT, path)).read()
        code = "\n".join(l for l in src.splitlines() if "sys.path" in l or "open(" in l or "import " in l)
        assert "/root/reference" not in code, path


def test_bench_power_sampler_parses_rocm_smi_json():
    """bench.py's `power` object: the rocm-smi JSON of one poll -> clock / power / cap (no GPU needed for the parser)."""
    import importlib.util
    spec = importlib.util.spec_from_file_location("omg_bench", os.path.join(ROOT, "bench.py"))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    txt = ('{"card0": {"Temperature (Sensor junction) (C)": "45.0", "sclk clock speed:": "(1857Mhz)", "sclk clock level:": "1", '
           '"mclk clock speed:": "(2000Mhz)", "Current Socket Graphics Package Power (W)": "1102.0", "Max Graphics Package Power (W)": "1400.0"}}')
    assert bench.PowerSampler.parse(txt) == {"sclk": 1857.0, "w": 1102.0, "cap": 1400.0}
    s = bench.PowerSampler(0)
    s.rows = [{"sclk": 1600.0, "w": 1400.0, "cap": 1400.0}, {"sclk": 1700.0, "w": 1390.0}]
    out = s.summary()
    assert out["avg_sclk_mhz"] == 1650.0 and out["avg_w"] == 1395.0 and out["cap_w"] == 1400.0 and out["samples"] == 2


def test_bench_dump_outputs_are_float_seeded_and_bounded(tmp_path):
    """bench.py --dump-outputs: float32 / float64 .npy files, at most 64 MB, a large output as the same seeded sample every time."""
    import importlib.util
    import numpy as np
    spec = importlib.util.spec_from_file_location("omg_bench", os.path.join(ROOT, "bench.py"))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    g = torch.Generator().manual_seed(0)
    outs = {"latents": torch.randn(8, 2, 4, 128, 128, generator=g), "images": torch.rand(2, 2, 3, 512, 768, generator=g), "absent": None}
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), outs)
    names = sorted(os.listdir(tmp_path / "a"))
    assert names == ["images_sample.npy", "images_sample_index.npy", "latents.npy"]
    assert sum(os.path.getsize(tmp_path / "a" / n) for n in names) <= 64 << 20
    for n in names:
        a, b = np.load(tmp_path / "a" / n), np.load(tmp_path / "b" / n)
        assert a.dtype in (np.float32, np.float64) and np.array_equal(a, b), n
    assert np.array_equal(np.load(tmp_path / "a" / "latents.npy"), outs["latents"].numpy())
    idx = np.load(tmp_path / "a" / "images_sample_index.npy").astype(np.int64)
    assert len(idx) == bench.DUMP_MAX_VALUES and idx.min() >= 0 and idx.max() < outs["images"].numel()
    assert np.array_equal(np.load(tmp_path / "a" / "images_sample.npy"), outs["images"].reshape(-1).numpy()[idx])


def test_bench_rejects_fewer_than_one_timed_step():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "0"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 2 and "--steps" in r.stderr, r.stderr


@pytest.mark.parametrize("extra", [["--by-shape", "shapes.txt"], ["--dedup-steps", "2"]])
def test_bench_extras_without_full_are_refused(extra):
    """A plain run measures the headline only: asking it for a roofline table or a dedup region without --full is an error, not a no-op."""
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + extra, capture_output=True, text=True, timeout=300)
    assert r.returncode == 2 and "--full" in r.stderr, r.stderr


def test_groupnorm_workspace_holds_partials_and_folded_statistics():
    from omg_amd import _lib
    lib = _lib.lib()
    B, G = 64, 32
    assert lib.omg_groupnorm_ws_floats(B, G, 16384) == B * 1024 * G * 2 + B * G * 2
