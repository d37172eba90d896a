"""ctypes binding of ``libomg_hip.so``, derived from ``include/omg_hip.h``.

The header is the one declaration of the C ABI: the ``.hip`` files include it, so the compiler checks it against the code, and this
module parses it at import into ``STRUCTS`` (argument structs), ``SYMBOLS`` (prototypes) and ``CONSTS`` (enums and integer
``#define``s).  A new entry point, struct field or constant is declared in the header and nowhere else.  Importing needs neither the
library nor a compiler; the parser knows only the header's narrow grammar and refuses everything else.

There is deliberately NO fallback: if the shared library has not been built
(``python -c 'import __graft_entry__ as g; g.build()'`` or ``make -C omg_amd/csrc``)
importing :func:`lib` raises — the product path never computes on the CPU.
"""
from __future__ import annotations

import ctypes as C
import os
import re

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("OMG_HIP_LIB") or os.path.join(_HERE, "csrc", "libomg_hip.so")   # override: A/B builds in tools/
HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "omg_hip.h")


class OmgHipError(RuntimeError):
    pass


# ---------------------------------------------------------------------------------------------- the header's grammar
_SCALARS = {"int": C.c_int32, "int32_t": C.c_int32, "int64_t": C.c_int64, "float": C.c_float, "uint8_t": C.c_uint8}
_POINTEES = set(_SCALARS) | {"void", "char", "long long"}       # what a pointer that becomes c_void_p may point to
_PREPROC = re.compile(r"^[ \t]*#[ \t]*(?:include\b.*|ifndef[ \t]+\w+|ifdef[ \t]+__cplusplus|endif|define[ \t]+(\w+)(?:[ \t]+(\S+))?)[ \t]*$", re.M)
_ENUM = re.compile(r"\benum\s*\{([^{}]*)\}\s*;")
_STRUCT = re.compile(r"\btypedef\s+struct\s*\{([^{}]*)\}\s*(\w+)\s*;")
_PROTO = re.compile(r"(?:\bconst\s+)?\b([\w ]+?)\s*(\*?)\s*\b(omg_\w+)\s*\(([^()]*)\)\s*;")
_DECL = re.compile(r"(?:const\s+)?(.+?)\s*(\*?)\s*\b(\w+)\s*(?:\[(\w+)\])?")       # type, pointer, name, array length


def parse_header(text: str):
    """C header text -> (structs, symbols, consts); raises OmgHipError on anything outside the grammar."""
    structs, symbols, consts = {}, {}, {}

    def integer(word):
        try:
            return consts[word] if word in consts else int(word, 0)
        except ValueError:
            raise OmgHipError(f"omg_hip.h: not an integer constant: {word!r}") from None

    def ctype(base, ptr, arg):
        if ptr and base in structs:
            return C.POINTER(structs[base]) if arg else C.c_void_p
        if ptr and base in _POINTEES:
            return C.c_void_p
        if not ptr and base in _SCALARS:
            return _SCALARS[base]
        if not ptr and base in structs:
            return structs[base]
        raise OmgHipError(f"omg_hip.h: unknown type {base + ptr!r}")

    def decls(items, arg):
        """'const void* A', 'int32_t H[4]' ... -> [(name, ctype)]"""
        out = []
        for item in items:
            m = _DECL.fullmatch(item.strip())
            if not m:
                raise OmgHipError(f"omg_hip.h: cannot parse declaration {item.strip()!r}")
            base, ptr, name, length = m.groups()
            t = ctype(base, ptr, arg)
            out.append((name, t * integer(length) if length else t))
        return out

    def define(m):
        if m.group(2) is not None:
            consts[m.group(1)] = integer(m.group(2))
        return ""

    def enum(m):
        for item in m.group(1).split(","):
            name, eq, value = (s.strip() for s in item.partition("="))
            if not (re.fullmatch(r"\w+", name) and eq):
                raise OmgHipError(f"omg_hip.h: cannot parse enumerator {item.strip()!r}")
            consts[name] = integer(value)
        return ""

    def struct(m):
        fields = []
        for decl in filter(None, (d.strip() for d in m.group(1).split(";"))):
            first, *more = decl.split(",")                                  # `int32_t M, N, K`: the later names repeat the first's type
            head = _DECL.fullmatch(first.strip())
            if not head:
                raise OmgHipError(f"omg_hip.h: cannot parse declaration {decl!r}")
            fields += decls([first] + [f"{head.group(1)}{head.group(2)} {d}" for d in more], arg=False)
        structs[m.group(2)] = type(m.group(2), (C.Structure,), {"_fields_": fields})
        return ""

    def proto(m):
        base, ptr, name, params = m.groups()
        if ptr:
            if base != "char":
                raise OmgHipError(f"omg_hip.h: unknown return type {base + ptr!r} of {name}")
            res = C.c_char_p
        else:
            res = None if base == "void" else ctype(base, "", arg=True)
        args = [] if params.strip() == "void" else [t for _, t in decls(params.split(","), arg=True)]
        symbols[name] = (res, args)
        return ""

    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    text = _PREPROC.sub(define, text)
    text = re.sub(r'\bextern\s+"C"\s*\{(.*)\}', r"\1", text, flags=re.S)
    for pattern, consume in ((_ENUM, enum), (_STRUCT, struct), (_PROTO, proto)):
        text = pattern.sub(consume, text)
    if text.strip():
        raise OmgHipError(f"omg_hip.h: not understood: {text.strip()[:200]!r}")
    return structs, symbols, consts


with open(HEADER_PATH) as _f:
    STRUCTS, SYMBOLS, CONSTS = parse_header(_f.read())      # C struct name -> Structure; name -> (restype, argtypes); name -> int


def _consts(*names):
    return [CONSTS["OMG_" + n] for n in names]


# the names the package, the tests and the tools use
OMG_F16, OMG_BF16, OMG_F32 = _consts("F16", "BF16", "F32")
OMG_OK, OMG_EINVAL, OMG_EDTYPE, OMG_ELAUNCH = _consts("OK", "EINVAL", "EDTYPE", "ELAUNCH")
ACT_NONE, ACT_SILU, ACT_GEGLU = _consts("ACT_NONE", "ACT_SILU", "ACT_GEGLU")
LORA_PLAIN, LORA_HADA, LORA_KRON = _consts("LORA_PLAIN", "LORA_HADA", "LORA_KRON")
OMG_ABI_VERSION, MAX_CONCEPTS, LORA_MAX_TERMS = _consts("ABI_VERSION", "MAX_CONCEPTS", "LORA_MAX_TERMS")
GemmArgs, GemmMx8Args = STRUCTS["omg_gemm_args"], STRUCTS["omg_gemm_mx8_args"]
Conv2dArgs, Conv2dSlotsArgs, Conv2dMx8Args = STRUCTS["omg_conv2d_args"], STRUCTS["omg_conv2d_slots_args"], STRUCTS["omg_conv2d_mx8_args"]
Conv2dF32Args, Conv2dF32WinoArgs = STRUCTS["omg_conv2d_f32_args"], STRUCTS["omg_conv2d_f32_wino_args"]
AttnArgs, VMapArgs, MsdeformArgs, StepArgs = STRUCTS["omg_attn_args"], STRUCTS["omg_vmap_args"], STRUCTS["omg_msdeform_args"], STRUCTS["omg_step_args"]
LoraTermDesc, LoraMergeArgs = STRUCTS["omg_lora_term"], STRUCTS["omg_lora_merge_args"]

_lib = None


def lib() -> C.CDLL:
    """Load (once) and return the shared library; raise loudly if it is missing."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise OmgHipError(
            f"{LIB_PATH} not found: the HIP extension has not been built. "
            "Run `python -c 'import __graft_entry__ as g; g.build()'` (needs hipcc). "
            "omg_amd has no CPU fallback."
        )
    # torch bundles its own libamdhip64 (same SONAME as /opt/rocm's): it must be in the process
    # BEFORE this library is, so that both resolve to ONE HIP runtime (streams, allocations and
    # graph capture are shared).  Loading in the other order yields hipErrorNoDevice at first launch.
    import torch  # noqa: F401

    l = C.CDLL(LIB_PATH)
    for name, (res, args) in SYMBOLS.items():
        fn = getattr(l, name)  # AttributeError if the .so is stale
        fn.restype = res
        fn.argtypes = args
    if l.omg_abi_version() != OMG_ABI_VERSION:
        raise OmgHipError("libomg_hip.so ABI version mismatch; rebuild")
    v = os.environ.get("OMG_GEMM_VARIANT")      # debugging/benchmarking aid: force one GEMM tile configuration
    if v:
        l.omg_debug_set_gemm_variant(int(v))
    v = os.environ.get("OMG_ATTN_VARIANT")      # ditto for the attention kernels (bit 16: attn_fwd_kernel7 without its XCD-aware block order)
    if v:
        l.omg_debug_set_attn_variant(int(v, 0))
    v = os.environ.get("OMG_MX8_SPLIT")         # ditto for the MX-fp8 GEMM: DMA split | debug bits << 8 (128 << 8: the one-tile-per-block form of the Linear kernel)
    if v:
        l.omg_debug_set_mx8_split(int(v, 0))
    _lib = l
    return l


def check(rc: int, what: str) -> None:
    if rc != 0:
        msg = lib().omg_last_error()
        raise OmgHipError(f"{what} failed (rc={rc}): {msg.decode() if msg else ''}")
