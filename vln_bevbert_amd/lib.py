"""ctypes binding of libbevbert_hip.so, derived from its C ABI: include/bevbert_hip.h is parsed once per process and
gives every entry point its restype / argtypes and both state structs their fields -- nothing of the ABI is typed here.

The shared library is built in-tree by ``__graft_entry__.build()`` (hipcc --offload-arch=gfx950).
There is deliberately NO fallback: if the library is missing or a call fails, an exception is raised --
this package never routes work to PyTorch eager kernels or to the CPU oracle.
"""
import ctypes
import functools
import glob
import os
import re
import subprocess

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libbevbert_hip.so")
CSRC = os.path.join(_HERE, "csrc")
# Per-file compiler flags.  The persistent attention forward is compiled without the SLP vectoriser: it packs pairs of
# fp32 operations into v_pk_*_f32 instructions, and on gfx950 packed fp32 instructions do not overlap with the matrix
# instructions of the SIMD's other wave while plain ones do (scripts/probes/mfma_valu_overlap.hip,
# profiles/r05_mfma_valu_overlap_probe.txt).  Measured on that kernel: no difference either way.
EXTRA_FLAGS = {"attn_fwd4.hip": ["-fno-slp-vectorize"]}
SOURCES = ["splat.hip", "layernorm.hip", "colwise.hip", "optimizer.hip", "gather.hip", "pointwise.hip", "attn_simple.hip", "attn_f32.hip", "attn_mfma.hip", "attn_bwd1.hip", "attn_fwd2.hip", "attn_fwd4.hip", "attn_bwd7p1.hip", "attn_small.hip", "attn_short.hip", "smallk.hip", "sap_loss.hip", "graph_nav.hip", "nav_expert.hip", "nav_obj.hip", "waypoint.hip", "ce_map.hip", "ce_train.hip", "val_metrics.hip", "vit.hip", "depth_resnet.hip", "path_data.hip", "gemm.hip", "capi.hip"]
HEADER = os.path.join(os.path.dirname(_HERE), "include", "bevbert_hip.h")

F32, BF16, F16 = 0, 1, 2
_DT = {torch.float32: F32, torch.bfloat16: BF16, torch.float16: F16}


class BevBertHipError(RuntimeError):
    pass


def dtype_code(t):
    try:
        return _DT[t.dtype if torch.is_tensor(t) else t]
    except KeyError:
        raise BevBertHipError(f"unsupported dtype {t}") from None


def build(force=False, verbose=False):
    """Compile csrc/*.hip into libbevbert_hip.so for gfx950 (cross-compiles without a GPU): one object per source
    (only the stale ones, in parallel), then one link."""
    from concurrent.futures import ThreadPoolExecutor
    headers = glob.glob(os.path.join(CSRC, "*.h")) + [HEADER]
    hdr_time = max(os.path.getmtime(h) for h in headers)
    objdir = os.path.join(_HERE, "_obj")
    os.makedirs(objdir, exist_ok=True)
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    flags = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-fvisibility=hidden"]
    jobs, objs = [], []
    for name in SOURCES:
        src, obj = os.path.join(CSRC, name), os.path.join(objdir, name[:-4] + ".o")
        objs.append(obj)
        if force or not os.path.exists(obj) or os.path.getmtime(obj) < max(os.path.getmtime(src), hdr_time):
            jobs.append([hipcc] + flags + EXTRA_FLAGS.get(name, []) + ["-c", src, "-o", obj])
    if not jobs and os.path.exists(LIB_PATH) and all(os.path.getmtime(LIB_PATH) >= os.path.getmtime(o) for o in objs):
        return LIB_PATH

    def run(cmd):
        if verbose:
            print(" ".join(cmd), flush=True)
        subprocess.run(cmd, check=True, cwd=CSRC)

    with ThreadPoolExecutor(max_workers=min(8, max(1, len(jobs)))) as ex:
        list(ex.map(run, jobs))
    run([hipcc, "--offload-arch=gfx950", "-shared", "-fPIC", "-o", LIB_PATH] + objs + ["-lhipblaslt"])
    return LIB_PATH


# ---- the C ABI, read from include/bevbert_hip.h ----------------------------------------------------------------------
# The header is the only place where a prototype or a state struct is written down.  The map below is closed: a
# declaration using anything else is an error, never a guess.  Pointers (struct pointers and [] parameters included) are
# c_void_p, so callers may pass data_ptr() ints, ctypes.addressof results, byref objects and ctypes arrays alike.
_SCALARS = {"int": ctypes.c_int, "int64_t": ctypes.c_int64, "uint64_t": ctypes.c_uint64, "uint32_t": ctypes.c_uint32,
            "float": ctypes.c_float, "double": ctypes.c_double, "hipStream_t": ctypes.c_void_p}
_POINTEES = {"void", "char", "uint8_t", "int16_t", *_SCALARS}       # and the header's own structs
_DECL = re.compile(r"""\s*(?: typedef\s+struct\s+\w+\s*\*\s*hipStream_t\s*;                               # the opaque handle
    | typedef\s+struct\s+\w*\s*\{(?P<body>(?:[^{};]+;)+)\s*\}\s*(?P<struct>\w+)\s*;                       # a state struct
    | (?P<ret>[\w\s*]+?)\b(?P<fn>\w+)\s*\((?P<params>[^(){};]*)\)\s*; )""", re.X)                        # an entry point
_VAR = re.compile(r"(?P<type>[\w\s*]+?)\b(?P<names>\w+(?:\s*,\s*\w+)*)\s*(?P<array>\[\d*\])?")


def _fail(what):
    raise BevBertHipError(f"bevbert_hip.h: {what}")


def _ctype(decl, structs):
    base = decl.replace("*", " ").replace("const ", " ").split()
    if len(base) == 1 and "*" not in decl and base[0] in _SCALARS:
        return _SCALARS[base[0]]
    if len(base) == 1 and "*" in decl and (base[0] in _POINTEES or base[0] in structs):
        return ctypes.c_char_p if base == ["char"] and decl.count("*") == 1 else ctypes.c_void_p
    _fail(f"unknown type {decl.strip()!r}")


def parse_header(text):
    """(prototypes, structs) of a C header written like include/bevbert_hip.h: {name: (restype, [argtypes])} for every
    ``ret name(params);`` and {name: [(field, ctype)]} for every ``typedef struct { ... } name;``.  Strict: anything else
    that is not a comment, a preprocessor line, the extern "C" braces or hipStream_t's typedef raises."""
    text = re.sub(r"/\*.*?\*/|//[^\n]*|^[ \t]*#[^\n]*", " ", text, flags=re.S | re.M)
    m = re.fullmatch(r'\s*extern\s+"C"\s*\{(.*)\}\s*', text, re.S)
    text = (m[1] if m else text).rstrip()
    protos, structs, pos = {}, {}, 0
    while pos < len(text):
        m = _DECL.match(text, pos) or _fail(f"cannot parse {' '.join(text[pos:pos + 80].split())!r}")
        pos = m.end()
        if m["struct"]:
            fields = structs[m["struct"]] = []
            for f in m["body"].split(";")[:-1]:
                v = _VAR.fullmatch(f.strip())
                ct = _ctype(v["type"], structs) if v and not v["array"] else None
                if not (ct is ctypes.c_int or ct is ctypes.c_void_p and "," not in v["names"]):
                    _fail(f"{m['struct']}: field {f.strip()!r} is neither a pointer nor int")
                fields += [(n, ct) for n in v["names"].replace(",", " ").split()]
        elif m["fn"]:
            params = [] if m["params"].strip() == "void" else m["params"].split(",")
            params = [_VAR.fullmatch(p.strip()) or _fail(f"{m['fn']}: cannot parse parameter {p.strip()!r}") for p in params]
            protos[m["fn"]] = (_ctype(m["ret"], structs), [_ctype(v["type"] + "*" * bool(v["array"]), structs) for v in params])
    return protos, structs


@functools.lru_cache(None)
def _parsed():
    with open(HEADER) as f:
        return parse_header(f.read())


def prototypes():
    """{name: (restype, argtypes)} of every entry point include/bevbert_hip.h declares (parsed once per process)."""
    return _parsed()[0]


@functools.lru_cache(None)
def struct(name):
    """The ctypes.Structure of a state struct of the header (bevbert_gm_state, bevbert_ce_state): its fields in
    declaration order, pointers as c_void_p."""
    fields = _parsed()[1].get(name) or _fail(f"no struct {name}")
    return type(name, (ctypes.Structure,), {"_fields_": fields})


_lib = None


def load():
    """dlopen the library and type every entry point as the header declares it. Raises if it has not been built, or if
    it does not export a declared symbol."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise BevBertHipError(
            f"{LIB_PATH} is missing: run `python -c 'import __graft_entry__ as g; g.build()'` "
            "(there is no PyTorch/CPU fallback for the hot path)")
    lib = ctypes.CDLL(LIB_PATH)
    for name, (restype, argtypes) in prototypes().items():
        try:
            fn = getattr(lib, name)
        except AttributeError:
            raise BevBertHipError(f"{LIB_PATH} does not export {name}, which bevbert_hip.h declares") from None
        fn.restype, fn.argtypes = restype, argtypes
    _lib = lib
    return lib


_fns = {}


def call(name, *args):
    fn = _fns.get(name)
    if fn is None:
        fn = _fns[name] = getattr(load(), name)
    rc = fn(*args)
    if rc != 0:
        raise BevBertHipError(f"{name} failed ({rc}): {load().bevbert_last_error().decode()}")


def ptr(t):
    """Device pointer of a tensor (None -> NULL). The tensor must live on a HIP device."""
    if t is None:
        return None
    if not t.is_cuda:
        raise BevBertHipError("libbevbert_hip.so operates on device memory only; got a CPU tensor "
                              "(no CPU fallback exists for the hot path)")
    return t.data_ptr()


_raw_stream = torch._C._cuda_getCurrentRawStream
_device_index = None


_override = None


def stream():
    """hipStream_t the next launch goes to: torch's current stream on this process's GPU, unless a launch-stream
    override is active (ops.WgradStream).  One process per GPU: the device index is read once;
    torch.cuda.current_stream() costs ~3 us of host time per call, the raw getter ~0.2 us."""
    global _device_index
    if _override is not None:
        return _override
    if _device_index is None:
        _device_index = torch.cuda.current_device()
    return _raw_stream(_device_index)


def set_stream_override(handle):
    """Route every following C-ABI launch to `handle` (a hipStream_t as int) until reset with None."""
    global _override
    _override = handle
