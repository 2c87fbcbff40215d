"""CPU tests of the host-side logic and of the C-ABI surface (no GPU, no compute calls)."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from oracle import bevbert_ref as R
from tests.attn_cases import ATTN_KNOBS
from tests.helpers import read_shapes
from vln_bevbert_amd import lib, synthetic
from vln_bevbert_amd.config import BevBertConfig

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_library_builds_loads_and_exports_header_symbols():
    lib.build()
    l = lib.load()
    assert l.bevbert_version() >= 100 and l.bevbert_arch() == b"gfx950"
    protos = lib.prototypes()
    assert len(protos) >= 20
    # the parser covers exactly the names the header holds: nothing is skipped, nothing invented
    with open(lib.HEADER) as f:
        assert set(protos) == set(re.findall(r"\b(bevbert_\w+)\s*\(", f.read()))
    # every one resolves in the loaded library and carries the derived typing
    for name, (restype, argtypes) in protos.items():
        fn = getattr(l, name)
        assert fn.restype is restype and list(fn.argtypes) == argtypes, name


def test_representative_prototypes_are_what_the_header_declares():
    """One entry per type kind, written out: a parser regression cannot hide behind the parser's own output."""
    P, S, I, I64, U64, U32, F, D = (ctypes.c_void_p, ctypes.c_char_p, ctypes.c_int, ctypes.c_int64, ctypes.c_uint64,
                                    ctypes.c_uint32, ctypes.c_float, ctypes.c_double)
    want = {
        # uint64_t seed / offset, const int64_t* strides, uint64_t* drop_bits
        "bevbert_attn_fwd": (I, [P, P, P, P, P, P, P, P, I, I, I, I, I, F, I, I, F, U64, U64, P, I, P]),
        # int and int64_t interleaved
        "bevbert_gemm": (I, [P, P, P, P, I, I, I, I, I, I64, I64, I64, I, I64, I64, I64, I, I, I, F, P, I64, I, P]),
        # double by value
        "bevbert_nav_metrics": (I, [P, I, I, P, P, P, I, P, P, P, I, I, D, P, P, P]),
        # struct pointer, double, double, uint32_t
        "bevbert_ce_update": (I, [P, P, P, P, P, P, P, I, P, P, P, I, D, D, U32, P, P]),
        # char* and an int64_t return
        "bevbert_gemm_tuning_export": (I64, [S, I64]),
        # const char* return, one float among ints
        "bevbert_attn_plan": (S, [I, I, I, I, I, I, I, I, F, I, I, I, I, I]),
        "bevbert_attn_drop_bits_words": (I64, [I, I, I, I]),
        # struct pointer first
        "bevbert_gm_update": (I, [P, P, P, P, P, P, P, P, P, P, I, I, P, P, P]),
        # (void)
        "bevbert_last_error": (S, []),
    }
    protos = lib.prototypes()
    for name, (restype, argtypes) in want.items():
        assert protos[name][0] is restype and protos[name][1] == argtypes, (name, protos[name])


def test_header_parser_is_strict():
    I, P = ctypes.c_int, ctypes.c_void_p
    good = ("typedef struct st { double* a; /* (B) */ int B, N; } st;\n"
            "int bevbert_a(const st* s, const float* x, int64_t n, hipStream_t stream);\n"
            "const char* bevbert_b(void);\n")
    protos, structs = lib.parse_header(good)
    assert protos == {"bevbert_a": (I, [P, P, ctypes.c_int64, P]), "bevbert_b": (ctypes.c_char_p, [])}
    assert structs == {"st": [("a", P), ("B", I), ("N", I)]}
    for bad in ("int bevbert_a(const float* x, size_t n);\n",                      # a type outside the map
                "int bevbert_a(const size_t* x, int n);\n",                        # ... also behind a pointer
                "int bevbert_a(const float* x, int n)\nint bevbert_b(void);\n",    # no terminating ;
                "int bevbert_a(int n)\n",
                "typedef struct st { double* a; float scale; int B; } st;\n",      # a field that is neither pointer nor int
                "int bevbert_a(int n);\nstatic\nint bevbert_b(void);\n",           # stray text between declarations
                "int bevbert_a(int n);\n}\n",
                "int bevbert_a(int);\n",                                           # unnamed parameter
                "int bevbert_a();\n"):                                             # no prototype
        with pytest.raises(lib.BevBertHipError):
            lib.parse_header(bad)
            pytest.fail(f"parsed: {bad!r}")


def test_state_structs_are_the_headers():
    from vln_bevbert_amd import ce_map, graph_map_dev
    gm, ce = lib.struct("bevbert_gm_state"), lib.struct("bevbert_ce_state")
    assert graph_map_dev._GmState is gm and ce_map._CeState is ce
    assert ctypes.sizeof(gm) == 96 and ctypes.sizeof(ce) == 192        # 10 pointers + 4 ints; 21 pointers + 6 ints
    assert [n for n, _ in gm._fields_] == ["pos", "dis", "point", "hops", "visited", "step_ids", "pc_list", "npc", "node_row",
                                           "node_T", "B", "N", "V", "pad"]
    assert [t for _, t in gm._fields_] == [ctypes.c_void_p] * 10 + [ctypes.c_int] * 4
    assert len(ce_map._PTRS) == 21 and ce_map._PTRS[0] == "node_pos" and ce_map._PTRS[-1] == "overflow"
    assert [n for n, _ in ce._fields_] == list(ce_map._PTRS) + ["B", "N", "Gh", "P", "H", "dtype"]
    assert [t for _, t in ce._fields_] == [ctypes.c_void_p] * 21 + [ctypes.c_int] * 6
    with pytest.raises(lib.BevBertHipError):
        lib.struct("bevbert_no_such_state")


# The attention dispatch as a table: (B, Lq, Lk, dtype, impl, graph bias, dropout p, keep-bit workspace, knobs) ->
# (forward kernel, backward kernel).  Workspace: "none" = no pointer, "empty" = passed with bits_ready = 0, "ready" = filled
# ahead by bevbert_attn_drop_bits.  dbias is wanted wherever there is a bias.  Every row was issued as a real forward +
# backward call on the commit before attn_plan_fwd / attn_plan_bwd existed (one process per knob arm) and the names are what
# bevbert_attn_last_path said there; the plan is evaluated for 256 CUs.
_A = "attn_"
ATTN_PLAN_ROWS = [
    (2, 80, 80, "bf16", 2, False, 0.1, "empty", {}, "short_fwd", "short_bwd"),              # text self-attention
    (2, 96, 96, "bf16", 2, False, 0.1, "empty", {}, "short_fwd", "short_bwd"),
    (2, 441, 80, "bf16", 2, False, 0.1, "empty", {}, "short_fwd", "mfma_bwd1"),             # BEV <- text
    (2, 441, 80, "bf16", 2, False, 0.1, "ready", {}, "short_fwd", "mfma_bwd1"),
    (2, 17, 17, "bf16", 2, True, 0.1, "empty", {}, "mfma_fwd", "mfma_bwd1"),                # global map, graph bias
    (2, 130, 200, "bf16", 2, True, 0.0, "none", {}, "mfma_fwd", "mfma_bwd"),
    (2, 100, 140, "bf16", 2, False, 0.1, "empty", {}, "mfma_fwd", "mfma_bwd1"),             # small scores: inline hash
    (2, 100, 140, "bf16", 2, False, 0.1, "ready", {}, "fwd2", "mfma_bwd1"),
    (64, 441, 441, "bf16", 2, False, 0.1, "ready", {}, "fwd4", "bwd3"),                     # BEV self-attention: 3 full rounds
    (32, 441, 441, "bf16", 2, False, 0.1, "ready", {}, "fwd2", "bwd3"),                     # 1.5 rounds
    (2, 441, 441, "bf16", 2, False, 0.1, "ready", {}, "fwd2", "bwd3"),
    (2, 441, 441, "bf16", 2, False, 0.1, "none", {}, "mfma_fwd", "mfma_bwd"),               # dropout without a workspace
    (2, 441, 441, "bf16", 2, False, 0.1, "ready", {"BEVBERT_ATTN_FWD4": "1"}, "fwd4", "bwd3"),
    (64, 441, 441, "bf16", 2, False, 0.1, "ready", {"BEVBERT_ATTN_FWD4": "0"}, "fwd2", "bwd3"),
    (2, 80, 441, "bf16", 2, False, 0.0, "none", {}, "fwd2", "bwd3"),                        # MLM: text -> BEV
    (2, 80, 600, "bf16", 2, False, 0.0, "none", {}, "fwd2", "mfma_bwd"),
    (2, 80, 80, "bf16", 2, False, 0.1, "empty", {"BEVBERT_ATTN_SHORT": "0"}, "mfma_fwd", "small_bwd2"),
    (2, 441, 80, "bf16", 2, False, 0.1, "empty", {"BEVBERT_ATTN_SHORT": "0"}, "fwd2", "mfma_bwd1"),
    (2, 80, 80, "bf16", 2, False, 0.1, "empty", {"BEVBERT_ATTN_SHORT": "0", "BEVBERT_ATTN_SMALL_BWD": "0"}, "mfma_fwd", "mfma_bwd1"),
    (2, 80, 80, "bf16", 2, False, 0.1, "empty", {"BEVBERT_ATTN_SMALL": "1"}, "small_fwd", "small_bwd2"),
    (2, 441, 80, "bf16", 2, False, 0.1, "empty", {"BEVBERT_ATTN_SMALL": "1"}, "small_fwd", "small_bwd"),
    (2, 80, 80, "bf16", 2, False, 0.1, "empty", {"BEVBERT_ATTN_FWD": "1"}, "mfma_fwd", "short_bwd"),
    (2, 441, 441, "bf16", 2, False, 0.1, "ready", {"BEVBERT_ATTN_BWD3": "0"}, "fwd2", "bwd2"),
    (2, 441, 441, "bf16", 2, False, 0.1, "ready", {"BEVBERT_ATTN_BWD": "1"}, "fwd2", "mfma_bwd1"),
    (2, 441, 441, "bf16", 2, False, 0.1, "ready", {"BEVBERT_ATTN_BWD": "split"}, "fwd2", "mfma_bwd"),
    (2, 441, 441, "bf16", 3, False, 0.1, "ready", {}, "fwd2", "mfma_bwd"),
    (2, 80, 80, "f32", 0, False, 0.0, "none", {}, "f32_fwd", "f32_bwd"),
    (2, 80, 80, "f32", 0, False, 0.0, "none", {"BEVBERT_ATTN_F32": "simple"}, "simple_fwd", "simple_bwd"),
    (2, 80, 80, "bf16", 1, False, 0.0, "none", {}, "simple_fwd", "simple_bwd"),
]


def test_attention_sources_read_only_the_listed_switches():
    """The dispatch plan is the whole rule: the only environment switches the attention sources and the C ABI name are the
    ones in ATTN_KNOBS (each read per call, each with plan rows above or cases in tests/attn_cases.py), and README.md's
    table documents every one.  A switch added without both fails here."""
    csrc = os.path.join(os.path.dirname(lib.__file__), "csrc")
    paths = [os.path.join(csrc, f) for f in sorted(os.listdir(csrc)) if re.fullmatch(r"attn_\w+\.(hip|h)|capi\.hip", f)]
    assert len(paths) >= 13, paths
    found = set()
    for path in paths:
        with open(path) as f:
            found |= set(re.findall(r'"(BEVBERT_[A-Z0-9_]+)"', f.read()))
    assert found == set(ATTN_KNOBS), sorted(found ^ set(ATTN_KNOBS))
    with open(os.path.join(os.path.dirname(os.path.dirname(lib.__file__)), "README.md")) as f:
        table = [line for line in f if line.lstrip().startswith("|")]
    for name in ATTN_KNOBS:
        assert any(f"`{name}`" in line for line in table), f"README.md's environment table has no row for {name}"


# Every environment variable the rest of the package reads.  A new entry needs a README row, and -- if it selects a code
# path -- a test, script or benchmark line that runs the path behind it; one that selects a path nothing runs goes, with
# its path.
PACKAGE_KNOBS = (
    # select a code path: a test, a script or bench.py sets it, or reaches the attribute / function that reads it
    # (BEVBERT_LT_GEMM=0 forces the fallback that problems without a plan take anyway: ops.GEMM_FALLBACKS)
    "BEVBERT_GRAPHS", "BEVBERT_OVERLAP_ZERO", "BEVBERT_GRAD_EXCHANGE", "BEVBERT_FOLD_STORE", "BEVBERT_RES32_Y32",
    "BEVBERT_NAV_TEXT_CACHE", "BEVBERT_WGRAD_STREAM", "BEVBERT_WGRAD_STREAMS", "BEVBERT_DEFER_FINALIZE", "BEVBERT_LT_GEMM",
    "BEVBERT_GEMM_TUNING",
    # guards against machine behaviour (hwqueues.py, the collective's queue)
    "BEVBERT_COPY_STREAM_PROBE", "BEVBERT_STEER_POOL", "BEVBERT_COLLECTIVE_QUEUE_CHECK",
    # sizes, counts and locations: no second code path
    "BEVBERT_WGRAD_BATCH", "BEVBERT_SCRATCH_MB", "BEVBERT_SCRATCH_MAX_MB", "BEVBERT_SCRATCH_INITIAL_MB", "BEVBERT_SPLITK_MAX",
    "BEVBERT_LT_AUTOTUNE", "BEVBERT_LT_PLAN_BUDGET", "BEVBERT_LT_WS_MB", "BEVBERT_LT_EXHAUSTIVE", "BEVBERT_GEMM_DETERMINISTIC",
    "BEVBERT_GEMM_TABLE", "BEVBERT_TXT_PAD", "BEVBERT_PANO_PAD", "BEVBERT_VIEW_PAD", "BEVBERT_OBJ_PAD",
    "BEVBERT_REDUCE_TEXT_LAYERS", "BEVBERT_LIBHDF5")


def test_package_sources_read_only_the_listed_switches():
    """What ATTN_KNOBS is to the attention sources, PACKAGE_KNOBS is to everything else: the quoted BEVBERT_* names in the
    package's Python modules and in the HIP sources the attention test does not cover are exactly that tuple, and README.md's
    environment table has a row for each.  A switch added without both, or left behind by a retired path, fails here."""
    pkg = os.path.dirname(lib.__file__)
    csrc = os.path.join(pkg, "csrc")
    paths = [os.path.join(pkg, f) for f in sorted(os.listdir(pkg)) if f.endswith(".py")]
    paths += [os.path.join(csrc, f) for f in sorted(os.listdir(csrc))
              if f.endswith((".hip", ".h")) and not re.fullmatch(r"attn_\w+\.(hip|h)|capi\.hip", f)]
    assert len(paths) >= 50, paths
    found = {}
    for path in paths:
        with open(path) as f:
            for name in re.findall(r'"(BEVBERT_[A-Z0-9_]+)"', f.read()):
                found.setdefault(name, os.path.basename(path))
    assert len(set(PACKAGE_KNOBS)) == len(PACKAGE_KNOBS) and not set(PACKAGE_KNOBS) & set(ATTN_KNOBS)
    assert set(found) == set(PACKAGE_KNOBS), sorted((n, found.get(n)) for n in set(found) ^ set(PACKAGE_KNOBS))
    with open(os.path.join(os.path.dirname(pkg), "README.md")) as f:
        table = [line for line in f if line.lstrip().startswith("|")]
    for name in PACKAGE_KNOBS:
        assert any(f"`{name}`" in line for line in table), f"README.md's environment table has no row for {name}"


def attn_plan(l, row, ncu, monkeypatch):
    """(forward, backward) kernel names bevbert_attn_plan gives a row of ATTN_PLAN_ROWS under the row's knobs."""
    B, Lq, Lk, dtype, impl, bias, p, bits, env = row[:9]
    for name in ATTN_KNOBS:
        monkeypatch.delenv(name, raising=False)
    for name, value in env.items():
        monkeypatch.setenv(name, value)
    code = lib.BF16 if dtype == "bf16" else lib.F32
    return tuple(l.bevbert_attn_plan(B, 12, Lq, Lk, code, impl, 0, int(bias), p, int(bits != "none"), int(bits == "ready"),
                                     int(bias), ncu, backward).decode() for backward in (0, 1))


def test_attention_dispatch_plan_table(monkeypatch):
    l = lib.load()
    for row in ATTN_PLAN_ROWS:
        assert attn_plan(l, row, 256, monkeypatch) == (_A + row[9], _A + row[10]), row
    # the occupancy rule of the persistent forward follows the CU count it is handed: 768 items are 2.4 rounds of 320 CUs
    # (80 % full) and six full rounds of 128
    bev = ATTN_PLAN_ROWS[8]
    assert attn_plan(l, bev, 320, monkeypatch)[0] == "attn_fwd2" and attn_plan(l, bev, 128, monkeypatch)[0] == "attn_fwd4"
    assert l.bevbert_attn_plan(2, 12, 80, 80, lib.F32, 2, 0, 0, 0.0, 0, 0, 0, 256, 0) == b""      # rejected by the calls too
    # the keep-bit planner's question, against the expression ops_attention.py used to carry
    lens = (1, 17, 36, 80, 96, 97, 128, 181, 182, 256, 257, 441, 448, 600)
    for small in (None, "0", "1"):
        if small is None:
            monkeypatch.delenv("BEVBERT_ATTN_SMALL", raising=False)
        else:
            monkeypatch.setenv("BEVBERT_ATTN_SMALL", small)
        for Lq in lens:
            for Lk in lens:
                for has_bias in (False, True):
                    old = (Lq * Lk >= 32768 or Lk > 256) and not (Lk <= 96 and not has_bias and small == "1")
                    assert l.bevbert_attn_bits_ahead(Lq, Lk, int(has_bias)) == int(old), (Lq, Lk, has_bias, small)


def test_code_object_targets_gfx950_only():
    # --offloading drops the extracted code objects next to its INPUT file: work on a copy in a scratch directory so
    # that nothing lands in the package directory
    import shutil
    import tempfile
    with tempfile.TemporaryDirectory() as tmp:
        so = shutil.copy(lib.LIB_PATH, tmp)
        out = subprocess.run(["/opt/rocm/lib/llvm/bin/llvm-objdump", "--offloading", so], capture_output=True,
                             text=True, cwd=tmp).stdout
    archs = set(re.findall(r"gfx[0-9a-f]+", out))
    assert archs == {"gfx950"}, archs


def test_invalid_arguments_are_rejected_without_a_gpu():
    l = lib.load()
    # argument validation happens before any launch: bad shapes come back as -1 with a message
    rc = l.bevbert_bias_gelu_fwd(None, None, None, 4, 7, 0, None)
    assert rc == -1 and b"multiple of 4" in l.bevbert_last_error()
    rc = l.bevbert_bev_lift_bin(None, None, None, None, None, 1, 12, 64, 10.0, 21, 0.5, 0.5, None, None, None, None)
    assert rc == -1 and b"out of range" in l.bevbert_last_error()
    strides = (ctypes.c_int64 * 8)(*([768] * 8))
    rc = l.bevbert_attn_fwd(None, None, None, None, None, None, None, strides, 1, 12, 4, 4, 32, 0.125, 1, 0, 0.0, 0, 0, None, 0, None)
    assert rc == -1 and b"head_dim" in l.bevbert_last_error()
    # the fp32-residual LayerNorm has kernels for H = 256, 512, 768 and 1024 only; H <= 0 must not reach a launch
    for H in (0, -256, 1280):
        rc = l.bevbert_layernorm_res32_fwd(None, None, None, 0, None, None, None, None, None, None, None, 1, H, 1e-12,
                                           0.0, 0, 0, None)
        assert rc == -1 and b"must be 256, 512, 768 or 1024" in l.bevbert_last_error(), (H, rc)
        dy16 = ctypes.c_uint16(0)           # a non-null output gradient, so that the shape check is the one that fires
        rc = l.bevbert_layernorm_res32_bwd(ctypes.addressof(dy16), None, None, None, None, None, None, None, None, None,
                                           None, None, 1, H, 0.0, 0, 0, 0, 0, None)
        assert rc == -1 and b"must be 256, 512, 768 or 1024" in l.bevbert_last_error(), (H, rc)


def test_layernorm_width_and_dtype_dispatch_answers_without_a_gpu():
    """What the plain LayerNorm entries answer for a width or dtype they have no kernel for (rows = 1, null pointers: the
    answer comes before any launch).  The forward is instantiated for H / 256 in {1, 2, 3, 4, 6, 8}, the backward for 1..4."""
    l = lib.load()
    N = None
    entries = {
        "fwd": lambda H, dt: l.bevbert_bias_dropout_residual_layernorm_fwd(N, N, N, N, N, N, N, N, N, 1, H, 1e-12, dt, 0.0, 0, 0, N),
        "post_fwd": lambda H, dt: l.bevbert_layernorm_post_fwd(N, N, N, N, N, N, N, N, N, N, 1, H, 1e-12, dt, N),
        "embed_fwd": lambda H, dt: l.bevbert_embed_sum_layernorm_fwd(N, N, N, N, N, N, N, N, N, N, 1, 1, H, 1e-12, dt, 0.0, 0, 0, N),
        "bwd": lambda H, dt: l.bevbert_layernorm_bwd(N, N, N, N, N, N, N, N, N, N, N, 1, H, dt, 0.0, 0, 0, 0, N),
        "bwd_add": lambda H, dt: l.bevbert_layernorm_bwd_add(N, N, N, N, N, N, N, N, N, N, N, N, 1, H, dt, 0.0, 0, 0, 0, N),
    }
    for name, f in entries.items():
        bwd = name.startswith("bwd")
        for dt in (0, 1):
            rc = f(1536 if bwd else 1280, dt)
            want = b"layernorm_bwd: H=1536 unsupported" if bwd else b"H=1280 unsupported"
            assert rc == -3 and want in l.bevbert_last_error(), (name, dt, rc, l.bevbert_last_error())
            rc = f(100, dt)
            want = b"bad shape rows=1 L=1 H=100" if name == "embed_fwd" else b"multiple of 256"
            assert rc == -1 and want in l.bevbert_last_error(), (name, dt, rc, l.bevbert_last_error())
        for H in (768, 1280, 1536):       # the dtype is looked at before the width
            rc = f(H, 2)
            assert rc == -3 and b"dtype 2 unsupported" in l.bevbert_last_error(), (name, H, rc, l.bevbert_last_error())


def _dtype_answer_rows(l):
    """(entry, call(dtype), return code, message) for every launcher that picks a kernel instantiation from a runtime dtype."""
    N = None
    buf = (ctypes.c_uint8 * 64)()
    p = ctypes.addressof(buf)          # non-null wherever an entry checks a pointer before it looks at the dtype
    from vln_bevbert_amd.graph_map_dev import _GmState
    gm = _GmState(pos=p, dis=p, point=p, hops=p, visited=p, step_ids=p, B=1, N=1, V=1)
    gm.keep = buf                      # the rows' closures hold gm, gm holds the buffer its pointers name
    st = ctypes.byref(gm)
    strides = (ctypes.c_int64 * 8)(*([64] * 8))
    unsup, inval = -3, -1
    return [
        # colwise.hip
        ("colsum_any", lambda dt: l.bevbert_colsum_any(N, N, 1, 4, dt, 0, N), unsup, "colsum_any: dtype %d unsupported"),
        ("bias_gelu_fwd", lambda dt: l.bevbert_bias_gelu_fwd(N, N, N, 1, 4, dt, N), unsup, "bias_act_fwd: dtype %d unsupported"),
        ("bias_gelu_fwd C=8", lambda dt: l.bevbert_bias_gelu_fwd(N, N, N, 1, 8, dt, N), unsup, "bias_act_fwd: dtype %d unsupported"),
        ("bias_relu_fwd", lambda dt: l.bevbert_bias_relu_fwd(N, N, N, 1, 4, dt, N), unsup, "bias_act_fwd: dtype %d unsupported"),
        ("bias_gelu_bwd", lambda dt: l.bevbert_bias_gelu_bwd(N, N, N, N, N, N, 1, 4, dt, 0, N), unsup, "bias_act_bwd: dtype %d unsupported"),
        ("bias_relu_bwd", lambda dt: l.bevbert_bias_relu_bwd(N, N, N, N, N, N, 1, 4, dt, 0, N), unsup, "bias_act_bwd: dtype %d unsupported"),
        ("colsum", lambda dt: l.bevbert_colsum(N, N, N, 1, 4, dt, 0, N), unsup, "colsum: dtype %d unsupported"),
        ("colsum_partials", lambda dt: l.bevbert_colsum_partials(N, N, 1, 4, dt, N), unsup, "colsum_partials: dtype %d unsupported"),
        # gather.hip
        ("segment_wsum", lambda dt: l.bevbert_segment_wsum(N, N, N, N, N, 1, 4, dt, N), unsup, "segment_wsum: dtype %d unsupported"),
        ("rows_gather", lambda dt: l.bevbert_rows_gather(N, N, N, 1, 4, dt, N), unsup, "rows_gather: dtype %d unsupported"),
        ("rows_scatter", lambda dt: l.bevbert_rows_scatter(N, N, N, 1, 4, dt, 0, N), unsup, "rows_scatter: dtype %d unsupported"),
        ("rows_scatter +=", lambda dt: l.bevbert_rows_scatter(N, N, N, 1, 4, dt, 1, N), unsup, "rows_scatter: dtype %d unsupported"),
        ("embedding_grad", lambda dt: l.bevbert_embedding_grad(N, N, N, 1, 4, 0, dt, N), unsup, "embedding_grad: dtype %d unsupported"),
        ("embedding_grad_sliced", lambda dt: l.bevbert_embedding_grad_sliced(N, N, N, 1, 4, 1, 1, dt, N), unsup,
         "embedding_grad_sliced: dtype %d unsupported"),
        # optimizer.hip
        ("accum_partials", lambda dt: l.bevbert_accum_partials(N, N, 1, 4, dt, N), unsup, "accum_partials: dtype %d unsupported"),
        ("cast_f32", lambda dt: l.bevbert_cast_f32(N, N, 4, dt, N), unsup, "cast_f32: dst dtype %d unsupported"),
        # smallk.hip
        ("smallk_fwd", lambda dt: l.bevbert_smallk_linear_layernorm_fwd(*[N] * 11, 1, 1, 256, 1e-12, dt, N), unsup,
         "smallk_linear_layernorm_fwd: dtype %d unsupported"),
        ("smallk_bwd", lambda dt: l.bevbert_smallk_linear_layernorm_bwd(N, N, N, N, gm.pos, gm.pos, N, N, N, N, N, gm.pos, 1, 1, 256, dt, N), unsup,
         "smallk_linear_layernorm_bwd: dtype %d unsupported"),
        # sap_loss.hip
        ("sap_loss_fwd", lambda dt: l.bevbert_sap_loss_fwd(*[N] * 15, 1, 1, 1, 1, dt, N), unsup, "sap_loss: dtype %d unsupported"),
        ("sap_loss_bwd", lambda dt: l.bevbert_sap_loss_bwd(*[N] * 7, 1, 1, 1, dt, N), unsup, "sap_loss: dtype %d unsupported"),
        ("cross_entropy_fwd", lambda dt: l.bevbert_cross_entropy_fwd(N, N, N, N, 1, 4, dt, N), unsup, "cross_entropy: dtype %d unsupported"),
        ("cross_entropy_bwd", lambda dt: l.bevbert_cross_entropy_bwd(N, N, N, N, N, 1, 4, dt, N), unsup, "cross_entropy: dtype %d unsupported"),
        ("bce_rows_fwd", lambda dt: l.bevbert_bce_rows_fwd(N, N, N, N, 1, 4, dt, N), unsup, "bce_rows_fwd: dtype %d unsupported"),
        ("bce_rows_bwd", lambda dt: l.bevbert_bce_rows_bwd(N, N, N, N, N, 1, 4, dt, N), unsup, "bce_rows_bwd: dtype %d unsupported"),
        # nav_expert.hip
        ("nav_ce_fwd", lambda dt: l.bevbert_nav_ce_fwd(N, N, N, 1, 4, -100, dt, N), unsup, "nav_ce: dtype %d unsupported"),
        ("nav_ce_bwd", lambda dt: l.bevbert_nav_ce_bwd(N, N, N, N, N, 1, 4, -100, dt, N), unsup, "nav_ce: dtype %d unsupported"),
        # graph_nav.hip (a host-side state struct passes gm_check before the dtype is looked at)
        ("gm_embed_update", lambda dt: l.bevbert_gm_embed_update(st, *[N] * 8, 1, 1, 4, dt, N), unsup, "gm_embed_update: dtype %d unsupported"),
        ("gm_node_embeds", lambda dt: l.bevbert_gm_node_embeds(st, N, N, N, N, 1, 4, dt, N, N), unsup, "gm_node_embeds: dtype %d unsupported"),
        # waypoint.hip: the dtype is an argument check like the others there
        ("wp_ring_attn", lambda dt: l.bevbert_wp_ring_attn(N, N, 1, 1, 1.0, dt, N), inval, "wp_ring_attn: dtype %d unsupported"),
        ("wp_pano_inputs", lambda dt: l.bevbert_wp_pano_inputs(N, N, dt, 1, *[N] * 12), inval, "wp_pano_inputs: dtype %d unsupported"),
        # attn_simple.hip: its three launchers sit behind the dtype check of the two attention entries
        ("attn_fwd", lambda dt: l.bevbert_attn_fwd(N, N, N, N, N, N, N, strides, 1, 1, 4, 4, 64, 0.125, dt, 1, 0.0, 0, 0, N, 0, N), inval,
         "attn_fwd: dtype %d unsupported"),
        ("attn_bwd", lambda dt: l.bevbert_attn_bwd(*[N] * 13, strides, 1, 1, 4, 4, 64, 0.125, dt, 1, 0.0, 0, 0, N, N), inval,
         "attn_bwd: dtype %d unsupported"),
    ]


def test_every_dtype_dispatching_entry_answers_a_dtype_without_a_kernel_before_any_launch():
    """One row per launcher that turns a runtime dtype into a kernel instantiation: the smallest arguments that pass its
    shape checks (null pointers, one row), a dtype code it has no kernel for, and what it answers -- the code and the
    message, recorded from the library before these launchers shared one dispatch helper.  fp16 (2) is unknown to all of
    them but cast_f32, which converts to bf16 or fp16 and refuses fp32 (0) and 3."""
    l = lib.load()
    for name, call, want_rc, want_msg in _dtype_answer_rows(l):
        for dt in ((0, 3) if name == "cast_f32" else (2, 3, -1)):
            rc = call(dt)
            msg = l.bevbert_last_error().decode()
            assert rc == want_rc and want_msg % dt in msg, (name, dt, rc, msg)
    # the small-K entries refuse a width they have no kernel for before they look at the dtype
    buf = (ctypes.c_uint8 * 64)()
    N, p = None, ctypes.addressof(buf)
    for H in (100, 1280):
        rc = l.bevbert_smallk_linear_layernorm_fwd(*[N] * 11, 1, 1, H, 1e-12, 2, N)
        assert rc == -1 and f"smallk_linear_layernorm_fwd: H={H} unsupported" in l.bevbert_last_error().decode()
        rc = l.bevbert_smallk_linear_layernorm_bwd(N, N, N, N, p, p, N, N, N, N, N, p, 1, 1, H, 2, N)
        assert rc == -1 and f"smallk_linear_layernorm_bwd: H={H} unsupported" in l.bevbert_last_error().decode()
    # and every entry returns before its dtype check when there are no rows
    assert l.bevbert_colsum(N, N, N, 0, 4, 2, 0, N) == 0 and l.bevbert_rows_scatter(N, N, N, 0, 4, 2, 0, N) == 0
    assert l.bevbert_sap_loss_fwd(*[N] * 15, 0, 1, 1, 1, 2, N) == 0 and l.bevbert_nav_ce_bwd(N, N, N, N, N, 0, 4, -100, 2, N) == 0


def test_cpu_tensors_fail_loudly():
    from vln_bevbert_amd import ops
    with pytest.raises(lib.BevBertHipError):
        ops.bias_gelu(torch.zeros(4, 8), torch.zeros(8))


def test_state_dict_keys_match_the_reference():
    from vln_bevbert_amd.nav_model import GlocalTextPathNavCMT, remap_pretrain_checkpoint
    from vln_bevbert_amd.pretrain_cmt import GlocalTextPathCMTPreTraining
    ce = BevBertConfig.ce(num_l_layers=2, num_x_layers=2, num_pano_layers=1, vocab_size=1200, max_position_embeddings=128)
    for cfg, f in ((ce, "pretrain_state_dict_keys_tiny_ce.txt"),         # continuous-environment fork (bevbert_ce)
                   (BevBertConfig.tiny(), "pretrain_state_dict_keys_tiny.txt")):
        m = GlocalTextPathCMTPreTraining(cfg)
        assert {k: tuple(v.shape) for k, v in m.state_dict().items()} == read_shapes(f)
        assert m.mlm_head.predictions.decoder.weight is m.bert.embeddings.word_embeddings.weight
    nav = GlocalTextPathNavCMT(BevBertConfig.tiny())
    want = read_shapes("nav_state_dict_keys.txt")
    assert {k: tuple(v.shape) for k, v in nav.state_dict().items()} == want
    # a pre-training checkpoint maps onto the fine-tuning model the way vlnbert_init.py:39-46 does
    mapped = remap_pretrain_checkpoint({"module." + k: v for k, v in m.state_dict().items()})
    assert set(want) <= set(mapped) | {k for k in want if k.startswith("og_head")}


def test_arena_layout_and_packed_views():
    from vln_bevbert_amd.pretrain_cmt import GlocalTextPathCMTPreTraining
    cfg = BevBertConfig.tiny(num_l_layers=1, num_x_layers=1, vocab_size=300)
    m = GlocalTextPathCMTPreTraining(cfg)
    before = {k: v.clone() for k, v in m.state_dict().items()}
    arena = m.finalize("cpu", torch.float32)
    assert arena.numel % 1024 == 0 and arena.n_params == sum(p.numel() for p in m.parameters())
    for k, v in m.state_dict().items():
        assert torch.equal(v, before[k])                       # values preserved
    for n, p in m.named_parameters():
        o, k = arena.slices[n]
        assert p.data_ptr() == arena.params[o:].data_ptr() and p.main_grad.data_ptr() == arena.grads[o:].data_ptr()
    att = m.bert.lang_encoder.layer[0].attention.self
    assert att.pw.compute.shape == (2304, 768)
    assert torch.equal(att.pw.compute[768:1536], att.key.weight) and torch.equal(att.pb.compute[1536:], att.value.bias)
    x = m.bert.local_encoder.encoder.x_layers[0].visual_attention.att
    assert x.pw.compute.shape == (1536, 768) and torch.equal(x.pw.compute[768:], x.value.weight)
    # decay flags follow the reference's substring rule (optim/misc.py:14)
    for n, p in m.named_parameters():
        a, _ = arena._seg_of[n]
        assert bool(arena._flags_host[a] & 1) == (not R.no_decay_key(n)), n
    assert not R.no_decay_key("bert.img_embeddings.img_layer_norm.weight")
    # load_state_dict writes through into the arena
    sd = {k: torch.full_like(v, 0.5) for k, v in m.state_dict().items()}
    m.load_state_dict(sd)
    assert float(arena.params[: arena.slices["bert.embeddings.word_embeddings.weight"][1]].min()) == 0.5


def test_residual_stream_mode_belongs_to_the_model_not_the_process():
    """finalize() of a second model used to flip ops.RT.res32 under every model finalized earlier.  The mode is
    stored on the arena and installed at each forward entry (vilmodel.ensure_arena)."""
    from vln_bevbert_amd import ops
    from vln_bevbert_amd.pretrain_cmt import GlocalTextPathCMTPreTraining
    from vln_bevbert_amd.vilmodel import ensure_arena
    cfg = BevBertConfig.tiny(num_l_layers=1, num_x_layers=1, vocab_size=300)
    a = GlocalTextPathCMTPreTraining(cfg)
    b = GlocalTextPathCMTPreTraining(cfg)
    a.finalize("cpu", torch.float32)
    a.arena.res32 = True          # what finalize(dev, torch.bfloat16, torch.float32) stores (a bf16 arena needs the GPU's cast kernel)
    b.finalize("cpu", torch.float32)
    assert not b.arena.res32 and a.arena.res32 and not ops.RT.res32
    ensure_arena(a)
    assert ops.RT.res32
    ensure_arena(b)
    assert not ops.RT.res32
    ensure_arena(a)
    assert ops.RT.res32
    ops.RT.res32 = False
    with pytest.raises(ValueError):
        GlocalTextPathCMTPreTraining(cfg).finalize("cpu", torch.float32, torch.bfloat16)


def test_sap_fusion_index_form_equals_the_reference_loop():
    from vln_bevbert_amd.pretrain_cmt import fuse_sap_logits, sap_fusion_indices
    cfg = BevBertConfig()
    for seed in range(6):
        b = synthetic.make_batch(cfg, "sap", 5, seed=seed, ragged=True)
        B, G, K = 5, b["gmap_step_ids"].shape[1], b["bev_cand_idxs"].shape[1]
        g = torch.Generator().manual_seed(seed)
        gl = torch.randn(B, G, generator=g)
        ll = torch.randn(B, K, generator=g)
        gl = gl.masked_fill(b["gmap_visited_masks"], float("-inf"))
        gl = gl.masked_fill(~R.seq_mask(b["gmap_lens"], G), float("-inf"))
        ll[torch.rand(B, K, generator=g) < 0.2] = float("-inf")          # masked candidates propagate -inf
        cvp = [[None] + c[-1] for c in b["traj_cand_vpids"]]
        want = R.fuse_sap_logits(gl, ll, b["gmap_vpids"], b["gmap_visited_masks"], cvp)
        src, vis = sap_fusion_indices(b["gmap_vpids"], b["gmap_visited_masks"].tolist(), cvp, G, K)
        got = fuse_sap_logits(gl, ll, torch.from_numpy(src), torch.from_numpy(vis))
        assert torch.equal(torch.nan_to_num(got, neginf=-1e30), torch.nan_to_num(want, neginf=-1e30))


def test_gmap_csr_equals_the_reference_aggregation():
    cfg = BevBertConfig()
    b = synthetic.make_batch(cfg, "sap", 6, seed=3, ragged=True)
    T, V = b["traj_view_img_fts"].shape[:2]
    emb = torch.randn(T, V, 16)
    masks = R.seq_mask(b["traj_vp_view_lens"], V)
    want = R.aggregate_gmap(emb, masks, b["traj_vp_view_lens"], b["traj_step_lens"], b["traj_vpids"],
                            b["traj_cand_vpids"], b["gmap_vpids"])
    # evaluate the CSR densely on the host (the kernel itself is covered by the GPU tests)
    from vln_bevbert_amd.vilmodel import build_gmap_csr
    csr, G = build_gmap_csr(b["traj_step_lens"], b["traj_vp_view_lens"].tolist(), b["traj_vpids"],
                            b["traj_cand_vpids"], b["gmap_vpids"], V, "cpu")
    flat = emb.reshape(-1, 16)
    got = torch.zeros(csr.n_out, 16)
    rp, idx, w = csr.rowptr.tolist(), csr.idx.long(), csr.w
    for r in range(csr.n_out):
        if rp[r + 1] > rp[r]:
            got[r] = (w[rp[r]:rp[r + 1], None] * flat[idx[rp[r]:rp[r + 1]]]).sum(0)
    assert float((got.view(6, G, 16) - want).abs().max()) < 1e-5
    # transposed CSR is a true transpose
    dense = torch.zeros(csr.n_out, csr.n_src)
    for r in range(csr.n_out):
        dense[r, idx[rp[r]:rp[r + 1]]] += w[rp[r]:rp[r + 1]]
    dt = torch.zeros(csr.n_src, csr.n_out)
    trp, tidx, tw = csr.t_rowptr.tolist(), csr.t_idx.long(), csr.t_w
    for r in range(csr.n_src):
        dt[r, tidx[trp[r]:trp[r + 1]]] += tw[trp[r]:trp[r + 1]]
    assert torch.equal(dense.t(), dt)


def test_task_sampler_and_schedule_are_rank_independent():
    from vln_bevbert_amd.train import TaskSampler, warmup_linear_lr
    a, b = TaskSampler(seed=4), TaskSampler(seed=4)
    seq = [a.next() for _ in range(200)]
    assert seq == [b.next() for _ in range(200)]
    frac = {t: seq.count(t) / 200 for t in ("mlm", "sap", "masksem")}
    assert 0.3 < frac["mlm"] < 0.6 and 0.3 < frac["sap"] < 0.6 and frac["masksem"] < 0.2
    assert warmup_linear_lr(5000, 5e-5, 10000, 100000) == pytest.approx(R.warmup_linear_lr(5000, 5e-5, 10000, 100000))
    assert warmup_linear_lr(100001, 5e-5, 10000, 100000) == 1e-8


def test_synthetic_batches_are_deterministic_and_rank_distinct():
    cfg = BevBertConfig()
    a = synthetic.make_batch(cfg, "mlm", 3, seed=1000)
    b = synthetic.make_batch(cfg, "mlm", 3, seed=1000)
    c = synthetic.make_batch(cfg, "mlm", 3, seed=1001)
    assert all(torch.equal(a[k], b[k]) for k in a if torch.is_tensor(a[k]))
    assert not torch.equal(a["rgbs"], c["rgbs"])
    assert a["rgbs"].shape == (3, 12, 14, 14, 768) and a["traj_view_img_fts"].shape == (15, 36, 512)
    assert a["sems"].dtype == torch.float64 and (a["txt_labels"] != -1).any(1).all()


def test_grid_feature_store_rows_and_attach():
    """f1: batches are row numbers into a resident store; unknown viewpoints fail loudly."""
    from vln_bevbert_amd.feature_store import GridFeatureStore
    rng = np.random.default_rng(0)
    keys = [f"scan{i // 3}_vp{i}" for i in range(7)]
    rgbs = rng.standard_normal((7, 12, 14, 14, 8)).astype(np.float16)
    depths = rng.random((7, 12, 14, 14)).astype(np.float32)
    sems = rng.integers(0, 40, (7, 12, 14, 14)).astype(np.uint8)
    st = GridFeatureStore(keys, rgbs, depths, sems, "cpu")
    assert len(st) == 7 and st.P == 2352 and st.rgbs.shape == (7, 2352, 8) and st.rgbs.dtype == torch.float16
    assert st.nbytes() == 7 * (2352 * 8 * 2 + 2352 * 4 + 2352)
    rows = st.rows(["scan1_vp4", "scan0_vp0", "scan1_vp4"])
    assert rows.dtype == torch.int32 and rows.tolist() == [4, 0, 4]
    r, d, s = st.gather(rows)
    assert torch.equal(r[0], torch.from_numpy(rgbs[4].reshape(2352, 8))) and torch.equal(d[1], torch.from_numpy(depths[0]))
    assert torch.equal(s[2], torch.from_numpy(sems[4].reshape(-1)))
    b = st.attach({"rgbs": 1, "depths": 2, "sems": 3, "txt_ids": 4}, ["scan2_vp6"])
    assert set(b) == {"txt_ids", "grid_store", "grid_rows"} and b["grid_rows"].tolist() == [6]
    with pytest.raises(KeyError, match="not in the grid-feature store"):
        st.rows(["scan9_vp99"])


def test_graph_map_batch_matches_reference_graphmap():
    """f3: the batched, device-resident rollout bookkeeping (graph_map.GraphMapBatch) against the reference's
    GraphMap / FloydGraph driven through the agent's per-step updates (golden: tests/golden/graph_nav.npz)."""
    import json
    from tests.helpers import load_golden
    from vln_bevbert_amd.graph_map import GraphMapBatch
    g = load_golden("graph_nav")
    B, T, H, seed = int(g["B"]), int(g["T"]), int(g["H"]), int(g["seed"])
    steps = json.loads(str(g["steps_json"]))
    obs_all, ended_all = synthetic.make_nav_episodes(B, T, seed)
    gm = GraphMapBatch([ob["viewpoint"] for ob in obs_all[0]], H, "cpu", capacity=4)     # capacity 4: exercises growth
    gm.update_graph(obs_all[0])

    class _Store:                       # the bookkeeping only needs key -> row
        row = {f"scan{i}_e{i}_v{n}": 100 * i + n for i in range(B) for n in range(14)}
    for t in range(T):
        obs, ended, ref = obs_all[t], ended_all[t], steps[t]
        if t > 0:
            gm.update_graph(obs, ended_all[t - 1])
        gm.set_step_ids(obs, t, ended)
        avg = torch.tensor(ref["avg"]).requires_grad_(True)
        pano = torch.tensor(ref["pano"]).requires_grad_(True)
        gm.update_node_embeds(obs, [[c["viewpointId"] for c in ob["candidate"]] for ob in obs], avg, pano, ended)
        gm.remember_views(obs, [f"{ob['scan']}_{ob['viewpoint']}" for ob in obs], _Store, ended)
        nv = gm.nav_gmap_variable(obs)
        assert nv["gmap_vpids"] == ref["gmap_vpids"] and nv["no_vp_left"] == ref["no_vp_left"]
        G = nv["gmap_img_embeds"].shape[1]
        for i in range(B):
            n = len(ref["gmap_vpids"][i])
            assert nv["gmap_masks"][i].tolist() == [True] * n + [False] * (G - n)
            assert nv["gmap_step_ids"][i, :n].tolist() == ref["gmap_step_ids"][i]
            assert nv["gmap_visited_masks"][i, :n].long().tolist() == ref["gmap_visited_masks"][i]
            assert np.array_equal(nv["gmap_pos_fts"][i, :n].numpy(), np.asarray(ref["gmap_pos_fts"][i], dtype=np.float32))
            assert np.array_equal(nv["gmap_pair_dists"][i, :n, :n].numpy(),
                                  np.asarray(ref["gmap_pair_dists"][i], dtype=np.float32))
            assert float(nv["gmap_pair_dists"][i, n:].abs().sum()) == 0 and float(nv["gmap_pos_fts"][i, n:].abs().sum()) == 0
            want = torch.tensor(ref["gmap_img_embeds"][i])
            assert torch.allclose(nv["gmap_img_embeds"][i, :n].detach(), want, rtol=0, atol=1e-6)
            assert float(nv["gmap_img_embeds"][i, n:].detach().abs().sum()) == 0
            ob = obs[i]
            assert gm.gather_nodes(i, ob["viewpoint"], 1) == ref["gather_order1"][i]
            assert gm.cand_cells(ob, 21, 0.5).tolist() == ref["cand_cells"][i]
            assert gm.cand_cells_batch(obs, 21, 0.5)[i].tolist() == ref["cand_cells"][i]
            got = gm.pos_fts(i, ob["viewpoint"], [gm.eps[i].start_vp], ob["heading"], ob["elevation"])
            assert np.array_equal(got, np.asarray(ref["start_pos_fts"][i], dtype=np.float32))
            for vp, path in ref["paths"][i].items():
                assert gm.eps[i].graph.path(ob["viewpoint"], vp) == path
        # the stored embeddings stay differentiable across steps (the reference keeps graph-attached tensors)
        if t == T - 1:
            nv["gmap_img_embeds"].sum().backward()
            assert avg.grad is not None and float(avg.grad.abs().sum()) > 0


def test_feature_cache_round_trip(tmp_path):
    """f2: sharded safetensors cache of the grid features -> GridFeatureStore, whole or per split; no h5py involved."""
    from vln_bevbert_amd import feature_cache
    from vln_bevbert_amd.feature_store import GridFeatureStore
    rng = np.random.default_rng(4)
    keys = [f"s{i % 3}_vp{i}" for i in range(11)]
    rgbs = rng.standard_normal((11, 12, 196, 16)).astype(np.float16)
    depths = rng.random((11, 12, 14, 14)).astype(np.float32)
    sems = rng.integers(0, 40, (11, 12, 14, 14)).astype(np.uint8)
    n = feature_cache.write_shards(((k, rgbs[i], depths[i], sems[i]) for i, k in enumerate(keys)), str(tmp_path), shard_size=4)
    assert n == 11 and sorted(os.listdir(tmp_path)) == ["index.json"] + [f"shard_{i:05d}.safetensors" for i in range(3)]
    idx = feature_cache.read_index(str(tmp_path))
    assert idx["keys"] == keys and idx["shape"] == {"V": 12, "hw": 14, "C": 16} and idx["shard_of"][4] == 1
    direct = GridFeatureStore(keys, rgbs, depths, sems, "cpu")
    st = feature_cache.load_store(str(tmp_path), "cpu")
    assert st.row == direct.row and torch.equal(st.rgbs, direct.rgbs) and torch.equal(st.depths, direct.depths)
    assert torch.equal(st.sems, direct.sems)
    part = feature_cache.load_store(str(tmp_path), "cpu", keys=[keys[9], keys[2], keys[5]])      # e.g. one data split
    assert sorted(part.row) == sorted([keys[9], keys[2], keys[5]]) and len(part) == 3
    for k in part.row:
        assert torch.equal(part.rgbs[part.row[k]], direct.rgbs[direct.row[k]])
        assert torch.equal(part.sems[part.row[k]], direct.sems[direct.row[k]])
    with pytest.raises(KeyError, match="not in the cache"):
        feature_cache.load_store(str(tmp_path), "cpu", keys=["nope_1"])
    with pytest.raises(ValueError, match="duplicate key"):
        feature_cache.write_shards([(keys[0], rgbs[0], depths[0], sems[0])] * 2, str(tmp_path / "dup"))
    with pytest.raises((FileNotFoundError, OSError, RuntimeError)):
        feature_cache.convert_hdf5("a.hdf5", "b.hdf5", "c.hdf5", str(tmp_path / "x"))


def _reference_config_bag(tag, **extra):
    """What train_r2r.py:102-113 hands the model: an attribute bag with ONLY the keys of configs/<tag>_model.json plus
    pretrain_tasks (a set) and sem_pred_token."""
    import json
    import types
    with open(os.path.join(ROOT, "tests", "golden", "model_configs.json")) as f:
        keys = json.load(f)[tag]
    bag = types.SimpleNamespace(**keys)
    for k, v in extra.items():
        setattr(bag, k, v)
    return bag, keys


def test_models_build_from_the_reference_config_object():
    """The drop-in boundary: the reference's own configuration object constructs the models; the
    constants its JSON does not carry come from the defaults the reference hard-codes in its model code."""
    from vln_bevbert_amd.nav_model import GlocalTextPathNavCMT
    from vln_bevbert_amd.pretrain_cmt import GlocalTextPathCMTPreTraining
    bag, keys = _reference_config_bag("r2r", pretrain_tasks={"mlm", "sap", "masksem"}, sem_pred_token="cattn")
    for absent in ("bev_res", "grid_hw", "sem_classes", "grid_views", "grid_feat_size"):
        assert absent not in keys                       # the point of the test: the JSON really lacks them
    m = GlocalTextPathCMTPreTraining(bag)
    assert not hasattr(bag, "grid_hw")                  # the caller's object is left alone
    c = m.config
    assert (c.grid_hw, c.bev_res, c.sem_classes, c.grid_views, c.bev_dim, c.feat_dropout) == (14, 0.5, 40, 12, 21, 0.4)
    assert c.pretrain_tasks == {"mlm", "sap", "masksem"} and m.sem_pred_token == "cattn"
    assert {k: tuple(v.shape) for k, v in m.state_dict().items()} == read_shapes("pretrain_state_dict_keys_r2r.txt")
    # list-valued tasks and the xlm-roberta file
    bag, _ = _reference_config_bag("rxr", pretrain_tasks=["mlm", "sap"], sem_pred_token="cattn")
    bag.num_l_layers, bag.num_x_layers, bag.num_pano_layers = 1, 1, 1          # keep the CPU test light
    m = GlocalTextPathCMTPreTraining(bag)
    assert m.config.vocab_size == 250002 and not hasattr(m, "local_sem_head")
    # transformers' own class, when importable, behaves like the bag
    try:
        from transformers import PretrainedConfig
    except Exception:
        PretrainedConfig = None
    if PretrainedConfig is not None:
        pc = PretrainedConfig(**{k: v for k, v in keys.items() if k not in ("num_labels",)})
        pc.num_l_layers, pc.num_x_layers, pc.num_pano_layers, pc.vocab_size = 1, 1, 1, 500
        pc.pretrain_tasks, pc.sem_pred_token = {"mlm", "sap", "masksem"}, "cattn"
        assert GlocalTextPathCMTPreTraining(pc).config.bev_res == 0.5
        # fine-tune side: vlnbert_init.py:57-76 sets these by hand on the PretrainedConfig
        pc.fix_lang_embedding = pc.fix_pano_embedding = pc.fix_local_branch = False
        assert GlocalTextPathNavCMT(pc).config.grid_hw == 14


def test_remapped_pretrain_checkpoint_loads_strictly():
    from vln_bevbert_amd.nav_model import GlocalTextPathNavCMT, remap_pretrain_checkpoint
    from vln_bevbert_amd.pretrain_cmt import GlocalTextPathCMTPreTraining
    cfg = BevBertConfig.tiny(num_l_layers=1, num_x_layers=1, vocab_size=300)
    pre = GlocalTextPathCMTPreTraining(cfg)
    nav = GlocalTextPathNavCMT(cfg)
    mapped, missing, unexpected = remap_pretrain_checkpoint({"module." + k: v for k, v in pre.state_dict().items()}, nav)
    assert missing == []
    assert unexpected and all(k.startswith(("mlm_head.", "local_sem_head.")) for k in unexpected)
    nav.load_state_dict(mapped, strict=True)
    assert torch.equal(nav.global_sap_head.net[0].weight, pre.global_sap_head.net[0].weight)


def test_entry_script_calls_from_pretrained_and_set_dropout_work_unchanged():
    """train_r2r.py:153-157: ``model_class.from_pretrained(None, config=, state_dict=)`` then the loop's own
    ``set_dropout(model, p)`` (utils/misc.py:19-25, restated here), which only knows ``nn.Dropout`` modules."""
    from vln_bevbert_amd.nav_model import GlocalTextPathNavCMT, VLNBert
    from vln_bevbert_amd.pretrain_cmt import GlocalTextPathCMTPreTraining
    cfg = BevBertConfig.tiny(num_l_layers=1, num_x_layers=1, vocab_size=300)
    src = GlocalTextPathCMTPreTraining(cfg)
    sd = {k: v.clone() for k, v in src.state_dict().items()}
    sd["cls.seq_relationship.weight"] = torch.zeros(2, 8)         # what a BERT checkpoint carries in excess
    del sd["bert.embeddings.LayerNorm.weight"]
    m = GlocalTextPathCMTPreTraining.from_pretrained(pretrained_model_name_or_path=None, config=cfg, state_dict=sd)
    assert m.load_report == {"missing_keys": ["bert.embeddings.LayerNorm.weight"],
                             "unexpected_keys": ["cls.seq_relationship.weight"]}
    assert not m.training                                           # transformers returns the model in eval mode
    assert m.mlm_head.predictions.decoder.weight is m.bert.embeddings.word_embeddings.weight
    assert torch.equal(m.global_sap_head.net[0].weight, src.global_sap_head.net[0].weight)
    sd["bert.embeddings.word_embeddings.weight"] = torch.zeros(3, 3)
    with pytest.raises(RuntimeError, match="size mismatch"):
        GlocalTextPathCMTPreTraining.from_pretrained(None, config=cfg, state_dict=sd)
    assert isinstance(GlocalTextPathNavCMT.from_pretrained(None, config=cfg, state_dict={}), GlocalTextPathNavCMT)

    def set_dropout(model, drop_p):
        for _, module in model.named_modules():
            if isinstance(module, torch.nn.Dropout) and module.p != drop_p:
                module.p = drop_p

    assert not [k for k in m.state_dict() if "drop" in k]           # the holders add no checkpoint keys
    layer = m.bert.img_embeddings.pano_encoder.layers[0]
    set_dropout(m, 0.3)
    assert m.feat_dropout == 0.3 and m.bert.embeddings.dropout_p == 0.3 and layer.drop_p == 0.3
    assert m.bert.lang_encoder.layer[0].attention.self.drop_p == 0.3
    assert layer.attn_drop_p == cfg.hidden_dropout_prob             # nn.MultiheadAttention's float stays, as there
    m.set_dropout(0.0)
    assert layer.attn_drop_p == 0.0 and m.feat_dropout == 0.0
    nav = VLNBert(cfg, feat_dropout=0.4)
    set_dropout(nav, 0.5)
    assert nav.feat_dropout == 0.5


def test_static_batch_host_side_and_in_place_refill():
    """static_step.StaticBatch on the CPU: the loader-built index tensors equal what the model would build inside its
    forward, padded row counts carry zero weight, and load() rewrites the same buffers."""
    from vln_bevbert_amd.pretrain_cmt import sap_fusion_indices
    from vln_bevbert_amd.static_step import GMAP_PAD, MLM_ROW_PAD, SEM_ROW_PAD, StaticBatch
    from vln_bevbert_amd.vilmodel import build_gmap_csr
    cfg = BevBertConfig.tiny()
    b1 = synthetic.make_batch(cfg, "sap", 4, seed=5, sems_as="ids")
    b2 = synthetic.make_batch(cfg, "sap", 4, seed=6, sems_as="ids")
    sb = StaticBatch(cfg, "sap", b1, "cpu")
    G0 = int(b1["gmap_lens"].max())
    G = sb.tensors["gmap_step_ids"].shape[1]
    assert G % GMAP_PAD == 0 and G0 <= G < G0 + GMAP_PAD and sb.tensors["gmap_pair_dists"].shape == (4, G, G)
    assert torch.equal(sb.tensors["gmap_pair_dists"][:, :G0, :G0], b1["gmap_pair_dists"])
    src, vis_c = sap_fusion_indices(b1["gmap_vpids"], b1["gmap_visited_masks"].tolist(),
                                    [[None] + c[-1] for c in b1["traj_cand_vpids"]], G0, b1["bev_cand_idxs"].shape[1])
    st = sb.tensors["_static"]
    assert np.array_equal(st["sap_src"].numpy()[:, :G0], src) and np.array_equal(st["sap_vis_c"].numpy(), vis_c)
    assert (st["sap_src"].numpy()[:, G0:] == b1["bev_cand_idxs"].shape[1] + 1).all()      # padding reads the zero slot
    ref_csr, _ = build_gmap_csr(list(b1["traj_step_lens"]), b1["traj_vp_view_lens"].tolist(), b1["traj_vpids"],
                                b1["traj_cand_vpids"], b1["gmap_vpids"], 36, "cpu", G=G)
    csr = sb.tensors["gmap_csr"][0]
    n = ref_csr.idx.numel()
    assert torch.equal(csr.rowptr, ref_csr.rowptr) and torch.equal(csr.idx[:n], ref_csr.idx) and csr.capacity >= n
    # round 5: the panorama axis is padded to a multiple of PANO_PAD with dummy panoramas of one zero view -- source rows
    # behind the real ones that no segment points at (empty rows of the transposed CSR)
    from vln_bevbert_amd.static_step import PANO_PAD
    nr = ref_csr.t_rowptr.numel()
    assert torch.equal(csr.t_rowptr[:nr], ref_csr.t_rowptr) and bool((csr.t_rowptr[nr:] == ref_csr.t_rowptr[-1]).all())
    assert torch.equal(csr.t_idx[:n], ref_csr.t_idx)
    T0 = b1["traj_view_img_fts"].shape[0]
    Tp = sb.tensors["traj_view_img_fts"].shape[0]
    assert Tp % PANO_PAD == 0 and T0 <= Tp < T0 + PANO_PAD and csr.n_src == Tp * 36
    assert torch.equal(sb.tensors["traj_view_img_fts"][:T0], b1["traj_view_img_fts"]) and not sb.tensors["traj_view_img_fts"][T0:].any()
    assert torch.equal(sb.tensors["traj_vp_view_lens"][:T0], b1["traj_vp_view_lens"]) and bool((sb.tensors["traj_vp_view_lens"][T0:] == 1).all())
    # refill in place: same buffers, the other batch's content
    ptrs = {k: v.data_ptr() for k, v in sb.tensors.items() if torch.is_tensor(v) and not k.endswith("_cpu")}
    assert StaticBatch(cfg, "sap", b2, "cpu").signature == sb.signature
    sb.load(b2)
    assert all(sb.tensors[k].data_ptr() == p for k, p in ptrs.items())
    fresh = StaticBatch(cfg, "sap", b2, "cpu")
    for k, v in fresh.tensors.items():
        if torch.is_tensor(v):
            assert torch.equal(sb.tensors[k], v), k
    assert torch.equal(sb.tensors["_static"]["sap_src"], fresh.tensors["_static"]["sap_src"])
    assert torch.equal(sb.tensors["gmap_csr"][0].rowptr, fresh.tensors["gmap_csr"][0].rowptr)
    # a different bucket is refused
    with pytest.raises(ValueError):
        sb.load(synthetic.make_batch(cfg, "sap", 3, seed=6, sems_as="ids"))
    # MLM: masked positions padded to a multiple of MLM_ROW_PAD with zero-weight rows
    bm = synthetic.make_batch(cfg, "mlm", 4, seed=7, sems_as="ids")
    sm = StaticBatch(cfg, "mlm", bm, "cpu").tensors["_static"]
    lab = bm["txt_labels"].reshape(-1)
    pos = torch.nonzero(lab != -1).squeeze(1)
    assert sm["mlm_n"] == pos.numel() and sm["mlm_pos"].numel() % MLM_ROW_PAD == 0
    assert torch.equal(sm["mlm_pos"][:sm["mlm_n"]], pos) and torch.equal(sm["mlm_targets"][:sm["mlm_n"]], lab[pos])
    assert float(sm["mlm_valid"].sum()) == sm["mlm_n"] and float(sm["mlm_n_dev"]) == sm["mlm_n"]
    # MaskSEM: the row capacity bounds the number of supervised cells from above
    bs = synthetic.make_batch(cfg, "masksem", 4, seed=8, sems_as="ids")
    cap = StaticBatch(cfg, "masksem", bs, "cpu").tensors["_static"]["sem_cap"]
    assert cap % SEM_ROW_PAD == 0 and cap >= int(bs["bev_mrc_masks"].sum())


HDF5_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "hdf5")
H5PY_PYTHON = "/opt/conda/bin/python3.9"          # the image's only interpreter with h5py (3.3.0 / HDF5 1.10.6)


def _hdf5_expected():
    rb = np.load(os.path.join(HDF5_DIR, "readback.npz"))
    keys = [str(k) for k in rb["rgb/keys"]]
    assert keys == sorted(keys) and len(keys) == 5
    return rb, keys


@pytest.mark.parametrize("backend", ["libhdf5", "auto"])
def test_hdf5_files_written_like_the_reference_are_read_bit_for_bit(backend):
    """f2, real files: tests/golden/hdf5/*.hdf5 were written by h5py with the reference's own create_dataset calls
    (grid_mp3d_clip.py:180 float16 + gzip, grid_depth.py:131 native float32 / float64, grid_sem.py:155 uint8 + gzip;
    tests/golden/make_hdf5_fixtures.py) and read back by h5py into readback.npz.  hdf5_reader (libhdf5 through ctypes; h5py
    itself where importable) must list the same keys in the same order and return the same dtypes and bits."""
    from vln_bevbert_amd import hdf5_reader
    if hdf5_reader.backend() is None:
        pytest.skip("neither h5py nor a loadable libhdf5 on this machine")
    if backend == "libhdf5":
        try:
            hdf5_reader._lib()
        except hdf5_reader.Hdf5Error as e:
            pytest.skip(str(e))
    rb, keys = _hdf5_expected()
    want_dtype = {"rgb": {np.dtype("float16")}, "depth": {np.dtype("float32"), np.dtype("float64")}, "sem": {np.dtype("uint8")}}
    for name in ("rgb", "depth", "sem"):
        with hdf5_reader.open_file(os.path.join(HDF5_DIR, name + ".hdf5"), prefer=None if backend == "auto" else backend) as f:
            assert list(f.keys()) == keys and keys[2] in f and "scan9_none" not in f
            seen = set()
            for k in keys:
                d = f[k]
                a, r = d[...], rb[f"{name}/{k}"]
                assert tuple(d.shape) == r.shape and a.dtype == r.dtype and a.tobytes() == r.tobytes(), (name, k)
                seen.add(a.dtype)
            assert seen == want_dtype[name]
    with pytest.raises((FileNotFoundError, OSError)):
        hdf5_reader.open_file(os.path.join(HDF5_DIR, "missing.hdf5"), prefer=None if backend == "auto" else backend)
    if backend == "libhdf5":
        with pytest.raises(hdf5_reader.Hdf5Error, match="not an HDF5 file"):
            hdf5_reader.open_file(os.path.join(HDF5_DIR, "readback.npz"), prefer="libhdf5")
        with hdf5_reader.open_file(os.path.join(HDF5_DIR, "sem.hdf5"), prefer="libhdf5") as f, pytest.raises(KeyError):
            f["scan9_none"]


def test_hdf5_converter_on_real_files(tmp_path):
    """f2: feature_cache.convert_hdf5 on the real HDF5 fixtures -> sharded cache -> GridFeatureStore: keys in the files'
    order, fp16 features as stored, depths as float32 (map_nav_src/utils/data.py:14,25: .astype(np.float32)), class ids
    as stored; a viewpoint missing from the depth file is an error, not a silent skip."""
    from vln_bevbert_amd import feature_cache, hdf5_reader
    if hdf5_reader.backend() is None:
        pytest.skip("neither h5py nor a loadable libhdf5 on this machine")
    rb, keys = _hdf5_expected()
    paths = [os.path.join(HDF5_DIR, n + ".hdf5") for n in ("rgb", "depth", "sem")]
    out = str(tmp_path / "cache")
    assert feature_cache.convert_hdf5(*paths, out, shard_size=2) == len(keys)
    idx = feature_cache.read_index(out)
    assert idx["keys"] == keys and max(idx["shard_of"]) == 2 and idx["shape"] == {"V": 12, "hw": 14, "C": 6}
    store = feature_cache.load_store(out, "cpu")
    for k in keys:
        r = store.rows([k]).long()
        assert store.rgbs[r][0].numpy().tobytes() == rb[f"rgb/{k}"].reshape(2352, 6).tobytes()
        assert torch.equal(store.depths[r][0], torch.from_numpy(rb[f"depth/{k}"].astype(np.float32)))
        assert torch.equal(store.sems[r][0], torch.from_numpy(rb[f"sem/{k}"].reshape(2352)))
    short = _one_key_short(rb, keys)
    with pytest.raises(KeyError, match="missing from the depth file"):
        feature_cache.convert_hdf5(*paths, str(tmp_path / "bad"),
                                   reader=lambda path: short if path == paths[1] else hdf5_reader.open_file(path))


def _one_key_short(rb, keys):
    """A depth 'file' that lacks the last viewpoint: the converter only needs keys() / in / [key][...] of it."""
    class Short(dict):
        def __enter__(self):
            return self

        def __exit__(self, *a):
            return False
    return Short({k: {Ellipsis: rb[f"depth/{k}"]} for k in keys[:-1]})


def test_hdf5_fixtures_are_what_the_committed_script_writes(tmp_path):
    """The fixtures are data made by tests/golden/make_hdf5_fixtures.py: where the image's h5py interpreter exists, run the
    script again and compare what h5py reads back from the fresh files with the committed readback.npz."""
    import subprocess
    if not os.path.exists(H5PY_PYTHON):
        pytest.skip("no interpreter with h5py on this machine")
    script = os.path.join(os.path.dirname(HDF5_DIR), "make_hdf5_fixtures.py")
    p = subprocess.run([H5PY_PYTHON, script, str(tmp_path)], capture_output=True, text=True, timeout=120)
    if p.returncode != 0 and "No module named" in p.stderr:
        pytest.skip("that interpreter has no h5py / numpy")
    assert p.returncode == 0, p.stderr[-400:]
    rb, keys = _hdf5_expected()
    fresh = np.load(str(tmp_path / "readback.npz"))
    assert sorted(fresh.files) == sorted(rb.files)
    for k in rb.files:
        assert fresh[k].dtype == rb[k].dtype and fresh[k].tobytes() == rb[k].tobytes(), k


def test_text_layer_regions_partition_the_text_encoder():
    """train.PretrainTrainer.text_layer_regions: the arena regions that go out during the text encoder's backward are
    adjacent, ordered from the last hooked layer down, end where the text encoder ends, and stay below the map encoders
    (whose region is phase A)."""
    from vln_bevbert_amd.pretrain_cmt import GlocalTextPathCMTPreTraining
    from vln_bevbert_amd.train import PretrainTrainer
    cfg = BevBertConfig.tiny(num_l_layers=6, num_x_layers=1, vocab_size=300)
    model = GlocalTextPathCMTPreTraining(cfg)
    arena = model.finalize("cpu", torch.float32)
    first_map = min(o for n, (o, k) in arena.slices.items()
                    if n.startswith("bert.local_encoder") or n.startswith("bert.global_encoder") or not n.startswith("bert."))
    text_end = max(o + k for n, (o, k) in arena.slices.items() if n.startswith("bert.lang_encoder."))
    auto = PretrainTrainer.text_layer_regions(model, arena, "auto")
    assert [k for k, _, _ in auto] == [4, 2]
    for spec, want in (("auto", [4, 2]), ("1,3,5", [5, 3, 1]), ("", []), ("0,6,9", [])):
        regs = PretrainTrainer.text_layer_regions(model, arena, spec)
        assert [k for k, _, _ in regs] == want
        hi = text_end
        for k, lo, h in regs:
            assert h == hi and lo < h <= first_map
            assert lo == min(o for n, (o, _) in arena.slices.items() if n.startswith(f"bert.lang_encoder.layer.{k}."))
            hi = lo


def test_map_layer_regions_hold_only_their_own_tensors():
    """the 'heads' region goes out from the first x-layer hook and each x-layer region from its own hook; no
    region of the shipped configs may contain a tensor whose gradient is final later (any bert.* tensor inside the heads
    span, a foreign tensor inside an x-layer run), and a layout that violates it drops the region to the catch-all."""
    from vln_bevbert_amd.pretrain_cmt import GlocalTextPathCMTPreTraining
    from vln_bevbert_amd.train import PretrainTrainer
    for cfg in (BevBertConfig.tiny(num_l_layers=2, num_x_layers=3, vocab_size=300), BevBertConfig.tiny(num_l_layers=1, num_x_layers=2, vocab_size=300)):
        model = GlocalTextPathCMTPreTraining(cfg)
        arena = model.finalize("cpu", torch.float32)
        regs = PretrainTrainer.map_layer_regions(model, arena)
        assert "heads" in regs and any(isinstance(k, tuple) for k in regs)
        lo, hi = regs["heads"]
        inside = [n for n, (o, c) in arena.slices.items() if lo <= o < hi]
        assert inside and not any(n.startswith("bert.") for n in inside)
        for key, (lo, hi) in regs.items():
            if key == "heads":
                continue
            enc, k = key
            pre = f"bert.{enc}_encoder.encoder.x_layers.{k}."
            assert all(n.startswith(pre) for n, (o, c) in arena.slices.items() if lo <= o < hi), key
        # a head registered in front of the encoder stack: the span would cover bert.* -> no heads region
        slices = dict(arena.slices)
        name = next(n for n in slices if not n.startswith("bert."))
        first_bert = min(o for n, (o, c) in slices.items() if n.startswith("bert."))
        fake = type("A", (), {"slices": {**{n: (o + 4096, c) for n, (o, c) in slices.items() if n != name}, name: (first_bert, slices[name][1])}})()
        assert "heads" not in PretrainTrainer.map_layer_regions(model, fake)


def test_graph_map_hop_counts_equal_the_recursive_path_lengths():
    """GraphMapBatch.hops() (bottom-up over the next-hop tables, all pairs of the whole batch at once) against
    len(path(x, y)) of the reference's recursion, after every update of a rollout; nodes out of each other's reach and
    x == y included."""
    from vln_bevbert_amd.graph_map import GraphMapBatch
    B, T = 6, 7
    obs_all, ended_all = synthetic.make_nav_episodes(B, T, seed=5, n_nodes=12)
    gm = GraphMapBatch([ob["viewpoint"] for ob in obs_all[0]], 8, "cpu", node_capacity=4)      # capacity 4: growth
    for t in range(T):
        gm.update_graph(obs_all[t], None if t == 0 else ended_all[t - 1])
        L = gm.hops()
        for b in range(B):
            names = gm.eps[b].names
            for i, x in enumerate(names):
                for j, y in enumerate(names):
                    assert L[b, i, j] == len(gm.eps[b].path(x, y)), (t, b, x, y)


def test_bucket_manager_keeps_shape_buckets_lru_and_round_robins_buffer_sets():
    """loader.BucketManager on the CPU (no streams): one bucket per shape signature, ``depth`` buffer sets per bucket
    allocated on first use and then refilled in turn, least-recently-used bucket evicted beyond ``max_buckets``."""
    from vln_bevbert_amd.loader import BucketManager
    from vln_bevbert_amd.static_step import StaticBatch
    cfg = BevBertConfig.tiny(num_l_layers=1, num_x_layers=1, vocab_size=400)
    mgr = BucketManager(cfg, "cpu", depth=2, max_buckets=2)
    b = [synthetic.make_batch(cfg, "sap", 2, seed=40 + i, sems_as="ids") for i in range(3)]
    s0 = mgr.acquire("sap", b[0])
    s1 = mgr.acquire("sap", b[0])
    assert s0.in_use and s1.in_use
    mgr.release(s0)
    s2 = mgr.acquire("sap", b[0])
    assert s0 is not s1 and s2 is s0 and mgr.stats["buffer_sets_allocated"] == 2 and mgr.stats["refills"] == 1
    assert torch.equal(s2.tensors["txt_ids"], b[0]["txt_ids"])
    mgr.release(s1)
    mgr.release(s2)
    sigs = {StaticBatch.plan(cfg, "sap", x)["signature"] for x in b}
    ragged = [synthetic.make_batch(cfg, "sap", 2, seed=90 + i, ragged=True, sems_as="ids") for i in range(6)]
    for x in ragged:
        mgr.release(mgr.acquire("sap", x))
    assert len(mgr.buckets) <= 2
    assert mgr.stats["buckets_created"] - mgr.stats["buckets_evicted"] == len(mgr.buckets)
    assert len(sigs) >= 1


def test_bucket_manager_never_refills_a_buffer_set_the_consumer_still_holds():
    """with depth 2 and one queued batch THREE batches are in flight; a single-task stream (every batch
    in one bucket -- the common case under the reference's random task draw) must not have batch k+2 written into the
    buffers of batch k while the consumer still holds k.  The consumer here holds every batch for a while, then checks
    that the buffers and the host-side fields still are that batch's."""
    import threading
    import time
    from vln_bevbert_amd.loader import BucketManager, StreamingLoader
    cfg = BevBertConfig.tiny(num_l_layers=1, num_x_layers=1, vocab_size=400)
    base = synthetic.make_batch(cfg, "mlm", 2, seed=7, sems_as="ids")
    batches = []
    for i in range(8):          # one shape bucket, distinguishable contents
        b = dict(base)
        b["txt_ids"] = base["txt_ids"].clone()
        b["txt_ids"][:, 1] = 100 + i
        batches.append(b)
    mgr = BucketManager(cfg, "cpu", depth=2, max_buckets=4)
    loader = StreamingLoader((("mlm", b) for b in batches), mgr, prefetch=1)
    seen = 0
    for i, (task, sb) in enumerate(loader):
        time.sleep(0.05)                              # the producer has time to run ahead as far as it may
        assert int(sb.tensors["txt_ids"][0, 1]) == 100 + i, (i, sb.tensors["txt_ids"][0, :3])
        assert sb.in_use
        loader.release(sb)
        seen += 1
    assert seen == len(batches) and len(mgr.buckets) == 1
    assert mgr.stats["buffer_sets_allocated"] == 2 and mgr.stats["refills"] == len(batches) - 2
    # a consumer that forgets to release: the producer reports it instead of overwriting or hanging silently
    mgr2 = BucketManager(cfg, "cpu", depth=2, max_buckets=4)
    mgr2.WAIT_TIMEOUT_S = 0.5
    mgr2.acquire("mlm", batches[0]); mgr2.acquire("mlm", batches[1])
    with pytest.raises(RuntimeError, match="never released"):
        mgr2.acquire("mlm", batches[2])


def test_streaming_loader_close_wakes_a_producer_that_waits_for_an_unreleased_set():
    """a consumer that stops early WITHOUT releasing what it holds (it raised, or broke out of its loop) leaves
    the producer waiting for that buffer set; close() must end that wait at once (not after the two-minute timeout of the
    wait), release what is still queued and leave no error behind."""
    import time
    from vln_bevbert_amd.loader import BucketManager, StreamingLoader
    cfg = BevBertConfig.tiny(num_l_layers=1, num_x_layers=1, vocab_size=400)
    base = synthetic.make_batch(cfg, "mlm", 2, seed=7, sems_as="ids")
    mgr = BucketManager(cfg, "cpu", depth=2, max_buckets=4)
    loader = StreamingLoader((("mlm", dict(base)) for _ in range(8)), mgr, prefetch=1)
    it = iter(loader)
    held = [next(it), next(it)]                       # both buffer sets of the bucket, never released
    time.sleep(0.3)                                   # the producer now waits for a set to come free
    t0 = time.perf_counter()
    loader.close()
    assert time.perf_counter() - t0 < 5.0
    assert not loader.thread.is_alive() and loader.error is None
    assert all(sb.in_use for _, sb in held)           # what the consumer holds is still the consumer's


def test_two_loaders_on_one_bucket_manager_both_deliver_every_batch():
    """the manager owns the shape buckets and their captured graphs, so it is reused across epochs.
    close() of the first loader used to leave ``manager.stopped`` set for good; the second loader's producer then ended at
    its first ordinary back-pressure wait and the stream finished early with ``error is None`` (2 of 8 batches).  The stop
    flag now belongs to the loader; a manager that WAS shut down surfaces as an error, never as a short epoch."""
    import time
    from vln_bevbert_amd.loader import BucketManager, LoaderStopped, StreamingLoader
    cfg = BevBertConfig.tiny(num_l_layers=1, num_x_layers=1, vocab_size=400)
    base = synthetic.make_batch(cfg, "mlm", 2, seed=7, sems_as="ids")
    mgr = BucketManager(cfg, "cpu", depth=2, max_buckets=4)
    for epoch in range(3):
        loader = StreamingLoader((("mlm", dict(base)) for _ in range(8)), mgr, prefetch=1)
        n = 0
        for task, sb in loader:
            time.sleep(0.02)                          # the producer runs into back-pressure (_wait_free) every batch
            loader.release(sb)
            n += 1
        loader.close()
        assert n == 8 and loader.error is None, (epoch, n, loader.error)
    assert len(mgr.buckets) == 1 and mgr.stats["buffer_sets_allocated"] == 2      # same bucket, same buffer sets throughout
    # an early close of one loader (consumer holds a set) does not poison the next one either
    loader = StreamingLoader((("mlm", dict(base)) for _ in range(8)), mgr, prefetch=1)
    it = iter(loader)
    held = [next(it), next(it)]
    time.sleep(0.2)
    loader.close()
    for _, sb in held:
        mgr.release(sb)
    loader = StreamingLoader((("mlm", dict(base)) for _ in range(8)), mgr, prefetch=1)
    n = 0
    for task, sb in loader:
        time.sleep(0.02)
        loader.release(sb)
        n += 1
    assert n == 8
    # a manager that was shut down ends the stream with an error
    loader = StreamingLoader((("mlm", dict(base)) for _ in range(8)), mgr, prefetch=1)
    it = iter(loader)
    first = [next(it), next(it)]
    time.sleep(0.2)
    mgr.stop()
    with pytest.raises(LoaderStopped):
        for _ in it:
            pass


def test_host_feed_cpu_fallback_and_bucket_padding():
    """graph_map.HostFeed on a CPU device packs like on the GPU (without pinning): typed views of one buffer, addresses for
    kernel arguments without a view; nav_static pads the node / candidate axes to multiples of the bucket step."""
    from vln_bevbert_amd.graph_map import HostFeed
    from vln_bevbert_amd.nav_static import _pad_to
    arrays = {"a": np.arange(6, dtype=np.int64).reshape(2, 3)[:, ::2], "m": np.array([True, False]), "e": np.zeros((0, 4), np.float32)}
    out = HostFeed("cpu")(arrays)
    for k, v in arrays.items():
        assert torch.equal(out[k], torch.from_numpy(np.ascontiguousarray(v))), k
    sh = HostFeed("cpu", slots=2).ship(arrays)
    for k, v in arrays.items():
        assert (sh.ptr(k) == sh[k].data_ptr() or v.size == 0) and sh.ptr(k) % 16 == 0 and k in sh
        assert torch.equal(sh[k], torch.from_numpy(np.ascontiguousarray(v))) and sh[k].shape == v.shape
    assert HostFeed.shared("cpu") is HostFeed.shared("cpu")
    assert [_pad_to(n, 8) for n in (1, 2, 8, 9, 16, 17)] == [8, 8, 8, 16, 16, 24]


def test_nav_graph_runner_clears_stale_padding_after_a_full_width_fill():
    """fill sequence 5 -> 8 (exactly the padded width) -> 6 nodes in one bucket: rows 6..7 must be zero again
    (they are masked-out padding; stale ``gmap_masks=True`` rows there would be attended to as real nodes)."""
    from types import SimpleNamespace
    from vln_bevbert_amd.nav_static import NavGraphRunner
    runner = NavGraphRunner(SimpleNamespace(training=False, vln_bert=None), eager_uses=10 ** 9)
    seen = []
    fn = lambda x: seen.append({k: v.clone() for k, v in x.items()}) or x
    for G in (5, 8, 6, 8, 3):
        feeds = {"gmap_masks": torch.ones(2, G, dtype=torch.bool), "gmap_pair_dists": torch.full((2, G, G), float(G))}
        runner._run(("nav", 2, 8), feeds, fn, {"gmap_masks": (2, 8), "gmap_pair_dists": (2, 8, 8)})
        got = seen[-1]
        assert bool(got["gmap_masks"][:, :G].all()) and not bool(got["gmap_masks"][:, G:].any()), G
        assert float(got["gmap_pair_dists"][:, :G, :G].min()) == G
        assert float(got["gmap_pair_dists"][:, G:].abs().max() if G < 8 else 0.0) == 0.0
        assert float(got["gmap_pair_dists"][:, :, G:].abs().max() if G < 8 else 0.0) == 0.0


def test_static_inputs_fill_clears_what_a_wider_fill_left_and_only_then():
    """capture.StaticInputs.fill, the one fill routine of both navigation runners, on the object itself: the sequence of the
    runner test above, with the ``zero_`` calls counted -- none on the first fill and on a fill of the buffer's own shape,
    one when the last fill was wider."""
    from vln_bevbert_amd.capture import StaticInputs

    class Counted(torch.Tensor):
        zeroed = 0

        def zero_(self):
            Counted.zeroed += 1
            return super().zero_()

    si = StaticInputs({"gmap_masks": torch.ones(2, 5, dtype=torch.bool), "gmap_pair_dists": torch.ones(2, 5, 5)},
                      {"gmap_masks": (2, 8), "gmap_pair_dists": (2, 8, 8)})
    assert si.bufs["gmap_masks"].shape == (2, 8) and si.bufs["gmap_masks"].dtype == torch.bool
    assert si.bufs["gmap_pair_dists"].shape == (2, 8, 8) and si.bufs["gmap_pair_dists"].dtype == torch.float32
    assert not any(bool(b.any()) for b in si.bufs.values())
    si.bufs = {k: b.as_subclass(Counted) for k, b in si.bufs.items()}
    for G, zeroed in ((5, 0), (8, 0), (6, 2), (8, 0), (3, 2)):             # two buffers
        Counted.zeroed = 0
        si.fill("gmap_masks", torch.ones(2, G, dtype=torch.bool))
        si.fill("gmap_pair_dists", torch.full((2, G, G), float(G)))
        assert Counted.zeroed == zeroed, (G, Counted.zeroed)
        assert si.filled == {"gmap_masks": (2, G), "gmap_pair_dists": (2, G, G)}
        got = {k: b.as_subclass(torch.Tensor) for k, b in si.bufs.items()}
        assert bool(got["gmap_masks"][:, :G].all()) and not bool(got["gmap_masks"][:, G:].any()), G
        assert float(got["gmap_pair_dists"][:, :G, :G].min()) == G
        assert float(got["gmap_pair_dists"][:, G:].abs().max() if G < 8 else 0.0) == 0.0
        assert float(got["gmap_pair_dists"][:, :, G:].abs().max() if G < 8 else 0.0) == 0.0


@pytest.mark.parametrize("with_text", [False, True])
def test_navigation_call_pads_the_shapes_and_builds_the_keys_of_both_runners(with_text):
    """nav_static.NavGraphRunner._navigation_call, the one builder of a navigation step's feeds: B = 2, G = 5 nodes, C = 3
    candidates, L = 4 tokens, 9 BEV cells.  Node and candidate axes are padded to 8; the key is the tuple both runners have
    always built for these sizes (bucket and segment counts hang on it); the fusion table is sap_fusion_indices' own."""
    from types import SimpleNamespace
    from vln_bevbert_amd.nav_static import NavGraphRunner
    from vln_bevbert_amd.pretrain_cmt import sap_fusion_indices
    B, G, C, L, H = 2, 5, 3, 4, 6
    g = torch.Generator().manual_seed(3)
    visited = torch.tensor([[True, True, False, False, True], [True, False, False, True, False]])
    nav = {"txt_embeds": torch.randn(B, L, H, generator=g), "txt_masks": torch.ones(B, L, dtype=torch.bool),
           "gmap_img_embeds": torch.randn(B, G, H, generator=g), "gmap_step_ids": torch.randint(0, 9, (B, G), generator=g),
           "gmap_pos_fts": torch.randn(B, G, 7, generator=g), "gmap_masks": torch.ones(B, G, dtype=torch.bool),
           "gmap_pair_dists": torch.rand(B, G, G, generator=g), "gmap_visited_masks": visited,
           "gmap_visited_masks_cpu": visited.clone(), "bev_fts": torch.randn(B, 9, H, generator=g),
           "bev_pos_fts": torch.randn(B, 9, 3, generator=g), "bev_nav_masks": torch.ones(B, 9, dtype=torch.bool),
           "bev_cand_idxs": torch.randint(0, 9, (B, C), generator=g),
           "gmap_vpids": [[None, "a", "b", "c", "d"], [None, "p", "q", "r", "s"]],
           "bev_cand_vpids": [[None, "b", "d"], [None, "r", "q"]]}
    runner = NavGraphRunner(SimpleNamespace(training=False, vln_bert=None))
    feeds, shapes, key, sizes = runner._navigation_call(nav, with_text=with_text)
    assert key == (2, 8, 8, 4, 9) and sizes == (5, 3)
    assert shapes == {"gmap_img_embeds": (2, 8, 6), "gmap_step_ids": (2, 8), "gmap_pos_fts": (2, 8, 7), "gmap_masks": (2, 8),
                      "gmap_pair_dists": (2, 8, 8), "gmap_visited_masks": (2, 8), "bev_cand_idxs": (2, 8)}
    names = ["gmap_img_embeds", "gmap_step_ids", "gmap_pos_fts", "gmap_masks", "gmap_pair_dists", "gmap_visited_masks",
             "bev_fts", "bev_pos_fts", "bev_nav_masks", "bev_cand_idxs", "src", "vis_c"]
    assert list(feeds) == (["txt_embeds", "txt_masks"] if with_text else []) + names
    assert all(feeds[k] is nav[k] for k in feeds if k not in ("src", "vis_c"))
    src, vis_c = sap_fusion_indices(nav["gmap_vpids"], visited.tolist(), nav["bev_cand_vpids"], 8, 8)
    assert src.shape == (2, 8) and vis_c.shape == (2, 8) and vis_c.any() and (src[:, 1:5] < 9).any()
    assert torch.equal(feeds["src"], torch.from_numpy(src)) and torch.equal(feeds["vis_c"], torch.from_numpy(vis_c))
    # the key each ``navigation`` method makes of it (the inference runner's bucket; the training runner's segment, in front
    # of which ``_segment`` puts the mode and the step index), and what it hands back of the padded outputs
    from vln_bevbert_amd.nav_static import NavTrainRunner
    out = {"gmap_embeds": torch.zeros(2, 8, H), "global_logits": torch.zeros(2, 8), "local_logits": torch.zeros(2, 8),
           "fused_logits": torch.zeros(2, 8)}
    seen = []
    if with_text:
        nav["txt_embeds"].requires_grad_(True)
        runner = NavTrainRunner(SimpleNamespace(training=True, vln_bert=None), None)
        runner._segment = lambda mode, key, feeds, *a: seen.append(((mode,) + key, list(feeds))) or out
        want = ("navigation", 2, 8, 8, 4, 9, ("txt_embeds",))
    else:
        runner._text_inputs = lambda *a: {}
        runner._run = lambda key, feeds, *a: seen.append((key, list(feeds))) or out
        want = ("navigation", 2, 8, 8, 4, 9)
    got = runner.navigation(nav)
    assert seen == [(want, list(feeds))]
    assert {k: v if v is None else tuple(v.shape) for k, v in got.items()} == {
        "gmap_embeds": (2, 5, H), "global_logits": (2, 5), "local_logits": (2, 3), "fused_logits": (2, 5), "obj_logits": None}


def test_device_graph_map_host_side_against_the_host_map(monkeypatch):
    """graph_map_dev.DeviceGraphMap without the device: its host half (observation digest, id -> node lookups, node order,
    what it ships to the kernels) on CPU tensors with the C-ABI launches recorded instead of run, against
    graph_map.GraphMapBatch (pinned to the reference's GraphMap by tests/golden/graph_nav.npz).  The kernels' half is
    tests/test_gpu_model.py::test_device_graph_map_equals_the_host_graph_map."""
    from vln_bevbert_amd import graph_map_dev, lib
    from vln_bevbert_amd.graph_map import GraphMapBatch
    B, T, H, n_nodes, V = 6, 9, 8, 14, 12
    calls = []
    monkeypatch.setattr(lib, "call", lambda name, *a: calls.append((name, a)))
    monkeypatch.setattr(lib, "stream", lambda: 0)

    class HostSide(graph_map_dev.DeviceGraphMap):
        def __init__(self, start_vps):
            self._setup(start_vps, H, torch.device("cpu"), torch.float32, 8, V)       # capacity 8: exercises growth

    class Store:
        hw = 14
        row = {f"scan{i}_e{i}_v{n}": i * n_nodes + n for i in range(B) for n in range(n_nodes)}
        depths = torch.zeros(B * n_nodes, V, 14, 14)
    Store.V = V
    obs_all, ended_all = synthetic.make_nav_episodes(B, T, seed=31, n_nodes=n_nodes)
    start = [ob["viewpoint"] for ob in obs_all[0]]
    host, dev = GraphMapBatch(start, H, "cpu"), HostSide(start)
    host.update_graph(obs_all[0])
    g = torch.Generator().manual_seed(0)
    saw_dead = False
    for t in range(T):
        obs, ended = obs_all[t], ended_all[t]
        keys = [f"{ob['scan']}_{ob['viewpoint']}" for ob in obs]
        avg, pano = torch.randn(B, H, generator=g), torch.randn(B, 36, H, generator=g)
        if t > 0:
            host.update_graph(obs, ended_all[t - 1])
        host.set_step_ids(obs, t, ended)
        host.remember_views(obs, keys, Store, ended)
        calls.clear()
        dev.update_graph(obs, None if t == 0 else ended_all[t - 1], step_id=t + 1, step_ended=ended,
                         store_rows=[Store.row[k] for k in keys])
        assert [c[0] for c in calls] == ["bevbert_gm_update"] and calls[0][1][10:12] == (dev._last_up[2], t + 1)
        up = dev._last_up[1]
        live_g = np.ones(B, bool) if t == 0 else ~np.asarray(ended_all[t - 1], dtype=bool)
        live_s = ~np.asarray(ended, dtype=bool)
        saw_dead |= not live_g.all()
        assert np.array_equal(up["live_g"].numpy().astype(bool), live_g) and np.array_equal(up["live_s"].numpy().astype(bool), live_s)
        assert np.array_equal(dev.n, host.n) and dev.names == [ep.names for ep in host.eps]
        nm = int(host.n.max())
        assert dev.N >= nm and np.array_equal(dev.visited_host[:, :nm], host.visited[:, :nm])
        cur, cand, nc, dist = (up[k].numpy() for k in ("cur", "cand", "ncand", "cand_dist"))
        for b in range(B):
            ep, ob = host.eps[b], obs[b]
            assert ep.names[cur[b]] == ob["viewpoint"]
            assert nc[b] == (len(ob["candidate"]) if live_g[b] else 0) and up["ncand_all"][b] == len(ob["candidate"])
            for j, c in enumerate(ob["candidate"]):
                assert ep.names[cand[b, j]] == c["viewpointId"]
                if live_g[b]:         # a direct edge is the shortest path between two viewpoints: the map holds its length
                    assert dist[b, j] == ep.distance(ob["viewpoint"], c["viewpointId"]), (t, b, j)
            if live_s[b]:
                row, Tm = ep.pc_nodes[ob["viewpoint"]]
                assert int(up["row"][b]) == row and np.array_equal(up["T"][b].numpy().reshape(V, 4, 4), Tm)
            else:
                assert int(up["row"][b]) == -1
        cand_vpids = [[c["viewpointId"] for c in ob["candidate"]] for ob in obs]
        host.update_node_embeds(obs, cand_vpids, avg, pano, ended)
        calls.clear()
        dev.update_node_embeds(obs, cand_vpids, avg, pano, ended)
        assert [c[0] for c in calls] == ["bevbert_gm_embed_update"]
        assert calls[0][1][5:9] == (up.ptr("live_s"), up.ptr("cur"), up.ptr("ncand_all"), up.ptr("cand"))   # the step record
        calls.clear()
        hn, dn = host.nav_gmap_variable(obs), dev.nav_gmap_variable(obs)
        assert [c[0] for c in calls] == ["bevbert_gm_nav_vars", "bevbert_gm_node_embeds"]
        assert dn["gmap_vpids"] == hn["gmap_vpids"] and dn["no_vp_left"] == hn["no_vp_left"]
        assert torch.equal(dn["gmap_visited_masks_cpu"], hn["gmap_visited_masks_cpu"])
        assert tuple(dn["gmap_pair_dists"].shape) == tuple(hn["gmap_pair_dists"].shape)
        calls.clear()
        hb, db = host.bev_inputs(obs, Store, pc_order=1), dev.bev_inputs(obs, Store, pc_order=1)
        assert [c[0] for c in calls] == ["bevbert_gm_bev_select", "bevbert_gm_gather_views"]
        assert tuple(db["grid_rows"].shape) == tuple(hb["grid_rows"].shape)             # the neighbour bound is tight
        assert calls[1][1][4:6] == (B * hb["grid_rows"].shape[1], V * 14 * 14 * 4)
        for k in ("T_w2c", "S_w2c", "bev_nav_masks", "bev_cand_idxs"):
            assert torch.equal(db[k], hb[k]), (t, k)
        assert db["bev_cand_vpids"] == hb["bev_cand_vpids"]
    assert saw_dead and dev.N > 8


def test_scratch_ring_continues_in_further_buffers_while_reductions_are_queued(monkeypatch):
    """ops.ScratchRing: the first buffer grows up to its size; a backward pass that queues more partial sums than that
    before its reductions are issued (the fine-tune rollout differentiates through 15 navigation steps at once) continues
    in further buffers, which later passes reuse in the same order -- the addresses repeat after reset(); with nothing
    queued the ring starts over instead; the total is bounded."""
    from vln_bevbert_amd import lib, ops
    monkeypatch.setattr(ops.ScratchRing, "INITIAL", 1024)
    ring = ops.ScratchRing(4096, max_total=3 * 4096)
    dev = torch.device("cpu")
    monkeypatch.setattr(ops.ReduceQueue, "jobs", [("queued",)])

    def one_pass(n):
        ring.reset()
        return [ring.alloc(1000, dev) for _ in range(n)]
    one_pass(4)                                          # grows 1024 -> 2048 -> 4096: the first buffer
    assert ring.ci == 0 and ring.size == 4096 and len(ring._old) == 2
    a = one_pass(10)                                     # 4 allocations (of 1024) per buffer: three buffers
    assert ring.ci == 2 and len(ring._chunks) == 3 and ring.total_bytes() == 3 * 4096
    assert len(set(a)) == 10
    for i, p in enumerate(a):                            # inside the buffer the allocation order says
        buf, base, size = ring._chunks[i // 4]
        assert base <= p and p + 1000 <= base + size
    assert one_pass(10) == a and one_pass(3) == a[:3]    # addresses repeat from pass to pass (task tables hold pointers)
    t = ring.tensor((5, 7), torch.float32, dev)
    assert t.shape == (5, 7) and t.data_ptr() == a[3]
    with pytest.raises(lib.BevBertHipError, match="BEVBERT_SCRATCH_MAX_MB"):
        one_pass(13)
    with pytest.raises(lib.BevBertHipError, match="buffer size"):
        ring.alloc(5000, dev)
    monkeypatch.setattr(ops.ReduceQueue, "jobs", [])     # nothing queued: the ring starts over rather than growing
    ring.reset()
    b = [ring.alloc(1000, dev) for _ in range(14)]
    assert b[:12] == a[:10] + b[10:12] and b[12:] == a[:2] and len(ring._chunks) == 3


def test_grad_reducer_skips_gaps_that_hold_no_tensor():
    """Round 5: regions issued from tensor borders leave the arena's alignment padding between them; a gap no tensor
    lives in is not a collective of its own, a gap with even a one-element tensor is."""
    from vln_bevbert_amd.train import GradReducer
    flat = torch.zeros(8192)
    red = GradReducer(flat, 4096)
    red.set_occupied([(0, 1000), (1024, 1), (2048, 2048), (4096, 3000), (7168, 1024)])
    red._done = [(0, 1000), (2048, 4096), (4096, 7096)]
    assert red._remaining() == [(1000, 2048), (7096, 8192)]          # [1000, 2048) holds the one-element tensor at 1024
    red._done += [(1024, 1025), (7168, 8192)]
    assert red._remaining() == []                                    # what is left is padding only
    red.occupied = None
    assert red._remaining() == [(1000, 1024), (1025, 2048), (7096, 7168)]


def test_summarize_trace_splits_a_kernel_symbol_by_problem_size(tmp_path):
    """scripts/summarize_trace.py (the per-step / per-shape view of a rocprofv3 kernel trace behind profiles/*_last_steps_*):
    keeps the last K steps (delimited by adamw_kernel), classes kernels, and splits ONE symbol launched on ONE grid into its
    duration clusters -- the 441 x 441 and 80 x 441 problems of an attention kernel share symbol and grid."""
    import subprocess
    import sys
    rows = ["Kind,Agent_Id,Queue_Id,Kernel_Name,Start_Timestamp,End_Timestamp,Workgroup_Size_X,Grid_Size_X"]
    t = 0
    for step in range(4):
        for dur, name, grid in ((160_000, "void attn_bwd3_kernel<true, false, 0>(AttnArgs)", 768 * 512),
                                (75_000, "void attn_bwd3_kernel<true, false, 0>(AttnArgs)", 768 * 512),
                                (90_000, "Cijk_Ailk_Bljk_BBS_BH_Bias_HA_S_SAV_UserArgs_MT128x128x128", 240 * 256),
                                (12_000, "void at::native::vectorized_elementwise_kernel<4>()", 1024 * 256),
                                (1_100_000, "adamw_kernel(float*, float const*)", 4096 * 256)):
            rows.append(f"KERNEL_DISPATCH,1,{1 + (name[0] == 'C')},\"{name}\",{t},{t + dur},{512 if 'attn' in name else 256},{grid}")
            t += dur + 5_000
    d = tmp_path / "trace"
    d.mkdir()
    (d / "x_kernel_trace.csv").write_text("\n".join(rows) + "\n")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = subprocess.run([sys.executable, os.path.join(root, "scripts", "summarize_trace.py"), str(d), "2"],
                         capture_output=True, text=True, check=True).stdout
    assert "last 2 steps" in out and "5 launches/step" in out
    assert "custom" in out and "gemm" in out and "torch" in out
    shape_lines = [ln for ln in out.splitlines() if "attn_bwd3_kernel" in ln and "calls/step" in ln]
    assert len(shape_lines) == 2, out                       # two problem sizes of one symbol on one grid
    assert "160.00 us avg" in shape_lines[0] and "75.00 us avg" in shape_lines[1]


def test_gpu_scripts_parse():
    """The gpurun scripts under scripts/ are only ever run on the GPU box: at least their shell syntax is checked here."""
    import glob
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    scripts = sorted(glob.glob(os.path.join(root, "scripts", "*.sh")))
    assert scripts
    for sh in scripts:
        r = subprocess.run(["bash", "-n", sh], capture_output=True, text=True)
        assert r.returncode == 0, (sh, r.stderr)
    for py in sorted(glob.glob(os.path.join(root, "scripts", "*.py"))) + [os.path.join(root, "bench.py")]:
        compile(open(py).read(), py, "exec")


def _load_bench():
    import importlib.util
    spec = importlib.util.spec_from_file_location("bench_module", os.path.join(ROOT, "bench.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_bench_contract_line_is_compact_and_carries_roofline_and_cpu_baseline():
    """Round 5's bench line was ~24 KB and the driver did not parse it (BENCH_r05.json: parsed null).  The line built
    from that recorded full record must stay under bench.LINE_LIMIT and still carry the contract fields, the roofline of
    the dominant kernel and the CPU baseline; an artificially bloated record sheds optional blocks, never contract ones."""
    import json
    bench = _load_bench()
    full = json.load(open(os.path.join(ROOT, "profiles", "r05z_bench.json")))
    assert len(json.dumps(full)) > 20000                        # the record that was not parsed
    line = bench.compact_line(full, "/x/bench_detail.json")
    text = json.dumps(line)
    assert len(text) < bench.LINE_LIMIT == 6144, len(text)
    back = json.loads(text)
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling",
              "vs_baseline", "dtype", "data", "config"):
        assert back[k] == full[k], k
    assert back["roofline"]["frac"] == full["roofline"]["frac"] and back["roofline"]["bound"] in ("hbm", "mfma")
    assert set(back["roofline"]) >= {"kernel", "bound", "achieved", "peak", "unit", "frac", "traffic", "avg_launch_us"}
    assert "entry_shapes" not in back["roofline"] and "entry_shapes" not in back["roofline_attn_fwd"]
    cb = back["cpu_baseline"]
    assert cb["value"] == full["cpu_baseline"]["value"] and cb["cores"] == 16 and cb["kind"] == "port" and cb["sample"]
    assert set(cb["forward_b2_all_cores"]) == {"sap", "mlm"}
    assert back["sustained"]["steps_eager"] == 0 and back["detail"] == "bench_detail.json"
    assert all(set(v) <= {"value", "ms_per_step", "ms_per_nav_step", "episodes_per_s", "note"} for v in back["side_configs"].values())
    # bloat: optional blocks go first, the contract fields stay
    fat = dict(full)
    fat["side_configs"] = {f"cfg{i}": {"value": 1.0, "ms_per_step": 2.0, "error": "x" * 300} for i in range(80)}
    thin = bench.compact_line(fat)
    assert len(json.dumps(thin)) < bench.LINE_LIMIT and "side_configs" not in thin
    assert thin["roofline"]["frac"] == full["roofline"]["frac"] and thin["cpu_baseline"]["value"] == cb["value"]


def test_bench_starts_its_own_ranks():
    """`python bench.py --gpus 2` without a launcher re-executes under torch.distributed.run with two ranks (VERDICT r5:
    the driver calls it that way; until round 5 it died on an assert).  --dry-launch stops each rank after it has printed
    its coordinates, so the launch logic runs here without a GPU; the torchrun form keeps working."""
    import json
    import sys
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "3", "--warmup", "1", "--dry-launch"],
                       capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, r.stderr[-2000:]
    got = sorted((json.loads(ln) for ln in r.stdout.splitlines() if ln.startswith("{")), key=lambda d: d["rank"])
    assert [(d["rank"], d["local_rank"], d["world_size"]) for d in got] == [(0, 0, 2), (1, 1, 2)], r.stdout
    assert got[0]["master"] == got[1]["master"] and got[0]["master"].startswith("127.0.0.1:")
    # a launcher whose world size disagrees with --gpus is refused with a message, not an assert
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "4", "--dry-launch"],
                       capture_output=True, text=True, timeout=120, env={**env, "WORLD_SIZE": "2", "RANK": "0", "LOCAL_RANK": "0"})
    assert r.returncode != 0 and "WORLD_SIZE=2" in r.stderr
    # one rank: no launcher involved
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--dry-launch"], capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 0 and json.loads(r.stdout.strip())["world_size"] == 1


def test_quiet_gc_takes_the_long_lived_objects_out_of_the_collectors_reach():
    """loader.quiet_gc (after warm-up): what is alive moves to the permanent generation, so a later generation-2 pass no
    longer walks the model / graphs / tables (85 ms with every thread stopped: profiles/r06x_*)."""
    import gc
    from vln_bevbert_amd.loader import quiet_gc
    assert gc.get_freeze_count() == 0
    try:
        quiet_gc()
        assert gc.get_freeze_count() > 1000 and gc.isenabled()
    finally:
        gc.unfreeze()


def test_attention_gradient_destinations_have_the_operand_strides():
    """ops_attention._grad_like: the backward kernels write dq / dk / dv with the OPERAND's strides, so the destination of a
    dense tensor, of a column slice of a packed tensor (the hoisted K|V stride) and of a row-and-column slice has exactly
    those strides and storage that covers its last element; an operand expanded over the batch is refused."""
    from vln_bevbert_amd.ops_attention import _expanded, _grad_like
    for dtype in (torch.float32, torch.bfloat16):
        parent = torch.zeros(2, 5, 24, dtype=dtype)
        for t in (parent, parent[..., 6:12], parent[..., 18:], parent[:, 1:4, 6:12], parent[1:, :, :6], parent[:1, :1, 6:12]):
            g = _grad_like(t)
            assert g.shape == t.shape and g.dtype == t.dtype and g.stride() == t.stride(), (t.stride(), g.stride())
            last = sum((n - 1) * st for n, st in zip(g.shape, g.stride()))
            assert g.storage_offset() + last < g.untyped_storage().nbytes() // g.element_size()
            g.fill_(3)                          # every element is addressable and the slices of a packed gradient are views
            assert float(g.sum()) == 3 * t.numel() and g[..., :3].data_ptr() == g.data_ptr()
    assert _expanded(torch.zeros(5, 24).expand(2, 5, 24)) and not _expanded(parent[:1, :, 6:12].expand(1, 5, 6))
    with pytest.raises(AssertionError):
        _grad_like(torch.zeros(5, 24).expand(2, 5, 24)[..., 6:12])


def test_hoisted_kv_holder_slot_is_claimed_once_and_sliced_at_the_packed_stride():
    """_KVGradHolder: the first consumer of a layer's view claims its slice of the (B, Lk, layers * width) buffer."""
    from vln_bevbert_amd.ops_gemm import _KVGradHolder
    parent = torch.zeros(2, 5, 24)
    h = _KVGradHolder(3, 6)
    assert [h.claim(1), h.claim(1), h.claim(0), h.claim(1)] == [True, False, True, False]
    assert h.grad_slice(1, parent[..., 6:12]).stride() == (3 * 6 * 5, 3 * 6, 1) and h.buf.shape == (2, 5, 18)


def test_attention_stride_block_follows_the_header_order():
    """ops_attention._strides: [ldq, ldk, ldv, ldo, bsq, bsk, bsv, bso] (include/bevbert_hip.h), every operand's own."""
    from vln_bevbert_amd.ops_attention import _strides
    q, o = torch.zeros(2, 7, 64), torch.zeros(2, 7, 64)
    k = torch.zeros(2, 5, 3 * 64)[..., 64:128]
    v = torch.zeros(2, 10, 5 * 64)[:, :5, 128:192]
    assert list(_strides(q, k, v, o)) == [64, 192, 320, 64, 7 * 64, 5 * 192, 10 * 320, 7 * 64]
    with pytest.raises(AssertionError):
        _strides(q.transpose(1, 2), k, v, o)
