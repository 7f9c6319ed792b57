"""C ABI: struct layouts agree across Python/ctypes, the oracle build and the product library;
the product library loads without a GPU and exports every symbol include/mjx355.h declares."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import mjx_amd
from mjx_amd import _lib, abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_symbols_exported():
    hdr = open(os.path.join(ROOT, "include", "mjx355.h")).read()
    declared = set(re.findall(r"^\s*(?:const char\*|long long|int|void)\s+(mjl_\w+)\(", hdr, re.M))
    assert declared == set(_lib.EXPORTS)
    L = _lib.lib()
    for name in declared:
        assert hasattr(L, name), name
    assert b"gfx950" in L.mjl_version()


def test_struct_layouts_match_oracle_build():
    import oracle as orc
    L = orc.lib()  # asserts sizeof(OrcState/ModelDesc/EnvConfig) against the C compiler
    assert L.orc_desc_size() == C.sizeof(abi.ModelDesc)
    assert L.orc_envcfg_size() == C.sizeof(abi.EnvConfigC)
    # the last field's offset: a reordering of equal-sized fields keeps sizeof and moves nothing but names,
    # a reordering of unequal ones moves this
    assert abi.ModelDesc._fields_[-1][0] == "sensor_adr" and abi.EnvConfigC._fields_[-1][0] == "obs_sign"
    assert L.orc_desc_last_offset() == abi.ModelDesc.sensor_adr.offset
    assert L.orc_envcfg_last_offset() == abi.EnvConfigC.obs_sign.offset


def test_every_export_has_its_signature():
    """No entry point is left on ctypes' defaults: argtypes are set for every function with parameters and
    count what the header declares; the non-int returns carry their restype. The header is read here with
    this test's own regex, not with the package's reader."""
    hdr = open(os.path.join(ROOT, "include", "mjx355.h")).read()
    protos = re.findall(r"^\s*(const char\*|long long|int|void)\s+(mjl_\w+)\(([^)]*)\)", hdr, re.M)
    assert [name for _, name, _ in protos] == _lib.EXPORTS  # header order
    L = _lib.lib()
    restype = {"const char*": C.c_char_p, "long long": C.c_longlong, "int": C.c_int, "void": None}
    for ret, name, args in protos:
        fn = getattr(L, name)
        nargs = 0 if args.strip() == "void" else args.count(",") + 1
        assert nargs == 0 or fn.argtypes is not None, name
        assert len(fn.argtypes or ()) == nargs, name
        assert fn.restype is restype[ret], name


def test_longest_signatures_pinned():
    """The exact argtypes of three long entry points, written out: uint64_t and int positions
    (mjl_env_step), pointer tables between scalars (mjl_adam_multi), 26 arguments (mjl_twin_head)."""
    L = _lib.lib()
    vp, i32, f32, u64 = C.c_void_p, C.c_int, C.c_float, C.c_uint64
    assert L.mjl_env_step.argtypes == [vp, vp, vp, vp, vp, vp, i32, u64, u64, vp]
    assert L.mjl_adam_multi.argtypes == [i32, vp, vp, vp, vp, vp, vp, i32, vp, f32, f32, f32, f32, vp, vp, i32, vp]
    assert L.mjl_twin_head.argtypes == [vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp,  # zh ... stats_row
                                        i32, i32, i32, f32, f32, f32, f32,  # n, A, K, clip_eps ... log_std_hi
                                        vp, vp, vp, vp, vp, vp, vp, vp]  # scratch ... biasp, stream
    assert L.mjl_model_create.argtypes == [C.POINTER(abi.ModelDesc), C.POINTER(vp)]
    assert L.mjl_env_config.argtypes == [vp, C.POINTER(abi.EnvConfigC)]


def test_header_reader_is_strict():
    """The reader accepts the header's own forms and raises on anything else, so that a construct it
    does not understand fails at import instead of leaving a function on ctypes' int default."""
    from mjx_amd._header import HeaderError, parse
    ok = parse("#define MJL_N 3\nenum { MJL_A = 0, MJL_B = 2 };\n"
               "typedef struct s { int32_t n, a[MJL_N][2]; /* c */ double x; } s;\ntypedef struct h h;\n"
               "long long mjl_f(const s* p, h** out, const float* const* w, unsigned m, void* stream);\n"
               "void mjl_g(void);\n")
    assert ok.defines == {"MJL_N": 3} and ok.enums == {"MJL_A": 0, "MJL_B": 2}
    assert ok.structs["s"] == [("n", "int32_t", ()), ("a", "int32_t", (3, 2)), ("x", "double", ())]
    assert ok.protos == [("long long", "mjl_f", ["s*", "h**", "float**", "unsigned", "void*"]), ("void", "mjl_g", [])]
    for bad in ("int mjl_foo(size_t n, void* stream);",  # unknown type
                "typedef struct s { int32_t a[MJL_NOPE]; } s;",  # array bound is an undefined macro
                "int mjl_foo(void (*cb)(int), void* stream);",  # a form the reader does not accept
                "int mjl_foo(int n)\n__attribute__((cold));",
                "#define MJL_N (1 << 3)\n",
                "enum { MJL_A, MJL_B };"):
        with pytest.raises(HeaderError):
            parse(bad)


def test_model_create_validates_without_gpu():
    L = _lib.lib()
    m = mjx_amd.load_model("humanoid_mjx")
    d = abi.model_desc(m)
    h = C.c_void_p()
    assert L.mjl_model_create(C.byref(d), C.byref(h)) == 0
    assert L.mjl_model_nefc_max(h) == 16 * 4 + 100 + 21 + 2  # nefc <= 187
    L.mjl_model_destroy(h)
    bad = abi.model_desc(m)
    bad.integrator = 1  # RK4
    assert L.mjl_model_create(C.byref(bad), C.byref(h)) == 2
    assert b"integrator" in L.mjl_last_error()


def test_no_silent_cpu_fallback():
    """Without a GPU the product path fails loudly instead of falling back to the CPU."""
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    from mjx_amd import mjx
    sys_ = mjx.put_model(mjx_amd.load_model("humanoid_mjx"))
    with pytest.raises(_lib.MjlError):
        mjx.make_data(sys_, 4)


def test_batch_create_rejects_empty_and_null_without_gpu():
    """An empty or negative batch and a null model are argument errors, reported before any device
    call (so also on a host without a GPU)."""
    L = _lib.lib()
    m = mjx_amd.load_model("humanoid_mjx")
    d = abi.model_desc(m)
    h, b = C.c_void_p(), C.c_void_p()
    assert L.mjl_model_create(C.byref(d), C.byref(h)) == 0
    for n in (0, -1):
        assert L.mjl_batch_create(h, n, 0, C.byref(b)) == 1  # MJL_ERR_ARG
        assert b"bad argument" in L.mjl_last_error()
    assert L.mjl_batch_create(None, 4, 0, C.byref(b)) == 1
    L.mjl_model_destroy(h)


def test_check_names_the_error_code():
    """check() keeps "mjx355 error <rc>" and the library's text, and names the code beside the number."""
    rc = _lib.lib().mjl_batch_create(None, 4, 0, C.byref(C.c_void_p()))
    with pytest.raises(_lib.MjlError, match=r"mjx355 error 1 \(MJL_ERR_ARG\): .*bad argument"):
        _lib.check(rc)
    _lib.check(0)


def test_fused_apg_entries_reject_null_without_gpu():
    """The fused APG entry points (record + bookkeeping + next policy, replay + policy backward) report a
    null batch or a null buffer as an argument error before any device call; the eligibility query says
    0 for a null batch."""
    L = _lib.lib()
    assert L.mjl_env_record_fused(None) == 0
    z = [None] * 7
    assert L.mjl_env_step_record_apg(None, 0, None, None, None, None, None, 0.99, 0.0, *z) == 1
    assert b"bad argument" in L.mjl_last_error()
    assert L.mjl_env_step_record_apg_next(None, 0, None, None, None, None, None, 0.99, 0.0, *([None] * 8), 0, None,
                                          None, None, 1, None, None, None, None, None) == 1
    assert L.mjl_env_step_vjp_replay_apg(None, 0, *([None] * 12), 1, None, None, None, None, None, None, None, 0,
                                         None) == 1
