"""The Python binding is derived from include/vlhip.h: the parsed signatures against literal expectations, what the parser
refuses, the named constants of ops.py and the launch-routing context.  CPU only; needs the library built."""
import re
from ctypes import c_char_p, c_float, c_int, c_int64, c_uint64, c_void_p

import pytest

from clg_vqa_amd import _lib, ops

P = c_void_p
# literal signatures, written out by hand: one per construct the parser meets in the header
PINNED = {
    "vl_version": (c_int, []),                                                    # (void), int
    "vl_last_error": (c_char_p, []),                                              # const char* return
    "vl_sumsq_ws_floats": (c_int64, []),                                          # int64_t return, (void)
    "vl_colsum_finalize": (c_int, [P, c_int64, c_int64, P, c_int64, c_int, P]),   # float* const* outs
    "vl_transpose_blocked": (c_int, [P, c_int64, c_int64, c_int64, P]),           # a parameter followed by a comment
    "vl_gemm_nt_ex": (c_int, [P, P, c_int64, P, P, c_int64, c_int64, c_int64, c_int64, c_int, c_int, P, P, P, c_int64,
                              P, P, P, c_int64, P, P]),
    "vl_ln_fwd_rr": (c_int, [P, P, P, P, c_int64, P, P, P, P, c_float, P, P, P, P, P, c_int64, c_int64, c_int64, c_int64,
                             c_int64, c_float, c_float, c_uint64, c_int64, c_int64, P]),
    "vl_attn2_fwd": (c_int, [P, P, P, P, P, P, c_int64, c_int64, c_int64, c_int64, c_int64, c_float, c_uint64, P]),
    "vl_adamw": (c_int, [P, P, P, P, c_int64, P, P, P, c_int64, c_float, c_float, c_float, c_int64, P, c_int, c_float,
                         P, c_float, P, c_float, c_float, P, c_int, P, c_int64, c_int64, c_int64, P]),
}


@pytest.mark.parametrize("name", sorted(PINNED))
def test_parsed_signature_equals_the_literal_one(name):
    res, args = _lib._SIGS[name]
    assert res is PINNED[name][0]
    assert args == PINNED[name][1]
    assert len(PINNED["vl_gemm_nt_ex"][1]) == 21 and len(PINNED["vl_ln_fwd_rr"][1]) == 26 and len(PINNED["vl_adamw"][1]) == 28


def test_every_declared_symbol_is_bound_with_the_parsed_signature():
    names = _lib.header_symbols()
    assert len(names) == len(_lib._SIGS) >= 64 and set(names) == set(_lib._SIGS)
    L = _lib.lib()
    for n in names:
        res, args = _lib._SIGS[n]
        fn = getattr(L, n)
        assert fn.restype is res, n
        assert list(fn.argtypes) == args, n
        assert all(t in (c_void_p, c_int, c_int64, c_uint64, c_float) for t in args), n


def test_header_is_read_once_and_the_engine_shares_the_constants_of_ops(monkeypatch):
    from clg_vqa_amd import engine
    assert engine.VL is ops.C and ops.C == _lib.header_constants()
    monkeypatch.setattr(_lib, "HEADER_PATH", "/nonexistent/vlhip.h")  # nothing opens the file again
    assert _lib.header_constants() == ops.C and set(_lib.header_symbols()) == set(_lib._SIGS)


@pytest.mark.parametrize("text, match", [
    ("int vl_probe(const float* x, double scale, void* stream);", r"vl_probe.*double scale"),      # unknown scalar type
    ("int vl_probe(unsigned n);", r"vl_probe.*unsigned n"),                                          # no guessed c_void_p
    ("int vl_probe(int);", r"vl_probe.*'int'"),                                                      # unnamed parameter
    ("void vl_probe(int n);", r"vl_probe.*'void'"),                                                  # unknown return type
    ("int vl_probe(const float* x, int64_t n;\nint vl_next(int n);", r"vl_probe.*int64_t n"),        # unterminated list
    ("int vl_probe(int n)", r"vl_probe"),                                                            # no semicolon: still seen
    ("int vl_probe(int n);\nint vl_probe(int64_t n);", r"vl_probe.*twice"),
    ("struct vl_probe { int n; };", r"vl_probe"),                                                    # vl_ name, no prototype
])
def test_parser_refuses_what_it_does_not_understand(text, match):
    with pytest.raises(RuntimeError, match=match):
        _lib.parse_signatures(text)


def test_parser_reads_a_well_formed_declaration():
    text = 'extern "C" {\n#define VL_N 3\nenum { VL_A = 0 };\nint64_t vl_probe(const int64_t* tab, int n,\n float p, uint64_t s);\n}'
    assert _lib.parse_signatures(text) == {"vl_probe": (c_int64, [c_void_p, c_int, c_float, c_uint64])}


def test_ops_enumerators_are_the_headers():
    C = _lib.header_constants()
    for n in ("F32", "GELU_SPLIT", "DGELU_BF16", "BF16", "SPLIT"):
        assert getattr(ops, "EPI_" + n) == C["VL_EPI_" + n]
    for n in ("NONE", "RELU", "TANH", "GELU"):
        assert getattr(ops, "ACT_" + n) == C["VL_ACT_" + n]
    # the values the kernels were built with (include/vlhip.h)
    assert (ops.EPI_F32, ops.EPI_GELU_SPLIT, ops.EPI_DGELU_BF16, ops.EPI_BF16, ops.EPI_SPLIT) == (0, 1, 2, 3, 4)
    assert (ops.ACT_NONE, ops.ACT_RELU, ops.ACT_TANH, ops.ACT_GELU) == (0, 1, 2, 3)
    assert (C["VL_GX_FIELDS"], C["VL_TR_FIELDS"], C["VL_DW_FIELDS"], C["VL_CR_FIELDS"], C["VL_SC_FIELDS"]) == (8, 6, 10, 8, 6)


def test_ops_source_names_no_abi_index_or_width():
    with open(ops.__file__) as f:
        src = f.read()
    assert not re.search(r"extra\[\d", src)
    assert not re.search(r"_table\(\d", src)


def _routing():
    return ops._launch.stream, ops._launch.hold


def test_launching_restores_the_previous_routing():
    assert _routing() == (None, None)
    hold_a, hold_b = [], []
    with ops.launching(11, hold_a):
        assert _routing() == (11, hold_a) and ops._launch.hold is hold_a
        assert ops._stream() == 11
        with ops.launching(22, hold_b):  # nested
            assert _routing() == (22, hold_b) and ops._launch.hold is hold_b
            with ops.launching(33):
                assert _routing() == (33, None)
            assert _routing() == (22, hold_b)
        assert _routing() == (11, hold_a) and ops._launch.hold is hold_a
    assert _routing() == (None, None)


def test_launching_restores_the_previous_routing_after_an_exception():
    with ops.launching(5):
        with pytest.raises(KeyError):
            with ops.launching(11):
                with ops.launching(22):
                    ops.set_stream(44)  # (the engine switches streams inside a pass with the primitive)
                    raise KeyError("x")
        assert _routing() == (5, None)
    assert _routing() == (None, None)
