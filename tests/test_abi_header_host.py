"""Host-side checks of the header reader behind vtx/_lib.py (no GPU): the binding of libvtx.so is derived from include/vtx.h,
so the reader is tested on synthetic header text -- one case per construct the public header uses -- and the two entries whose
hand-written binding had drifted from the header are called with the header's argument count."""
import ctypes
from ctypes import c_char, c_char_p, c_float, c_int, c_int64, c_size_t, c_uint, c_void_p

import pytest


def _read(text):
    from vtx import _lib
    return _lib.read_header(text)


def test_prototype_broken_over_three_lines():
    protos, structs, defines = _read("int vtx_foo(const void* x, int64_t rows,\n"
                                     "            size_t ws_bytes, float eps,\n"
                                     "            void* stream);\n")
    assert protos == {"vtx_foo": (c_int, [c_void_p, c_int64, c_size_t, c_float, c_void_p])}
    assert structs == {} and defines == {}


def test_pointer_to_const_pointer_parameter():
    protos, _, _ = _read("int vtx_colreduce(int n, const float* const* part, float* const* out0, double* flops);")
    assert protos["vtx_colreduce"] == (c_int, [c_int, c_void_p, c_void_p, c_void_p])


def test_unsigned_parameter_and_returns():
    protos, _, _ = _read("int vtx_poison(unsigned pattern, int rounds);\nconst char* vtx_strerror(int code);\nsize_t vtx_bytes(uint64_t seed);")
    assert protos["vtx_poison"] == (c_int, [c_uint, c_int])
    assert protos["vtx_strerror"] == (c_char_p, [c_int])
    assert protos["vtx_bytes"] == (c_size_t, [ctypes.c_uint64])


def test_void_parameter_list_is_empty():
    protos, _, _ = _read("int vtx_abi_version(void);\nsize_t vtx_plan_bytes( void );")
    assert protos == {"vtx_abi_version": (c_int, []), "vtx_plan_bytes": (c_size_t, [])}


def test_comments_are_not_declarations():
    text = ("/* partial rows: vtx_foo(1, 2) of stride vtx_ld(nH);\n"
            " * a second line; with semicolons; int vtx_ghost(int a); */\n"
            "#ifdef __cplusplus\nextern \"C\" {\n#endif\n"
            "#define VTX_ERR_NULL (-6)      /* required; pointer */\n"
            "#define VTX_Q_BIAS 16\n"
            "int vtx_real(int a);   // sizeof: vtx_desc_bytes(4 / 5); see above\n"
            "#ifdef __cplusplus\n}\n#endif\n")
    protos, _, defines = _read(text)
    assert protos == {"vtx_real": (c_int, [c_int])}
    assert defines == {"VTX_ERR_NULL": -6, "VTX_Q_BIAS": 16}


def test_struct_with_several_declarators_an_array_and_pointers():
    text = ("typedef struct VtxRec {\n"
            "  int family;                 /* 1 skinny | 2 two-group; */\n"
            "  int tile_m, tile_n, tile_k;\n"
            "  int64_t M;\n"
            "  const float *ln1_w, *ln1_b;\n"
            "  const float* rel_pos; const int64_t* pos;\n"
            "  void* ws;\n"
            "  size_t ws_bytes;\n"
            "  char label[96];\n"
            "} VtxRec;\n"
            "int vtx_route(const VtxRec* q, VtxRec* out);\n")
    protos, structs, _ = _read(text)
    assert protos == {"vtx_route": (c_int, [c_void_p, c_void_p])}          # the struct body is no prototype
    fields = structs["VtxRec"]
    assert [n for n, _ in fields] == ["family", "tile_m", "tile_n", "tile_k", "M", "ln1_w", "ln1_b", "rel_pos", "pos", "ws", "ws_bytes", "label"]
    kinds = dict(fields)
    assert kinds["tile_k"] is c_int and kinds["M"] is c_int64 and kinds["ln1_b"] is c_void_p and kinds["pos"] is c_void_p
    assert kinds["ws"] is c_void_p and kinds["ws_bytes"] is c_size_t
    assert kinds["label"]._type_ is c_char and kinds["label"]._length_ == 96

    class Rec(ctypes.Structure):
        _fields_ = fields
    assert ctypes.sizeof(Rec) == 4 * 4 + 8 + 5 * 8 + 8 + 96


@pytest.mark.parametrize("text", ["int vtx_foo(struct Thing t);", "int vtx_foo(long n);", "short vtx_foo(int n);", "float* vtx_foo(int n);",
                                  "int vtx_foo(int);", "typedef struct R { long n; } R;", "typedef struct R { int **pp; } R;", "int vtx_global;"])
def test_unknown_declarations_raise(text):
    from vtx._lib import VtxError
    with pytest.raises(VtxError, match="include/vtx.h"):
        _read(text)


def test_binding_of_the_real_header_is_the_headers():
    """Every prototype of include/vtx.h is bound, the public structs come from its typedefs, the constants from its #defines."""
    from vtx import _lib
    protos, structs, defines = _lib.read_header(open(_lib.HEADER_PATH).read())
    assert protos == _lib._SIGNATURES and len(protos) == 169
    assert sorted(structs) == ["VtxGemmQuery", "VtxLayerBwd", "VtxLayerFwd", "VtxRoute", "VtxSrLayerBwd", "VtxSrLayerFwd", "VtxTimerRec"]
    for name, fields in structs.items():
        assert getattr(_lib, name[3:])._fields_ == fields
    assert (_lib.F32, _lib.BF16, _lib.ATTN_WINDOW, _lib.ATTN_GLOBAL) == (0, 1, 1, 2)
    assert (_lib.OK, _lib.ERR_SHAPE, _lib.ERR_NULL, _lib.ERR_JPEG) == (0, -1, -6, -7)
    assert [_lib.Q_RESID, _lib.Q_AUXOUT, _lib.Q_AUXIN, _lib.Q_MAPPED, _lib.Q_BIAS, _lib.Q_ROWSCALE, _lib.Q_INPLACE] == [1 << i for i in range(7)]
    assert _lib.ABI_VERSION == defines["VTX_ABI_VERSION"] == 30
    assert _lib._SIGNATURES["vtx_debug_mfma_peak"][1][3] is c_void_p       # bench.py passes byref(c_double)
    fl = ctypes.c_double(0.0)
    assert c_void_p.from_param(ctypes.byref(fl)) is not None


def test_mapped_window_attention_entries_take_the_headers_argument_counts():
    """vtx_wattn_fwd_mapped has 16 parameters and vtx_wattn_bwd_mapped 22 (the hand-written table had 17 and 23).  Both
    definitions return VTX_ERR_NULL on their first line, before any HIP call: callable without a GPU."""
    from vtx import _lib
    lib = _lib.load()
    assert len(_lib._SIGNATURES["vtx_wattn_fwd_mapped"][1]) == 16 and len(_lib._SIGNATURES["vtx_wattn_bwd_mapped"][1]) == 22
    #                            qkv   o     lse   rel   pos   region perm  Bk L   nH H   W   win shift dtype     stream
    assert lib.vtx_wattn_fwd_mapped(None, None, None, None, None, None, None, 1, 49, 3, 14, 14, 7, 0, _lib.BF16, None) == _lib.ERR_NULL
    #                            qkv   o     dout  lse   rel   pos   region dqkv  ws   bytes inv  n  perm  Bk L   nH H   W   win shift dtype    stream
    assert lib.vtx_wattn_bwd_mapped(None, None, None, None, None, None, None, None, None, 0, None, 0, None, 1, 49, 3, 14, 14, 7, 0, _lib.BF16, None) == _lib.ERR_NULL
