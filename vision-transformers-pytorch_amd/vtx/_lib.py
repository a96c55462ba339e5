"""ctypes binding of libvtx.so, derived from include/vtx.h and include/vtx_vos.h at import.

The C ABI is written down once, in include/vtx.h: every csrc/*.hip compiles its definitions against that header, and this
module reads the same file -- prototypes, the public structs and the integer #defines -- instead of mirroring it.  Only the
JPEG records of csrc/jpeg_host.h / csrc/jpeg_sync.h, which the public header does not declare, are typed by hand.
include/vtx_vos.h (the DAVIS J&F entries of csrc/davis.hip) is read the same way into a table of its own, _VOS_SIGNATURES, with
its own version: _SIGNATURES, exported_symbols() and ABI_VERSION remain what include/vtx.h states.

The library is the product: there is NO fallback.  If libvtx.so is missing or a call returns a
non-zero code this module raises -- it never routes to PyTorch ops or to the CPU oracle.
"""
import ctypes
import os
import re

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("VTX_LIBVTX") or os.path.join(_HERE, "libvtx.so")   # (override: A/B of two builds on one box)
HEADER_PATH = os.path.join(os.path.dirname(os.path.dirname(_HERE)), "include", "vtx.h")
VOS_HEADER_PATH = os.path.join(os.path.dirname(HEADER_PATH), "vtx_vos.h")


class VtxError(RuntimeError):
    pass


_SCALARS = {"int": ctypes.c_int, "unsigned": ctypes.c_uint, "int64_t": ctypes.c_int64, "uint64_t": ctypes.c_uint64,
            "size_t": ctypes.c_size_t, "float": ctypes.c_float, "double": ctypes.c_double, "int32_t": ctypes.c_int32,
            "uint16_t": ctypes.c_uint16}


def _ctype(ctext, decl, ret=False, name="include/vtx.h"):
    """ctypes type of the C type ``ctext``: any pointer is c_void_p (callers pass integers, None and byref(...)), a returned
    ``const char*`` is c_char_p, the scalars of _SCALARS map to themselves; anything else raises, naming ``decl``."""
    words = " ".join(ctext.replace("*", " * ").split())
    if "*" in words:
        if not ret:
            return ctypes.c_void_p
        if words == "const char *":
            return ctypes.c_char_p
    elif words.replace("const ", "") in _SCALARS:
        return _SCALARS[words.replace("const ", "")]
    raise VtxError(f"{name}: no ctypes type for '{ctext.strip()}' in '{' '.join(decl.split())}'")


def _struct_fields(body, decl, header="include/vtx.h"):
    """_fields_ of one struct body: ``type a, *b, c[96];`` per statement, several declarators allowed."""
    fields = []
    for stmt in filter(None, (s.strip() for s in body.split(";"))):
        base, rest = re.fullmatch(r"((?:const\s+)?\w*)(.*)", stmt, re.S).groups()
        for d in rest.split(","):
            m = re.fullmatch(r"\s*(\*?)\s*(\w+)\s*(?:\[(\d+)\])?\s*", d)
            if not m:
                raise VtxError(f"{header}: cannot read the field '{' '.join(stmt.split())}' of {decl}")
            star, name, dim = m.groups()
            t = ctypes.c_char if (base, star, bool(dim)) == ("char", "", True) else _ctype(base + star, f"{decl}: {stmt}", name=header)
            fields.append((name, t * int(dim) if dim else t))
    return fields


def read_header(text, name="include/vtx.h"):
    """The C ABI as a public header states it: (prototypes, structs, defines) =
    ({name: (restype, [argtypes])}, {typedef name: _fields_}, {macro: int}).  A declaration that is not understood raises,
    naming the file ``name``."""
    text = re.sub(r"/\*.*?\*/|//[^\n]*", lambda m: " " + "\n" * m.group().count("\n"), text, flags=re.S)   # comments name entries too
    defines = {m.group(1): int(m.group(2)) for m in re.finditer(r"^[ \t]*#[ \t]*define[ \t]+(\w+)[ \t]+\(?(-?\d+)\)?[ \t]*$", text, re.M)}
    text = re.sub(r"^[ \t]*#[ \t]*ifdef[ \t]+__cplusplus\b.*?^[ \t]*#[ \t]*endif\b", "", text, flags=re.M | re.S)   # extern "C" { and }
    text = re.sub(r"^[ \t]*#.*$", "", text, flags=re.M)
    structs = {}

    def take_struct(m):
        structs[m.group(2)] = _struct_fields(m.group(1), m.group(2), name)
        return " "
    text = re.sub(r"\btypedef\s+struct\s+\w*\s*\{([^{}]*)\}\s*(\w+)\s*;", take_struct, text)
    text = re.sub(r"\benum\s*\w*\s*\{[^{}]*\}\s*;", " ", text)
    protos = {}
    for stmt in filter(None, (s.strip() for s in text.split(";"))):
        m = re.fullmatch(r"([^()]*?)(\w+)\s*\(([^()]*)\)", stmt)
        if not m:
            raise VtxError(f"{name}: not a prototype: '{' '.join(stmt.split())}'")
        params = [] if m.group(3).strip() in ("", "void") else m.group(3).split(",")
        protos[m.group(2)] = (_ctype(m.group(1), stmt, ret=True, name=name),
                              [_ctype(re.fullmatch(r"(.*?)\w*", p, re.S).group(1), stmt, name=name) for p in params])
    return protos, structs, defines


try:
    with open(HEADER_PATH) as _fh:
        _SIGNATURES, _STRUCTS, _DEFINES = read_header(_fh.read())
except OSError as _e:
    raise VtxError(f"{HEADER_PATH} not found: the binding of libvtx.so is read from the public header") from _e

# every integer VTX_* macro of the header under its name without the prefix: F32, BF16, ABI_VERSION, OK, ERR_SHAPE .. ERR_JPEG,
# ATTN_WINDOW, ATTN_GLOBAL, Q_RESID .. Q_INPLACE
globals().update({k[4:]: v for k, v in _DEFINES.items() if k.startswith("VTX_")})
ABI_VERSION = _DEFINES["VTX_ABI_VERSION"]      # (named: load() compares the library against it)

# the second public header: the DAVIS J&F entries (csrc/davis.hip).  Its prototypes are bound next to _SIGNATURES and its
# VTX_VOS_* macros are exported as VOS_*; it declares no struct and no error code.
try:
    with open(VOS_HEADER_PATH) as _fh:
        _VOS_SIGNATURES, _VOS_STRUCTS, _VOS_DEFINES = read_header(_fh.read(), "include/vtx_vos.h")
except OSError as _e:
    raise VtxError(f"{VOS_HEADER_PATH} not found: the binding of libvtx.so is read from the public headers") from _e
if _VOS_STRUCTS or set(_VOS_SIGNATURES) & set(_SIGNATURES) or set(_VOS_DEFINES) & set(_DEFINES):
    raise VtxError("include/vtx_vos.h declares a struct, or redeclares an entry or a macro of include/vtx.h")
globals().update({k[4:]: v for k, v in _VOS_DEFINES.items() if k.startswith("VTX_VOS_")})
VOS_ABI_VERSION = _VOS_DEFINES["VTX_VOS_ABI_VERSION"]


class LayerFwd(ctypes.Structure):
    """include/vtx.h VtxLayerFwd (load() checks sizeof against the library)."""
    _fields_ = _STRUCTS["VtxLayerFwd"]


class LayerBwd(ctypes.Structure):
    """include/vtx.h VtxLayerBwd."""
    _fields_ = _STRUCTS["VtxLayerBwd"]


class SrLayerFwd(ctypes.Structure):
    """include/vtx.h VtxSrLayerFwd."""
    _fields_ = _STRUCTS["VtxSrLayerFwd"]


class SrLayerBwd(ctypes.Structure):
    """include/vtx.h VtxSrLayerBwd."""
    _fields_ = _STRUCTS["VtxSrLayerBwd"]


class TimerRec(ctypes.Structure):
    """include/vtx.h VtxTimerRec."""
    _fields_ = _STRUCTS["VtxTimerRec"]


class Route(ctypes.Structure):
    """include/vtx.h VtxRoute: the kernel instantiation a launch takes, as the library decides it (vtx_*_route)."""
    _fields_ = _STRUCTS["VtxRoute"]


class GemmQuery(ctypes.Structure):
    """include/vtx.h VtxGemmQuery."""
    _fields_ = _STRUCTS["VtxGemmQuery"]


_I, _L = ctypes.c_int, ctypes.c_int64


class JpegInfo(ctypes.Structure):
    """csrc/jpeg_host.h VtxJpegInfo."""
    _fields_ = [(n, _I) for n in ("width", "height", "ncomp", "hs", "vs", "mcux", "mcuy", "reason", "restart")] + [("reserved", _I * 3)]


class JpegPlan(ctypes.Structure):
    """csrc/jpeg_host.h VtxJpegPlan (load() checks sizeof against vtx_jpeg_plan_bytes())."""
    _fields_ = ([(n, _I) for n in ("width", "height", "ncomp", "hs", "vs", "mcux", "mcuy", "mx0", "my0", "smx", "smy", "row0", "col0",
                                   "rows", "cols", "pad")] +
                [(n, _L) for n in ("coef_off", "ws_off", "out_off", "reserved")] + [("q", ctypes.c_uint16 * 64 * 3)])


class JpegScanHead(ctypes.Structure):
    """csrc/jpeg_sync.h JsScan up to ``reserved``: the fixed-size head of a scan record (the Huffman tables follow)."""
    _fields_ = ([(n, ctypes.c_int32) for n in ("ncomp", "hs", "vs", "mcux", "mcuy", "mx0", "my0", "smx", "smy", "restart", "nseg", "nsub")] +
                [(n, _L) for n in ("coef_off", "stream_off", "stream_bytes", "seg_off", "sub_off", "reserved")])


_lib = None


def load():
    """Load libvtx.so once; raise VtxError (never fall back) if it is absent or stale."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise VtxError(
            f"{LIB_PATH} not found: the HIP extension is the product path and has no fallback. "
            "Build it with `python -c 'import __graft_entry__ as g; g.build()'`.")
    lib = ctypes.CDLL(LIB_PATH)
    for name, (res, args) in list(_SIGNATURES.items()) + list(_VOS_SIGNATURES.items()):
        try:
            fn = getattr(lib, name)
        except AttributeError as e:
            raise VtxError(f"libvtx.so does not export {name} (stale build?)") from e
        fn.restype = res
        fn.argtypes = args
    if lib.vtx_abi_version() != ABI_VERSION:
        raise VtxError(f"libvtx.so ABI {lib.vtx_abi_version()} != binding ABI {ABI_VERSION}: rebuild")
    if lib.vtx_vos_abi_version() != VOS_ABI_VERSION:
        raise VtxError(f"libvtx.so VOS ABI {lib.vtx_vos_abi_version()} != binding VOS ABI {VOS_ABI_VERSION} "
                       "(include/vtx_vos.h): rebuild")
    if lib.vtx_layer_desc_bytes(0) != ctypes.sizeof(LayerFwd) or lib.vtx_layer_desc_bytes(1) != ctypes.sizeof(LayerBwd):
        raise VtxError("libvtx.so layer descriptors do not match the bindings (VtxLayerFwd / VtxLayerBwd): rebuild")
    if lib.vtx_layer_desc_bytes(2) != ctypes.sizeof(SrLayerFwd) or lib.vtx_layer_desc_bytes(3) != ctypes.sizeof(SrLayerBwd):
        raise VtxError("libvtx.so layer descriptors do not match the bindings (VtxSrLayerFwd / VtxSrLayerBwd): rebuild")
    if lib.vtx_layer_desc_bytes(4) != ctypes.sizeof(Route) or lib.vtx_layer_desc_bytes(5) != ctypes.sizeof(GemmQuery):
        raise VtxError("libvtx.so route records do not match the bindings (VtxRoute / VtxGemmQuery): rebuild")
    if lib.vtx_jpeg_plan_bytes() != ctypes.sizeof(JpegPlan) or lib.vtx_jpeg_scan_bytes() < ctypes.sizeof(JpegScanHead):
        raise VtxError("libvtx.so JPEG records do not match the bindings (VtxJpegPlan / JsScan): rebuild")
    _lib = lib
    return lib


def exported_symbols():
    return sorted(_SIGNATURES)


def check(code, what):
    if code != 0:
        msg = load().vtx_strerror(code).decode()
        raise VtxError(f"{what} failed: {msg} (code {code})")
