"""Members of primme_params / primme_svds_params by name, and the configuration listing (include/primme_amd.h:
primme_member_info, primme_set_member, primme_constant_info, primme_display_params and their primme_svds_* twins).

A name is the library's own ("correction_maxInnerIterations") or the member as C writes it
("correctionParams.maxInnerIterations"); for primme_svds_params, "primme.<name>" and "primmeStage2.<name>" reach into the two
eigensolver blocks."""
import ctypes as C

from . import _ffi as F

PRIMME_INT_KIND, PRIMME_DOUBLE_KIND, PRIMME_POINTER_KIND, PRIMME_STRING_KIND = range(4)     # primme_type


def _info(lib, svds, name):
    """(label, kind, arity) of the member `name`; ValueError when the library knows no such member"""
    member_info = lib.primme_svds_member_info if svds else lib.primme_member_info
    for cand in dict.fromkeys((name, name.replace("Params.", ".").replace(".", "_"))):
        label, cname, kind, arity = C.c_int(0), C.c_char_p(cand.encode()), C.c_int(0), C.c_int(0)
        if member_info(C.byref(label), C.byref(cname), C.byref(kind), C.byref(arity)) == 0:
            return label.value, kind.value, arity.value
    raise ValueError(f"members: {'primme_svds_params' if svds else 'primme_params'} has no member {name!r}")


def _set(lib, svds, block, name, value, keep):
    label, kind, arity = _info(lib, svds, name)
    if kind == PRIMME_INT_KIND:
        if isinstance(value, str):
            v = C.c_int(0)
            if (lib.primme_svds_constant_info if svds else lib.primme_constant_info)(value.encode(), C.byref(v)):
                raise ValueError(f"members: {name!r}: unknown constant {value!r}")
            value = v.value
        if hasattr(value, "__len__"):
            arg = (F.PRIMME_INT * len(value))(*[int(x) for x in value])     # iseed
        else:
            arg = F.PRIMME_INT(int(value))
        arg = C.cast(C.pointer(arg), C.c_void_p)
    elif kind == PRIMME_DOUBLE_KIND and arity == 1:
        arg = C.cast(C.pointer(C.c_double(float(value))), C.c_void_p)
    elif kind == PRIMME_DOUBLE_KIND:
        arr = (C.c_double * len(value))(*[float(x) for x in value])         # the array itself is the member: it must outlive the solve
        keep.append(arr)
        arg = C.cast(arr, C.c_void_p)
    elif kind == PRIMME_STRING_KIND:
        s = C.c_char_p(value if isinstance(value, bytes) else str(value).encode())
        keep.append(s)
        arg = C.cast(s, C.c_void_p)
    else:
        arg = C.c_void_p(value) if value is None or isinstance(value, int) else C.cast(value, C.c_void_p)
    if (lib.primme_svds_set_member if svds else lib.primme_set_member)(block, label, arg):
        raise ValueError(f"members: {name!r} cannot be set to {value!r}")


def apply_members(lib, p, members, keep):
    """primme_set_member for every item of `members` on the PrimmeParams `p`; arrays and strings handed over are appended to
    `keep`, which must live as long as `p` is used"""
    F.declare_members(lib)
    for name, value in (members or {}).items():
        _set(lib, False, C.byref(p), name, value, keep)


def apply_svds_members(lib, ps, members, keep):
    F.declare_members(lib)
    for name, value in (members or {}).items():
        stage, _, rest = name.partition(".")
        if stage in ("primme", "primmeStage2") and rest:
            block = C.c_void_p()
            lib.primme_svds_get_member(C.byref(ps), _info(lib, True, stage)[0], C.byref(block))
            _set(lib, False, block, rest, value, keep)
        else:
            _set(lib, True, C.byref(ps), name, value, keep)


def display_params(p, lib=None):
    """The text primme_display_params (a PrimmeParams) or primme_svds_display_params (a PrimmeSvdsParams) prints for `p`."""
    lib = lib or F.load_product()
    F.declare_members(lib)
    libc = C.CDLL(None)
    libc.open_memstream.restype = C.c_void_p
    libc.open_memstream.argtypes = [C.POINTER(C.c_void_p), C.POINTER(C.c_size_t)]
    libc.fclose.argtypes = [C.c_void_p]
    libc.free.argtypes = [C.c_void_p]
    buf, size = C.c_void_p(), C.c_size_t(0)
    stream = libc.open_memstream(C.byref(buf), C.byref(size))
    if not stream:
        raise OSError("open_memstream failed")
    q = type(p).from_buffer_copy(p)       # the listing goes to the block's outputFile: a copy, so that `p` keeps its own
    q.outputFile = stream
    try:
        (lib.primme_svds_display_params if isinstance(p, F.PrimmeSvdsParams) else lib.primme_display_params)(q)
    finally:
        libc.fclose(stream)
    text = C.string_at(buf, size.value).decode()
    libc.free(buf)
    return text
