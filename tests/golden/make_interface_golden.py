"""Captures from the LIVE reference (oracle/_ref/libprimme_ref.so, built by `make -C oracle ref`) what
tests/test_interface_members.py and tests/test_interface_members_gpu.py compare the product with:

    reference_member_names.json     per structure: every label primme_member_info knows (label, name, type, arity), the labels
                                    in range it does not know, the enumerator names with their values (the enumerator names
                                    are read from the reference's headers and asked of ?_constant_info one by one) and, per
                                    member of enum type, the names ?_enum_member_info lists
    display_ex_eigs_members.txt     what primme_display_params prints for the settings of examples/ex_eigs_members.c

    python tests/golden/make_interface_golden.py [path to the reference's include directory]
"""
import ctypes as C
import json
import os
import re
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "oracle"))

import checkers                                   # noqa: E402
from primme_amd import _ffi as F                  # noqa: E402
from primme_amd.members import display_params     # noqa: E402

# examples/ex_eigs_members.c: its options, then primme_set_method(PRIMME_DEFAULT_MIN_MATVECS)
EXAMPLE_OPTIONS = [("n", 100), ("numEvals", 5), ("eps", 1e-9), ("target", "primme_smallest"), ("maxBasisSize", 20), ("printLevel", 0)]


def enumerators(include_dir):
    names = []
    for h in ("primme_eigs.h", "primme_svds.h"):
        txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(include_dir, h)).read(), flags=re.S)
        for body in re.findall(r"typedef\s+enum\s*\{(.*?)\}", txt, flags=re.S):
            names += re.findall(r"\b([A-Za-z_]\w*)\b\s*(?:=\s*\d+\s*)?(?:,|$)", body.strip())
    return list(dict.fromkeys(names))


def capture(lib, prefix, names):
    info, const, enum = (getattr(lib, prefix + f) for f in ("member_info", "constant_info", "enum_member_info"))
    members, unknown, label = [], [], 1
    misses = 0
    while misses < 8:                        # the labels are dense but for a few the reference has no name for
        lb, nm, ty, ar = C.c_int(label), C.c_char_p(None), C.c_int(-1), C.c_int(-1)
        if info(C.byref(lb), C.byref(nm), C.byref(ty), C.byref(ar)) == 0:
            members.append(dict(label=lb.value, name=nm.value.decode(), type=ty.value, arity=ar.value))
            unknown += list(range(label - misses, label))
            misses = 0
        else:
            misses += 1
        label += 1
    constants = {}
    for n in names:
        v = C.c_int(-12345)
        if const(n.encode(), C.byref(v)) == 0:
            constants[n] = v.value
    enums = {}
    for m in members:
        got, value = [], 0
        while True:
            v, s = C.c_int(value), C.c_char_p(None)
            if enum(m["label"], C.byref(v), C.byref(s)) != 0:
                break
            got.append(s.value.decode())
            value += 1
        if got:
            enums[m["name"]] = got
    return dict(members=members, unnamed_labels=unknown, constants=constants, enum_members=enums)


def example_display(lib):
    p = F.PrimmeParams()
    lib.primme_initialize(C.byref(p))
    for name, value in EXAMPLE_OPTIONS:
        lb, nm, ty, ar = C.c_int(0), C.c_char_p(name.encode()), C.c_int(0), C.c_int(0)
        assert lib.primme_member_info(C.byref(lb), C.byref(nm), C.byref(ty), C.byref(ar)) == 0, name
        if isinstance(value, str):
            v = C.c_int()
            assert lib.primme_constant_info(value.encode(), C.byref(v)) == 0, value
            value = v.value
        arg = C.c_double(value) if ty.value == 1 else F.PRIMME_INT(value)
        assert lib.primme_set_member(C.byref(p), lb.value, C.cast(C.pointer(arg), C.c_void_p)) == 0, name
    assert lib.primme_set_method(F.PRIMME_DEFAULT_MIN_MATVECS, C.byref(p)) == 0
    return display_params(p, lib=lib)


def main():
    include_dir = sys.argv[1] if len(sys.argv) > 1 else "/root/reference/include"
    lib = checkers.load_reference()
    F.declare_members(lib)
    names = enumerators(include_dir)
    out = dict(eigs=capture(lib, "primme_", names), svds=capture(lib, "primme_svds_", names))
    with open(os.path.join(HERE, "reference_member_names.json"), "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    with open(os.path.join(HERE, "display_ex_eigs_members.txt"), "w") as f:
        f.write(example_display(lib))
    for k in ("eigs", "svds"):
        print(k, len(out[k]["members"]), "named labels,", out[k]["unnamed_labels"], "unnamed,", len(out[k]["constants"]), "constants")


if __name__ == "__main__":
    main()
