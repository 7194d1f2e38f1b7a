"""The boundary a program written against the reference sees: primme.h, the members by label and by name, the
configuration listings.  Everything is equality with the LIVE reference (oracle/_ref, skipped where it is not built) or
with what tests/golden/make_interface_golden.py captured from it (tests/golden/reference_member_names.json)."""
import ctypes as C
import json
import os
import subprocess

import pytest

from primme_amd import _ffi as F

import checkers

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = json.load(open(os.path.join(ROOT, "tests", "golden", "reference_member_names.json")))
REF_EXAMPLES = "/root/reference/examples"
STRUCTS = {"eigs": ("primme_", F.PrimmeParams), "svds": ("primme_svds_", F.PrimmeSvdsParams)}
INT, DOUBLE, POINTER, STRING = range(4)
libc = C.CDLL(None)
libc.fopen.restype = C.c_void_p
libc.fopen.argtypes = [C.c_char_p, C.c_char_p]
libc.fclose.argtypes = [C.c_void_p]


@pytest.fixture(scope="module")
def product(built):
    lib = checkers.load_hostcheck()       # the product's eigs_members.c / svds_members.c, loadable without a GPU
    F.declare_members(lib)
    return lib


@pytest.fixture(scope="module")
def reference(built):
    if not os.path.exists(checkers.REFERENCE_LIB):
        pytest.skip("oracle/_ref is not built")
    lib = checkers.load_reference()
    F.declare_members(lib)
    return lib


def fn(lib, which, name):
    return getattr(lib, STRUCTS[which][0] + name)


def info(lib, which, label=None, name=None):
    """(rc, label, name, type, arity) of ?_member_info looked up by label or by name"""
    lb, nm, ty, ar = C.c_int(label or 0), C.c_char_p(None if name is None else name.encode()), C.c_int(-1), C.c_int(-1)
    rc = fn(lib, which, "member_info")(C.byref(lb), C.byref(nm), C.byref(ty), C.byref(ar))
    return rc, lb.value, None if nm.value is None else nm.value.decode(), ty.value, ar.value


def fresh(lib, which):
    p = STRUCTS[which][1]()                # zero-filled: the padding too
    (lib.primme_initialize if which == "eigs" else lib.primme_svds_initialize)(C.byref(p))
    p.outputFile = None                    # each library's own `stdout`
    if which == "svds":
        p.primme.outputFile = p.primmeStage2.outputFile = None
    return p


def walk(lib, which):
    """labels from 0 upward until ?_member_info fails, twice: 0 is the invalid label, so the walk proper starts at 1"""
    assert info(lib, which, label=0)[0] != 0
    seen, label = [], 1
    while True:
        got = info(lib, which, label=label)
        if got[0] != 0:
            return seen, label
        seen.append(got[1:])
        label += 1


# ---- labels ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("which", ["eigs", "svds"])
def test_labels_match_the_fixture(product, which):
    gold = GOLD[which]
    top = max(m["label"] for m in gold["members"])
    named = {m["label"]: m for m in gold["members"]}
    for label in range(0, top + 6):
        rc, lb, nm, ty, ar = info(product, which, label=label)
        if label in named:
            m = named[label]
            assert (rc, lb, nm, ty, ar) == (0, label, m["name"], m["type"], m["arity"]), label
            assert info(product, which, name=m["name"]) == (0, label, m["name"], m["type"], m["arity"]), m["name"]   # and by name
        else:
            assert rc == 1, label
    assert sorted(set(range(1, top + 1)) - set(named)) == gold["unnamed_labels"]
    assert info(product, which, name="noSuchMember")[0] == 1
    assert fn(product, which, "member_info")(None, None, None, None) == 1


@pytest.mark.parametrize("which", ["eigs", "svds"])
def test_labels_match_the_reference(product, reference, which):
    mine, mine_end = walk(product, which)
    theirs, theirs_end = walk(reference, which)
    assert mine == theirs and mine_end == theirs_end
    names = {m["name"] for m in GOLD[which]["members"]}
    assert all(nm in names for _, nm, _, _ in mine)
    # the walk stops at the first label the reference has no name for; past it, label by label and name by name
    top = max(m["label"] for m in GOLD[which]["members"])
    for label in range(0, top + 6):
        assert info(product, which, label=label) == info(reference, which, label=label), label
    for nm in sorted(names) + ["noSuchMember", "globalSumReal_type", "correctionParams.maxInnerIterations"]:
        assert info(product, which, name=nm) == info(reference, which, name=nm), nm
    # a name and a label that disagree: both libraries settle it the same way
    assert info(product, which, label=3, name="numProcs") == info(reference, which, label=3, name="numProcs")


# ---- round trip ------------------------------------------------------------------------------------------------------------------

def values_for(which, m, k):
    """what to write into member m (k: its position, which makes the value distinct): [(ctypes argument, comparable), ...]"""
    if m["type"] == INT:
        enums = GOLD[which]["enum_members"].get(m["name"])
        vals = [GOLD["svds"]["constants"][e] for e in enums] if enums else [3 + k]
        if m["name"] == "iseed":
            return [((F.PRIMME_INT * 4)(k + 1, k + 2, k + 3, k + 4), None)]
        return [(F.PRIMME_INT(v), v) for v in vals] + [(F.PRIMME_INT(2 ** 31 + k), None)]      # above INT_MAX: refused for int members
    if m["type"] == DOUBLE and m["arity"] == 1:
        return [(C.c_double(0.5 + k), 0.5 + k)]
    return [(None, 0x1000 + 16 * k)]         # pointers, strings, arrays: the pointer itself is the value (never followed here)


@pytest.mark.parametrize("which", ["eigs", "svds"])
def test_set_and_get_round_trip_like_the_reference(product, reference, which):
    top = max(m["label"] for m in GOLD[which]["members"])
    named = {m["label"]: m for m in GOLD[which]["members"]}
    a, b = fresh(product, which), fresh(reference, which)
    refused = []
    for label in range(0, top + 3):
        m = named.get(label, dict(name=f"#{label}", type=INT, arity=1))
        for arg, plain in values_for(which, m, label):
            if arg is None:
                va = vb = C.c_void_p(plain)
            else:
                va, vb = C.cast(C.pointer(arg), C.c_void_p), C.cast(C.pointer(arg), C.c_void_p)
            ra = fn(product, which, "set_member")(C.byref(a), label, va)
            rb = fn(reference, which, "set_member")(C.byref(b), label, vb)
            assert ra == rb, (m["name"], plain)
            if ra and plain is not None:
                refused.append(m["name"])
            # read back: 4 PRIMME_INTs are room for every kind
            ga, gb = (F.PRIMME_INT * 4)(-7, -7, -7, -7), (F.PRIMME_INT * 4)(-7, -7, -7, -7)
            ra = fn(product, which, "get_member")(C.byref(a), label, C.cast(ga, C.c_void_p))
            rb = fn(reference, which, "get_member")(C.byref(b), label, C.cast(gb, C.c_void_p))
            assert ra == rb, m["name"]
            if m["name"] in ("primme", "primmeStage2"):     # the address of the nested block inside each structure
                assert ga[0] - C.addressof(a) == gb[0] - C.addressof(b) == getattr(STRUCTS[which][1], m["name"]).offset
            else:
                assert list(ga) == list(gb), (m["name"], plain)
            assert bytes(a) == bytes(b), (m["name"], plain)
    # what the reference refuses to set (and what it cannot read) is restated, not repaired
    expect = {"eigs": ["stats_numGlobalSum", "stats_numBroadcast", "#0", "#90", "#91"],
              "svds": ["primme", "primmeStage2", "stats_numGlobalSum", "stats_numBroadcast", "stats_lockingIssue", "#0", "#63", "#64"]}[which]
    assert sorted(set(refused)) == sorted(expect)
    if which == "eigs":
        for label in GOLD["eigs"]["unnamed_labels"]:        # globalSumReal_type, broadcastReal_type: set yes, get no
            v = F.PRIMME_INT(2)
            assert product.primme_set_member(C.byref(a), label, C.cast(C.pointer(v), C.c_void_p)) == 0
            assert product.primme_get_member(C.byref(a), label, C.cast(C.pointer(v), C.c_void_p)) == 1
        assert a.globalSumReal_type == 2 and a.broadcastReal_type == 2


# ---- constants ------------------------------------------------------------------------------------------------------------------

def constant(lib, which, name):
    v = C.c_int(-12345)
    return fn(lib, which, "constant_info")(name.encode(), C.byref(v)), v.value


def enum_info(lib, which, label, value, name):
    v, s = C.c_int(value), C.c_char_p(None if name is None else name.encode())
    rc = fn(lib, which, "enum_member_info")(label, C.byref(v), C.byref(s))
    return rc, v.value, None if s.value is None else s.value.decode()


@pytest.mark.parametrize("which", ["eigs", "svds"])
def test_constants_match_the_fixture(product, which):
    gold = GOLD[which]
    for name, value in gold["constants"].items():
        assert constant(product, which, name) == (0, value), name
    for name in set(GOLD["svds"]["constants"]) - set(gold["constants"]) | {"primme_no_such_constant"}:
        assert constant(product, which, name) == (1, -12345), name
    labels = {m["name"]: m["label"] for m in gold["members"]}
    for member, names in gold["enum_members"].items():
        for name in names:
            value = GOLD["svds"]["constants"][name]
            assert enum_info(product, which, labels[member], -1, name) == (0, value, name)
            assert enum_info(product, which, labels[member], value, None) == (0, value, name)


@pytest.mark.parametrize("which", ["eigs", "svds"])
def test_constants_match_the_reference(product, reference, which):
    names = sorted(GOLD["svds"]["constants"]) + ["primme_no_such_constant"]
    for name in names:
        assert constant(product, which, name) == constant(reference, which, name), name
    top = max(m["label"] for m in GOLD[which]["members"])
    for label in range(0, top + 2):
        for name in names:
            assert enum_info(product, which, label, -1, name) == enum_info(reference, which, label, -1, name), (label, name)
        for value in range(0, 17):
            assert enum_info(product, which, label, value, None) == enum_info(reference, which, label, value, None), (label, value)
        # the combinations both refuse with -1
        assert enum_info(product, which, label, 1, names[0]) == enum_info(reference, which, label, 1, names[0]) == (-1, 1, names[0])
        assert enum_info(product, which, label, -1, None) == enum_info(reference, which, label, -1, None) == (-1, -1, None)


# ---- display ------------------------------------------------------------------------------------------------------------------

def shown(lib, which, p, path):
    f = libc.fopen(str(path).encode(), b"w")
    assert f
    p.outputFile = f
    try:
        fn(lib, which, "display_params")(p)
    finally:
        libc.fclose(f)
        p.outputFile = None
    return open(path, "rb").read()


def eigs_blocks():
    """name -> function that prepares a PrimmeParams through the library `lib`; `keep` holds arrays alive"""
    def preset(method):
        def f(lib, p, keep):
            p.n, p.numEvals = 1000, 3
            assert lib.primme_set_method(method, C.byref(p)) == 0
        return f

    def shifts(lib, p, keep):
        keep.append((C.c_double * 2)(0.25, -1.5e3))
        p.n, p.target, p.numTargetShifts, p.targetShifts = 500, F.primme_closest_abs, 2, keep[-1]
        assert lib.primme_set_method(F.PRIMME_JDQMR, C.byref(p)) == 0

    def ranks(lib, p, keep):
        p.n, p.nLocal, p.numProcs, p.procID = 4000, 1000, 4, 2

    def sizes(lib, p, keep):
        p.n, p.locking, p.numOrthoConst, p.initSize, p.orth, p.internalPrecision = 300, 1, 2, 3, F.primme_orth_explicit_I, F.primme_op_float
        p.aNorm, p.eps, p.correctionParams.relTolBase = 12.5, 1e-12, 1.5
        for i in range(4): p.iseed[i] = 10 ** (3 * i)

    blocks = {"initialised": lambda lib, p, keep: None, "targetShifts": shifts, "numProcs": ranks, "locking": sizes}
    for name, method in F.METHODS.items():
        blocks["method " + name] = preset(method)
    blocks["method DEFAULT_METHOD"] = preset(F.PRIMME_DEFAULT_METHOD)
    return blocks


@pytest.mark.parametrize("name", sorted(eigs_blocks()))
def test_display_params_prints_what_the_reference_prints(product, reference, tmp_path, name):
    out = []
    for lib, tag in ((product, "a"), (reference, "b")):
        p, keep = fresh(lib, "eigs"), []
        eigs_blocks()[name](lib, p, keep)
        out.append(shown(lib, "eigs", p, tmp_path / tag))
    assert out[0] == out[1]
    assert out[0].startswith(b"// ---") and b"primme.n = " in out[0]


def svds_blocks():
    def default(lib, ps, keep):
        ps.m, ps.n = 700, 300

    def hybrid(lib, ps, keep):
        ps.m, ps.n, ps.numSvals, ps.target, ps.eps, ps.internalPrecision = 300, 700, 4, 1, 1e-7, F.primme_op_double
        assert lib.primme_svds_set_method(F.SVDS_METHODS["hybrid"], F.PRIMME_DEFAULT_MIN_MATVECS, F.PRIMME_JDQMR, C.byref(ps)) == 0

    def shifts(lib, ps, keep):
        keep.append((C.c_double * 2)(0.75, 2.0))
        ps.m, ps.n, ps.target, ps.numTargetShifts, ps.targetShifts, ps.aNorm = 90, 80, 2, 2, keep[-1], 3.0
        assert lib.primme_svds_set_method(F.SVDS_METHODS["default"], F.PRIMME_DEFAULT_METHOD, F.PRIMME_DEFAULT_METHOD, C.byref(ps)) == 0
    return {"default": default, "hybrid": hybrid, "targetShifts": shifts}


@pytest.mark.parametrize("name", sorted(svds_blocks()))
def test_svds_display_params_prints_what_the_reference_prints(product, reference, tmp_path, name):
    out = []
    for lib, tag in ((product, "a"), (reference, "b")):
        ps, keep = fresh(lib, "svds"), []
        svds_blocks()[name](lib, ps, keep)
        out.append(shown(lib, "svds", ps, tmp_path / tag))
    assert out[0] == out[1]
    assert out[0].count(b"primme configuration") == {"default": 0, "hybrid": 2, "targetShifts": 2}[name]


def test_python_display_params_and_members(product):
    """primme_amd.display_params returns the listing; members= names are the library's or the C path"""
    from primme_amd.members import apply_members, apply_svds_members, display_params
    p, keep = fresh(product, "eigs"), []
    apply_members(product, p, {"maxBasisSize": 12, "correctionParams.maxInnerIterations": 0, "correction_robustShifts": 1, "eps": 1e-5,
                               "projectionParams.projection": "primme_proj_refined", "iseed": [1, 2, 3, 4],
                               "targetShifts": [0.5], "numTargetShifts": 1}, keep)
    assert (p.maxBasisSize, p.correctionParams.maxInnerIterations, p.correctionParams.robustShifts, p.eps) == (12, 0, 1, 1e-5)
    assert p.projectionParams.projection == F.primme_proj_refined and list(p.iseed) == [1, 2, 3, 4] and p.targetShifts[0] == 0.5
    text = display_params(p, lib=product)
    assert "primme.maxBasisSize = 12\n" in text and "primme.projection.projection = primme_proj_refined\n" in text
    assert "primme.targetShifts = 5.000000e-01\n" in text and not p.outputFile
    with pytest.raises(ValueError, match="noSuchMember"):
        apply_members(product, p, {"noSuchMember": 1}, keep)
    with pytest.raises(ValueError, match="primme_proj_nonsense"):
        apply_members(product, p, {"projectionParams.projection": "primme_proj_nonsense"}, keep)
    with pytest.raises(ValueError, match="stats.numGlobalSum"):
        apply_members(product, p, {"stats.numGlobalSum": 1}, keep)
    ps = fresh(product, "svds")
    apply_svds_members(product, ps, {"primme.maxBasisSize": 12, "primmeStage2.correctionParams.maxInnerIterations": 7, "maxBlockSize": 2,
                                     "method": "primme_svds_op_AtA"}, keep)
    assert (ps.primme.maxBasisSize, ps.primmeStage2.correctionParams.maxInnerIterations, ps.maxBlockSize, ps.method) == (12, 7, 2, 1)
    assert "primme_svds.method = primme_svds_op_AtA\n" in display_params(ps, lib=product)
    with pytest.raises(ValueError, match="noSuchMember"):
        apply_svds_members(product, ps, {"primme.noSuchMember": 1}, keep)


# ---- the headers ------------------------------------------------------------------------------------------------------------------

INC = os.path.join(ROOT, "include")


@pytest.mark.skipif(not os.path.isdir(REF_EXAMPLES), reason="the reference's examples are not on this machine")
@pytest.mark.parametrize("example", ["ex_eigs_dseq.c", "ex_svds_dseq.c"])
def test_reference_examples_build_as_they_lie(built, tmp_path, example):
    r = subprocess.run(["gcc", "-I", INC, os.path.join(REF_EXAMPLES, example), "-o", str(tmp_path / "example"),
                        "-L", os.path.join(ROOT, "primme_amd"), "-lprimme_amd", "-Wl,-rpath," + os.path.join(ROOT, "primme_amd"),
                        "-Wl,--no-undefined", "-lm"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0 and "undefined" not in r.stdout, r.stdout
    assert os.path.exists(tmp_path / "example")          # built, not run: the solve needs the device


PROBE = '#include "primme.h"\n#include <stdio.h>\nint main(void) { PRIMME_INT n = PRIMME_INT_MAX; printf("%" PRIMME_INT_P " %d.%d %d\\n", ' \
        'n, PRIMME_VERSION_MAJOR, PRIMME_VERSION_MINOR, (int)sizeof(PRIMME_COMPLEX_DOUBLE) + PRIMME_FUNCTION_UNAVAILABLE); return 0; }\n'


@pytest.mark.parametrize("compiler, suffix, flags, expect", [
    ("gcc", "c", [], "9223372036854775807 3.2 -28"), ("g++", "cpp", [], "9223372036854775807 3.2 -28"),
    ("gcc", "c", ["-DPRIMME_INT_SIZE=32"], "2147483647 3.2 -28"), ("gcc", "c", ["-DPRIMME_INT_SIZE=0"], "2147483647 3.2 -28")])
def test_primme_h_alone(tmp_path, compiler, suffix, flags, expect):
    src = tmp_path / ("probe." + suffix)
    src.write_text(PROBE)
    subprocess.check_call([compiler, "-Wall", "-Werror", "-pedantic", "-I", INC] + flags + [str(src), "-o", str(tmp_path / "probe")])
    assert subprocess.check_output([str(tmp_path / "probe")], text=True).strip() == expect


def test_primme_amd_h_before_primme_h_and_the_forwarders(tmp_path):
    for first in ("primme_amd.h", "primme_eigs.h", "primme_svds.h"):
        src = tmp_path / "order.c"
        src.write_text(f'#include "{first}"\n' + PROBE)
        subprocess.check_call(["gcc", "-Wall", "-Werror", "-pedantic", "-fsyntax-only", "-I", INC, str(src)])
    codes = tmp_path / "codes.c"
    codes.write_text('#include "primme.h"\n#include <stdio.h>\nint main(void) { printf("%d %d %d %d %d %d %d %d\\n", PRIMME_UNEXPECTED_FAILURE, '
                     'PRIMME_MALLOC_FAILURE, PRIMME_MAIN_ITER_FAILURE, PRIMME_LAPACK_FAILURE, PRIMME_USER_FAILURE, '
                     'PRIMME_ORTHO_CONST_FAILURE, PRIMME_PARALLEL_FAILURE, PRIMME_FUNCTION_UNAVAILABLE); return 0; }\n')
    subprocess.check_call(["gcc", "-I", INC, str(codes), "-o", str(tmp_path / "codes")])
    assert subprocess.check_output([str(tmp_path / "codes")], text=True).split() == ["-1", "-2", "-3", "-40", "-41", "-42", "-43", "-44"]
