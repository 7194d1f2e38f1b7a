"""The _z rename list of primme_amd/csrc/eigs_scalar.h against the symbols the host solver really defines.

The sources that touch coefficient-space data are compiled twice (eigs_X.c as it is, and once more with PA_COMPLEX
through the one-line wrapper eigs_X_z.c); in the complex objects every external function carries the suffix _z, by the
`#define pa_x pa_x_z` list of eigs_scalar.h.  A name missing from the list is a duplicate symbol at link time.  The
other direction is checked here, on the host-only build of the solver (oracle/_build/libprimme_hostcheck.so):

  1. every listed name is defined twice, as pa_x and as pa_x_z (an entry for a function that exists once would
     leave pa_x_z undefined);
  2. every pa_*_z the library defines has its base name on the list;
  3. no complex object defines an external symbol without the suffix.  Checked on objects compiled here: each
     wrapper eigs_X_z.c goes through the command line the product Makefile itself prints for it (make -n), with
     the output path replaced and -O0 appended (which symbols an object defines does not depend on the optimisation
     level: no source uses a non-static inline function), so the check is quick and does not depend on which
     objects a build left behind.
"""
import concurrent.futures
import glob
import os
import re
import subprocess

import pytest

from checkers import HOSTCHECK_LIB

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "primme_amd", "csrc")


def _defined(obj):
    out = subprocess.run(["nm", "--defined-only", "-g", obj], check=True, stdout=subprocess.PIPE, universal_newlines=True).stdout
    return {ln.split()[-1] for ln in out.splitlines() if ln.strip()}


def _rename_list():
    names = []
    with open(os.path.join(CSRC, "eigs_scalar.h")) as f:
        for ln in f:
            m = re.match(r"\s*#define\s+(pa_\w+)\s+(pa_\w+)\s*$", ln)
            if m:
                assert m.group(2) == m.group(1) + "_z", ln
                names.append(m.group(1))
    return names


@pytest.fixture(scope="module")
def symbols(built):
    return _defined(HOSTCHECK_LIB)


def test_list_is_parsed():
    names = _rename_list()
    assert len(names) >= 30 and len(set(names)) == len(names), names


def test_every_listed_name_is_defined_twice(symbols):
    missing = [n for n in _rename_list() for sym in (n, n + "_z") if sym not in symbols]
    assert not missing, "on the _z list of eigs_scalar.h but not defined as both pa_x and pa_x_z: %s" % missing


def test_every_z_symbol_is_listed(symbols):
    listed = set(_rename_list())
    extra = sorted(s for s in symbols if re.match(r"pa_\w+_z$", s) and s[:-2] not in listed)
    assert not extra, "defined with the suffix _z but not on the list of eigs_scalar.h: %s" % extra


def _compile_wrapper(args):
    stem, tmp = args
    lines = subprocess.run(["make", "-C", CSRC, "-n", "-B", stem + ".o"], check=True, stdout=subprocess.PIPE,
                           universal_newlines=True).stdout.splitlines()
    cmd = [ln for ln in lines if " -c " in ln and stem + ".c" in ln][-1]
    obj = os.path.join(tmp, stem + ".o")
    assert "-o %s.o" % stem in cmd, cmd
    subprocess.run(cmd.replace("-o %s.o" % stem, "-O0 -o %s" % obj), shell=True, check=True, cwd=CSRC)
    return stem, _defined(obj)


def test_complex_objects_export_only_z_names(tmp_path):
    stems = sorted(os.path.basename(p)[:-2] for p in glob.glob(os.path.join(CSRC, "eigs_*_z.c")))
    assert len(stems) >= 8, stems
    with concurrent.futures.ThreadPoolExecutor(min(8, len(stems))) as pool:
        results = list(pool.map(_compile_wrapper, [(s, str(tmp_path)) for s in stems]))
    bad = {stem: sorted(s for s in syms if not s.endswith("_z")) for stem, syms in results}
    bad = {k: v for k, v in bad.items() if v}
    assert not bad, "external symbols without the suffix _z in complex objects: %s" % bad
    assert all(syms for _, syms in results), "a complex object defines nothing: %s" % [k for k, v in results if not v]
