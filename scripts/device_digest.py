#!/usr/bin/env python3
"""Per-kernel digest of the gfx950 device code of every .hip file under primme_amd/csrc.

For a refactor that must not move a device instruction: run it on both trees and diff the two lists.

   python scripts/device_digest.py [-j JOBS] [--root TREE] > digest.txt

Every translation unit is compiled with the Makefile's own command line plus --cuda-device-only, the gfx950 code
object is taken out of the bundle, and one line per kernel is printed, sorted by name over all units:

   name  vgpr_count  sgpr_count  group_segment_fixed_size  private_segment_fixed_size  instructions  sha256[:16]

The hash is over the disassembled instruction text of the function (up to its symbol size: no alignment padding)
without addresses and encodings and without the function index of local labels (.LBB12_3 -> .LBB_3).  A kernel that
two units define shows up twice.
"""
import argparse
import concurrent.futures
import hashlib
import os
import re
import subprocess
import sys
import tempfile
import time

ROCM = os.environ.get("ROCM", "/opt/rocm")
LLVM = os.path.join(ROCM, "llvm", "bin")
TARGET = "hipv4-amdgcn-amd-amdhsa--gfx950"
FIELDS = (".vgpr_count", ".sgpr_count", ".group_segment_fixed_size", ".private_segment_fixed_size")


def run(cmd, **kw):
    return subprocess.run(cmd, check=True, stdout=subprocess.PIPE, universal_newlines=True, **kw).stdout


def kernel_notes(obj):
    """{name: [the FIELDS]} from the amdhsa.kernels list of the code object's metadata note."""
    lines = run([os.path.join(LLVM, "llvm-readelf"), "--notes", obj]).splitlines()
    out, i = {}, 0
    while i < len(lines) and lines[i].strip() != "amdhsa.kernels:":
        i += 1
    i += 1
    if i >= len(lines):
        return out
    item = re.match(r"^(\s*)- ", lines[i])
    if not item:
        return out                                  # a code object without kernels
    indent = len(item.group(1))
    cur = None
    for ln in lines[i:]:
        if len(ln) - len(ln.lstrip()) < indent and ln.strip():
            break                                   # the next top-level key of the note
        if ln.startswith(" " * indent + "- "):
            cur = {}
            ln = " " * (indent + 2) + ln[indent + 2:]
        m = re.match(r"^ {%d}(\.[a-z_]+):\s*(.*)$" % (indent + 2), ln)
        if m and cur is not None:
            cur[m.group(1)] = m.group(2).strip().strip("'\"")
            if ".name" in cur and all(f in cur for f in FIELDS):
                out[cur[".name"]] = [cur[f] for f in FIELDS]
    return out


def kernel_text(obj):
    """{symbol: [instruction lines]} from the disassembly, each function cut at its symbol size (what follows is padding
    up to the next function's alignment, which depends on the neighbours in the unit)."""
    end = {}
    for ln in run([os.path.join(LLVM, "llvm-objdump"), "-t", obj]).splitlines():
        m = re.match(r"^([0-9a-f]+) .* F \.text\s+([0-9a-f]+) (?:\.\w+ )?(\S+)$", ln)
        if m:
            end[m.group(3)] = int(m.group(1), 16) + int(m.group(2), 16)
    text = run([os.path.join(LLVM, "llvm-objdump"), "-d", obj])
    out, cur, stop = {}, None, 0
    for ln in text.splitlines():
        m = re.match(r"^[0-9a-f]+ <(.+)>:$", ln)
        if m:
            cur, stop = out.setdefault(m.group(1), []), end.get(m.group(1), 0)
            continue
        a = re.search(r"// ([0-9A-F]+):", ln)
        if cur is None or not a or int(a.group(1), 16) >= stop:
            continue
        ins = ln.split("//")[0].strip()
        ins = re.sub(r"\.LBB\d+_", ".LBB_", ins)
        cur.append(re.sub(r"\s+", " ", ins))
    return out


def digest_unit(args):
    csrc, name, tmp = args
    stem = name[:-4]
    line = [l for l in run(["make", "-C", csrc, "-n", "-B", stem + ".o"]).splitlines() if " -c " in l][-1]
    bundle, obj = os.path.join(tmp, stem + ".bundle"), os.path.join(tmp, stem + ".gfx950.o")
    cmd = line.replace("-o %s.o" % stem, "--cuda-device-only -o %s" % bundle)
    t0 = time.time()
    subprocess.run(cmd, shell=True, check=True, cwd=csrc)
    sys.stderr.write("%s: device code compiled in %.0f s\n" % (name, time.time() - t0))
    subprocess.run([os.path.join(LLVM, "clang-offload-bundler"), "--unbundle", "--type=o", "--targets=" + TARGET,
                    "--input=" + bundle, "--output=" + obj], check=True)
    notes, text = kernel_notes(obj), kernel_text(obj)
    rows = []
    for k, res in notes.items():
        ins = text[k]
        rows.append("%s %s %d %s" % (k, " ".join(res), len(ins), hashlib.sha256("\n".join(ins).encode()).hexdigest()[:16]))
    return rows


def main():
    here = os.path.dirname(os.path.abspath(__file__))
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("-j", type=int, default=4, help="translation units compiled at a time")
    ap.add_argument("--root", default=os.path.dirname(here), help="repository tree to digest (default: this one)")
    a = ap.parse_args()
    csrc = os.path.join(a.root, "primme_amd", "csrc")
    units = sorted(f for f in os.listdir(csrc) if f.endswith(".hip"))
    with tempfile.TemporaryDirectory() as tmp, concurrent.futures.ThreadPoolExecutor(a.j) as pool:
        rows = [r for unit in pool.map(digest_unit, [(csrc, u, tmp) for u in units]) for r in unit]
    sys.stdout.write("\n".join(sorted(rows)) + "\n")


if __name__ == "__main__":
    main()
