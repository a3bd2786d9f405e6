#!/usr/bin/env python3
"""Is the device code of this tree the device code of another one?  (No GPU involved.)

    tools/code_object_identity.py PARENT_TREE [--out FILE]

PARENT_TREE is a checkout of the commit to compare against, made locally from git (`git worktree add DIR REV`, or
`git archive REV | tar -x -C DIR`).  Every source of _build.SOURCES is compiled for gfx950 from both trees with the flags of the
build (_build.FLAGS + _build.SOURCE_FLAGS) plus --cuda-device-only --no-gpu-bundle-output, at most eight compiles at a time, and the
two code objects are compared by `llvm-objdump -d` (without the line that names the file) and `llvm-readelf --notes`: the
instructions of every kernel, and its name, arguments, registers, LDS and scratch.  (The code objects themselves always differ, in
the symbol __hip_cuid_<hash of the translation unit's source>.)  The texts are hashed and compared, nothing else is done with them.

Prints one line per source -- lines and sha256 of both texts -- and exits non-zero when any of them differs.  This is the proof a
refactor of the kernel sources owes: profiles/field_launch_identity.txt and profiles/mfma_headers_identity.txt are its output.
"""
import argparse
import concurrent.futures
import hashlib
import importlib.util
import os
import shutil
import subprocess
import sys
import tempfile

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = "reflect_sampling_nerf_amd"


def _load_build():
    spec = importlib.util.spec_from_file_location("_rsn_build", os.path.join(REPO, PKG, "_build.py"))  # not the package: no torch
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _tool(hipcc, name):
    rocm = os.path.dirname(os.path.dirname(os.path.realpath(hipcc)))
    for cand in (shutil.which(name), os.path.join(rocm, "llvm", "bin", name), os.path.join(rocm, "lib", "llvm", "bin", name)):
        if cand and os.path.exists(cand):
            return cand
    raise SystemExit("%s not found beside %s" % (name, hipcc))


def _texts(hipcc, objdump, readelf, tree, src, flags, out):
    """(disassembly, notes) of `src` compiled from `tree`, each as a list of lines."""
    csrc = os.path.join(tree, PKG, "csrc")
    cmd = [hipcc, *flags, "--cuda-device-only", "--no-gpu-bundle-output", "-I", os.path.join(tree, "include"), "-I", csrc, "-c",
           os.path.join(csrc, src), "-o", out]
    res = subprocess.run(cmd, capture_output=True, text=True)
    if res.returncode != 0:
        raise RuntimeError("hipcc failed on %s of %s:\n%s%s" % (src, tree, res.stdout, res.stderr))
    dis = subprocess.run([objdump, "-d", out], capture_output=True, text=True, check=True).stdout.splitlines()
    notes = subprocess.run([readelf, "--notes", out], capture_output=True, text=True, check=True).stdout.splitlines()
    return [ln for ln in dis if out not in ln], [ln for ln in notes if out not in ln]


def _sha(lines):
    return hashlib.sha256("\n".join(lines).encode()).hexdigest()[:16]


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("parent_tree")
    ap.add_argument("--out", help="also write the table to this file")
    args = ap.parse_args()
    parent = os.path.abspath(args.parent_tree)
    build = _load_build()
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    objdump, readelf = _tool(hipcc, "llvm-objdump"), _tool(hipcc, "llvm-readelf")
    rows, differ = [], []
    with tempfile.TemporaryDirectory() as tmp, concurrent.futures.ThreadPoolExecutor(max_workers=8) as ex:
        futs = {}
        for src in build.SOURCES:
            flags = [*build.FLAGS, *build.SOURCE_FLAGS.get(src, ())]
            for side, tree in (("parent", parent), ("new", REPO)):
                futs[(src, side)] = ex.submit(_texts, hipcc, objdump, readelf, tree, src, flags,
                                              os.path.join(tmp, "%s.%s.co" % (src, side)))
        for src in build.SOURCES:
            (pd, pn), (nd, nn) = futs[(src, "parent")].result(), futs[(src, "new")].result()
            same = pd == nd and pn == nn
            if not same:
                differ.append(src)
            rows.append("%-26s %8s %8s  %s %s   %6s %6s  %s %s  %s" % (src, format(len(pd), ","), format(len(nd), ","), _sha(pd), _sha(nd),
                                                                     format(len(pn), ","), format(len(nn), ","), _sha(pn), _sha(nn),
                                                                     "identical" if same else "DIFFERENT"))
    head = "%-26s %17s  %-33s   %13s  %-33s" % ("source", "disassembly lines", "sha256 (parent, new)", "notes lines", "sha256 (parent, new)")
    tail = "%d of %d translation units identical in disassembly and notes" % (len(rows) - len(differ), len(rows))
    text = "\n".join([head, *rows, tail]) + "\n"
    sys.stdout.write(text)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(text)
    return 1 if differ else 0


if __name__ == "__main__":
    sys.exit(main())
