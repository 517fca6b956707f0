#!/usr/bin/env python3
"""Does every kernel that exists at a base revision still compile to the same instruction stream?  CPU only.

  python tools/isa_unchanged.py --base REV [--keep DIR]      (REV: the commit to compare with, e.g. the parent of a change)

Checks out REV into a temporary `git worktree`, compiles every .hip of the Makefile's SRCS to gfx950 device assembly
with tools/kernel_resources.py's flags, for the base and for the working tree, and compares the body of every function symbol present
in both (from its label to its .Lfunc_end marker; block and temporary label numbers, which shift when a translation unit gains a
function, are normalised).  Prints one line per translation unit and exits 1 if any shared symbol's body differs.  Symbols only in the
working tree are listed as new.
"""
import argparse
import os
import re
import shutil
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from kernel_resources import FLAGS, demangle  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REL_CSRC = os.path.join("spectrogram_rs_amd", "csrc")


def sources(csrc):
    mk = open(os.path.join(csrc, "Makefile")).read()
    return [f for f in re.search(r"^SRCS\s*:=\s*(.*)$", mk, re.M).group(1).split() if f.endswith(".hip")]


def device_asm(csrc, f):
    r = subprocess.run(["/opt/rocm/bin/hipcc", *FLAGS, "-S", "--cuda-device-only", "-o", "-", os.path.join(csrc, f)],
                       capture_output=True, text=True, cwd=csrc)
    if r.returncode != 0:
        raise RuntimeError("%s: %s" % (f, r.stderr[-2000:]))
    return r.stdout


def bodies(asm):
    out = {}
    for m in re.finditer(r"^\t\.type\t(\S+),@function\n(.*?)^\.Lfunc_end\d+:", asm, re.S | re.M):
        name, text = m.group(1), m.group(2)
        start = text.find("\n%s:" % name)
        body = text[start:] if start >= 0 else text
        body = re.sub(r"[ \t]*;.*$", "", body, flags=re.M)   # comments (they name blocks by function number)
        body = re.sub(r"\.LBB\d+_(\d+)", r".LBB_\1", body)
        body = re.sub(r"\.Ltmp\d+", ".Ltmp", body)
        out[name] = body
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--base", required=True, help="the revision whose kernels must be unchanged (e.g. HEAD~1 once the change is committed)")
    ap.add_argument("--keep", help="write both assemblies of every translation unit here")
    ap.add_argument("-j", type=int, default=8)
    a = ap.parse_args()

    tmp = tempfile.mkdtemp(prefix="isa_base_")
    wt = os.path.join(tmp, "base")
    subprocess.run(["git", "-C", ROOT, "worktree", "add", "--detach", "--quiet", wt, a.base], check=True)
    try:
        rev = subprocess.run(["git", "-C", wt, "rev-parse", "--short", "HEAD"], capture_output=True, text=True).stdout.strip()
        base_csrc, new_csrc = os.path.join(wt, REL_CSRC), os.path.join(ROOT, REL_CSRC)
        files = sources(new_csrc)
        base_files = set(sources(base_csrc))
        jobs = [(base_csrc, f) for f in files if f in base_files] + [(new_csrc, f) for f in files]
        with ThreadPoolExecutor(a.j) as ex:
            asms = dict(zip(jobs, ex.map(lambda j: device_asm(*j), jobs)))
    finally:
        subprocess.run(["git", "-C", ROOT, "worktree", "remove", "--force", wt])
        shutil.rmtree(tmp, ignore_errors=True)

    print("base %s against the working tree (%s)" % (rev, " ".join(FLAGS)))
    failed, n_same, new_names = [], 0, []
    for f in files:
        new = bodies(asms[(new_csrc, f)])
        old = bodies(asms[(base_csrc, f)]) if f in base_files else {}
        if a.keep:
            os.makedirs(a.keep, exist_ok=True)
            for tag, key in (("base", (base_csrc, f)), ("new", (new_csrc, f))):
                if key in asms:
                    open(os.path.join(a.keep, "%s.%s.s" % (f, tag)), "w").write(asms[key])
        shared = sorted(set(old) & set(new))
        diff = [n for n in shared if old[n] != new[n]]
        gone = sorted(set(old) - set(new))
        added = sorted(set(new) - set(old))
        n_same += len(shared) - len(diff)
        failed += [(f, n) for n in diff + gone]
        new_names += added
        print("%-24s %3d shared, %3d identical, %3d differ, %3d gone, %3d new" % (f, len(shared), len(shared) - len(diff), len(diff), len(gone), len(added)))
    names = demangle([n for _, n in failed] + new_names)
    for f, n in failed:
        print("CHANGED or GONE  %s  %s" % (f, names[n][:160]))
    for n in new_names:
        print("new  %s" % names[n][:160])
    print("%d pre-existing function bodies identical, %d changed or gone" % (n_same, len(failed)))
    return 1 if failed else 0


if __name__ == "__main__":
    sys.exit(main())
