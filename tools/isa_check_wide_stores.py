#!/usr/bin/env python3
"""A vector-memory store of more than 8 bytes reads its data registers after it issues: a VALU write to them must wait.  gfx940+ asks
for two wait states.  LLVM pads after every such store except a MUBUF store whose soffset is a register, which its hazard model exempts.
On gfx950 such an exempt store was followed at once by a VALU write to its first data register, and that dword came out wrong.  The
complex-row kernels therefore pass soffset 0 and keep the whole offset in voffset, so the compiler pads them.  This script checks the
device assembly: no VALU instruction writes a wide store's data VGPRs within two wait states of it (s_nop N counts N + 1), and no wide
MUBUF store of the named kernels uses a register soffset.

  python tools/isa_check_wide_stores.py [--kernels REGEX] file.s ...     (exit 1 on a finding in a kernel that REGEX matches)

Without --kernels every kernel is checked.  Each kernel is listed with its wide stores and findings.
"""
import argparse
import re
import subprocess
import sys

WIDE = re.compile(r"^\s*(buffer|global|flat|scratch)_store_(dwordx3|dwordx4|b96|b128)\s+(.*)$")
VREG = re.compile(r"^v(\d+)$|^v\[(\d+):(\d+)\]$")
NEED = 2   # wait states


def regs(tok):
    m = VREG.match(tok.strip())
    if not m:
        return set()
    if m.group(1) is not None:
        return {int(m.group(1))}
    return set(range(int(m.group(2)), int(m.group(3)) + 1))


def kernels(asm):
    for m in re.finditer(r"^\t\.type\t(\S+),@function\n(.*?)^\.Lfunc_end\d+:", asm, re.S | re.M):
        yield m.group(1), [l.split(";")[0].rstrip() for l in m.group(2).split("\n")]


def instructions(lines):
    return [l.strip() for l in lines if l.strip() and not l.strip().startswith((".", "#")) and not l.strip().endswith(":")]


def check(ins):
    stores, findings = 0, []
    for i, l in enumerate(ins):
        m = WIDE.match(l)
        if not m:
            continue
        stores += 1
        ops = [o.strip() for o in m.group(3).split(",")]
        # buffer: vdata, vaddr, srsrc, soffset ...; global / flat / scratch: vaddr, vdata, ...
        data = regs(ops[0] if m.group(1) == "buffer" else ops[1])
        if m.group(1) == "buffer" and len(ops) > 3 and re.match(r"^s\d+$|^s\[\d+:\d+\]$|^(vcc|m0|exec)", ops[3].split()[0]):
            findings.append("register soffset (%s): %s" % (ops[3].split()[0], l))
        waits = 0
        for nxt in ins[i + 1:]:
            if waits >= NEED:
                break
            op = nxt.split()[0]
            if op.startswith("v_"):
                dst = nxt[len(op):].split(",")[0]
                if regs(dst) & data:
                    findings.append("VALU write of the data %d wait state(s) after: %s  ->  %s" % (waits, l, nxt))
                    break
            if op in ("s_branch", "s_endpgm", "s_setpc_b64"):
                break
            waits += int(nxt.split()[1]) + 1 if op == "s_nop" else 1
    return stores, findings


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--kernels", default="")
    ap.add_argument("files", nargs="+")
    a = ap.parse_args()
    sel = re.compile(a.kernels)
    bad = 0
    rows = []
    for f in a.files:
        for name, lines in kernels(open(f).read()):
            n, found = check(instructions(lines))
            if n:
                rows.append((name, n, found, bool(sel.search(name))))
    try:
        names = dict(zip([r[0] for r in rows], subprocess.run(["c++filt"], input="\n".join(r[0] for r in rows), capture_output=True,
                                                               text=True).stdout.split("\n")))
    except OSError:   # (no c++filt: mangled names)
        names = {}
    for name, n, found, checked in rows:
        print("%-8s %3d wide stores, %d findings  %s" % ("checked" if checked else "listed", n, len(found), names.get(name, name)[:150]))
        for x in found:
            print("    " + x)
        bad += len(found) if checked else 0
    print("%d finding(s) in checked kernels" % bad)
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
