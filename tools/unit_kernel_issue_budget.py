#!/usr/bin/env python3
"""Static issue budget of one kernel instantiation (by default unit_fast_kernel): instructions per region of its gfx950 listing.

The unit kernel is paced by instruction issue (profiles/NOTES.md, round 12), so what a change saves can be read off the
compiler's listing before anything runs.  This tool compiles csrc/sann_fast.hip to a device listing with the Makefile's
flags (no GPU needed), picks one instantiation by its template arguments, splits it at its workgroup barriers in PROGRAM
order (the listing's order: a region may hold code of branches a unit does not take) and counts per region

  vector      mnemonics that start with v_
  mul         of those: v_mul_lo_u32, v_mul_hi_u32, v_mad_u64_u32 (quarter rate)
  cmp64       of those: v_cmp* / v_cmpx* on 64-bit integers (_i64, _u64)
  scalar      mnemonics that start with s_ (the barrier itself is counted in the region it ends)
  lds         mnemonics that start with ds_
  global      mnemonics that start with global_, flat_, buffer_ or scratch_

It classifies by mnemonic prefix and those few names only.  It is a report, not a gate.

Other kernels of the step are read the same way: --kernel NAME picks the function template, --source FILE.hip the file of
csrc/ that is compiled, e.g.
  --source sann_kernels.hip --kernel merge_kernel --args 512,1728
  --source sann_kernels.hip --kernel merge_wave_kernel --args 4,8
  --kernel desc_query_kernel --args 1                          (the descriptor kernel lives in sann_fast.hip)

usage: unit_kernel_issue_budget.py [--kernel NAME] [--source FILE.hip] [--args 128,12,64,0,false,true] [--listing FILE.s] [--keep FILE.s]
       unit_kernel_issue_budget.py [--kernel NAME] [--args ...] --compare OLD.s NEW.s
"""
import argparse
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "the-algorithm_amd", "csrc")
COLUMNS = ("vector", "mul", "cmp64", "scalar", "lds", "global")
MULS = ("v_mul_lo_u32", "v_mul_hi_u32", "v_mad_u64_u32")
DEFAULT_ARGS = "128,12,64,0,false,true"
DEFAULT_KERNEL = "unit_fast_kernel"
DEFAULT_SOURCE = "sann_fast.hip"


def mangled_args(args):
    """'128,12,64,0,false,true' -> 'ILi128ELi12ELi64ELi0ELb0ELb1EE', the Itanium spelling inside the kernel's symbol."""
    out = []
    for a in args.replace(" ", "").split(","):
        if a in ("true", "false"):
            out.append("Lb%dE" % (a == "true"))
        else:
            out.append("Li%dE" % int(a))
    return "I" + "".join(out) + "E"


def classify(mnemonic):
    """-> the columns one instruction counts in"""
    if mnemonic.startswith("v_"):
        cols = ["vector"]
        if mnemonic.startswith(MULS):
            cols.append("mul")
        if re.match(r"v_cmpx?_\w+_[iu]64", mnemonic):
            cols.append("cmp64")
        return cols
    if mnemonic.startswith("s_"):
        return ["scalar"]
    if mnemonic.startswith("ds_"):
        return ["lds"]
    if mnemonic.startswith(("global_", "flat_", "buffer_", "scratch_")):
        return ["global"]
    return []


def parse_listing(text, kernel=DEFAULT_KERNEL, args=DEFAULT_ARGS):
    """-> [ {column: count} per region ], regions split at s_barrier, of the function whose symbol holds the kernel's name
    followed by the mangled template arguments.  Raises LookupError if the listing has no such function."""
    want = kernel + mangled_args(args)
    regions, inside = None, False
    for line in text.splitlines():
        s = line.strip()
        if not inside:
            if want in s and re.match(r"^[A-Za-z_.$][\w.$]*:", s):
                inside, regions = True, [dict.fromkeys(COLUMNS, 0)]
            continue
        if s.startswith(".Lfunc_end"):
            break
        if not s or s[0] in ".;" or s.endswith(":") or re.match(r"^[\w.$]+:\s*(;.*)?$", s):
            continue  # directives, comments, labels
        mnemonic = s.split()[0]
        for c in classify(mnemonic):
            regions[-1][c] += 1
        if mnemonic == "s_barrier":
            regions.append(dict.fromkeys(COLUMNS, 0))
    if regions is None:
        raise LookupError("no function %s in the listing" % want)
    return regions


def totals(regions):
    return {c: sum(r[c] for r in regions) for c in COLUMNS}


def makefile_flags():
    """HIPFLAGS of csrc/Makefile, ARCH filled in"""
    arch, flags = "gfx950", None
    for line in open(os.path.join(CSRC, "Makefile")):
        m = re.match(r"ARCH \?= (\S+)", line)
        if m:
            arch = m.group(1)
        m = re.match(r"HIPFLAGS \?= (.*)", line)
        if m:
            flags = m.group(1)
    return flags.replace("$(ARCH)", arch).split()


def compile_listing(out_path, source=DEFAULT_SOURCE):
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    subprocess.run([hipcc] + makefile_flags() + ["-S", "--cuda-device-only", "-w", "-o", out_path, source], check=True, cwd=CSRC)


def table(regions):
    rows = [("region",) + COLUMNS]
    for i, r in enumerate(regions):
        rows.append(("%d" % i,) + tuple(str(r[c]) for c in COLUMNS))
    t = totals(regions)
    rows.append(("total",) + tuple(str(t[c]) for c in COLUMNS))
    return rows


def show(rows):
    w = [max(len(r[i]) for r in rows) for i in range(len(rows[0]))]
    for r in rows:
        print("  ".join(x.rjust(w[i]) for i, x in enumerate(r)))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--args", default=DEFAULT_ARGS, help="template arguments of the instantiation: WG,U,NS,ABL,NORMS,IDF[,...]")
    ap.add_argument("--kernel", default=DEFAULT_KERNEL, metavar="NAME", help="the kernel template's name (default %(default)s)")
    ap.add_argument("--source", default=DEFAULT_SOURCE, metavar="FILE.hip", help="the file of csrc/ to compile (default %(default)s)")
    ap.add_argument("--listing", help="read this listing instead of compiling the source file")
    ap.add_argument("--keep", help="compile and keep the listing here")
    ap.add_argument("--compare", nargs=2, metavar=("OLD.s", "NEW.s"))
    ap.add_argument("--new-args", help="with --compare: the instantiation's arguments in NEW.s, where they differ")
    a = ap.parse_args()
    if a.compare:
        old = parse_listing(open(a.compare[0]).read(), kernel=a.kernel, args=a.args)
        new = parse_listing(open(a.compare[1]).read(), kernel=a.kernel, args=a.new_args or a.args)
        print(a.kernel + "<%s> -> <%s>: old / new per region (regions are split at s_barrier, in program order)" % (a.args, a.new_args or a.args))
        rows = [("region",) + COLUMNS]
        empty = dict.fromkeys(COLUMNS, 0)
        for i in range(max(len(old), len(new))):
            o, n = (old[i] if i < len(old) else empty), (new[i] if i < len(new) else empty)
            rows.append(("%d" % i,) + tuple("%d / %d" % (o[c], n[c]) for c in COLUMNS))
        to, tn = totals(old), totals(new)
        rows.append(("total",) + tuple("%d / %d" % (to[c], tn[c]) for c in COLUMNS))
        rows.append(("delta",) + tuple("%+d" % (tn[c] - to[c]) for c in COLUMNS))
        show(rows)
        return 0
    if a.listing:
        text = open(a.listing).read()
    else:
        path = a.keep or os.path.join(tempfile.mkdtemp(), os.path.splitext(os.path.basename(a.source))[0] + ".s")
        compile_listing(path, a.source)
        text = open(path).read()
    print(a.kernel + "<%s>: instructions per region (regions are split at s_barrier, in program order)" % a.args)
    show(table(parse_listing(text, kernel=a.kernel, args=a.args)))
    return 0


if __name__ == "__main__":
    sys.exit(main())
