#!/usr/bin/env python3
"""Compare the gfx950 kernels of two builds of a kernel source: same set, same resources, same instruction stream.

For a refactor of a kernel file that must leave every kernel as it was.  Build both sides with the library's flags plus

    hipcc <flags> -S --cuda-device-only -Rpass-analysis=kernel-resource-usage FILE.hip -o FILE.s 2> FILE.remarks

and run

    python tools/kernel_isa_diff.py --parent a.s [b.s ..] --branch c.s [d.s ..] [--dropped SUBSTRING ..] [--markdown]

Each .s is read together with the .remarks next to it (same path, other suffix).  A side may be several files (a source that
was split).  Kernels are matched by demangled name.  For every matched kernel the resource figures of the remarks must be equal
and the instruction streams - what is left of the function's text when comments, labels, directives and blank lines are
stripped and the function's number is taken out of its local labels (and the file-wide one out of a long branch's `.Lpost_getpc`
anchor, which follows the order in which the file's kernels are emitted) - are compared as text.  A kernel whose stream differs is
listed with its instruction counts per class on both sides.  --dropped names kernels (a substring of the demangled name) that
the branch removes on purpose; any other missing or added kernel is a failure.  Exit status 0: nothing differs.
"""
import argparse
import difflib
import os
import re
import subprocess
import sys

FIELDS = ["VGPRs", "AGPRs", "TotalSGPRs", "SGPRs Spill", "VGPRs Spill", "ScratchSize [bytes/lane]", "LDS Size [bytes/block]",
          "Occupancy [waves/SIMD]"]
CLASSES = ["v_mfma", "v_pk_", "v_ (other)", "ds_", "buffer_/global_", "s_waitcnt", "s_barrier", "other"]


def demangle(names):
    tool = next((t for t in ("/opt/rocm/llvm/bin/llvm-cxxfilt", "llvm-cxxfilt", "c++filt")
                 if subprocess.run(["sh", "-c", "command -v " + t], capture_output=True).returncode == 0), None)
    if not tool or not names:
        return {n: n for n in names}
    out = subprocess.run([tool], input="\n".join(names), capture_output=True, text=True, check=True).stdout.split("\n")
    return dict(zip(names, out))


def read_remarks(path):
    res, cur = {}, None
    for line in open(path, errors="replace"):
        m = re.search(r"remark:\s+(.*?)\s+\[-Rpass-analysis=kernel-resource-usage\]", line)
        if not m:
            continue
        key, _, val = m.group(1).partition(": ")
        if key == "Function Name":
            cur = res.setdefault(val, {})
        elif cur is not None:
            cur[key.strip()] = val.strip()
    return res


def read_streams(path):
    """mangled kernel name -> list of instructions"""
    text = open(path, errors="replace").read().split("\n")
    kernels = set(re.findall(r"^\s*\.amdhsa_kernel\s+(\S+)", "\n".join(text), flags=re.M))
    out, cur = {}, None
    for line in text:
        m = re.match(r"^([A-Za-z_$][\w$.]*):", line)
        if m and m.group(1) in kernels:
            cur = out.setdefault(m.group(1), [])
            continue
        if cur is None:
            continue
        if re.match(r"^\.Lfunc_end\d+:", line):
            cur = None
            continue
        code = line.split(";")[0].strip()
        if not code or code.startswith(".") or code.endswith(":"):
            continue
        code = re.sub(r"\.L(BB|JTI|tmp)\d+_", r".L\1_", re.sub(r"\s+", " ", code))
        # the anchor label of a long branch is numbered through the whole file, in the order the kernels are emitted
        cur.append(re.sub(r"\.Lpost_getpc\d+", ".Lpost_getpc", code))
    return out


def classify(ins):
    op = ins.split(" ")[0]
    if op.startswith("v_mfma"):
        return "v_mfma"
    if op.startswith("v_pk_"):
        return "v_pk_"
    if op.startswith("v_"):
        return "v_ (other)"
    if op.startswith("ds_"):
        return "ds_"
    if op.startswith(("buffer_", "global_")):
        return "buffer_/global_"
    if op in ("s_waitcnt", "s_barrier"):
        return op
    return "other"


def counts(stream):
    c = dict.fromkeys(CLASSES, 0)
    for ins in stream:
        c[classify(ins)] += 1
    return c


def side(paths):
    res, streams = {}, {}
    for p in paths:
        rem = os.path.splitext(p)[0] + ".remarks"
        for k, v in read_remarks(rem).items():
            res[k] = v
        for k, v in read_streams(p).items():
            if k in streams:
                sys.exit("kernel %s is defined twice on one side" % k)
            streams[k] = v
    names = demangle(sorted(streams))
    return ({names[k]: res.get(k, {}) for k in streams}, {names[k]: v for k, v in streams.items()})


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--parent", nargs="+", required=True)
    ap.add_argument("--branch", nargs="+", required=True)
    ap.add_argument("--dropped", nargs="*", default=[], help="kernels the branch removes on purpose (substring of the demangled name)")
    ap.add_argument("--markdown", action="store_true", help="print the per-kernel table")
    ap.add_argument("--show-diff", type=int, default=0, metavar="N", help="print the first N lines of each differing stream's diff")
    a = ap.parse_args()
    pres, pstr = side(a.parent)
    bres, bstr = side(a.branch)
    missing = sorted(k for k in pstr if k not in bstr)
    expected = [k for k in missing if any(d in k for d in a.dropped)]
    missing = [k for k in missing if k not in expected]
    added = sorted(k for k in bstr if k not in pstr)
    bad_res, bad_stream, rows = [], [], []
    for k in sorted(pstr):
        if k not in bstr:
            continue
        rdiff = [f for f in FIELDS if pres[k].get(f) != bres[k].get(f)]
        same = pstr[k] == bstr[k]
        if rdiff:
            bad_res.append((k, rdiff))
        if not same:
            bad_stream.append(k)
        r = pres[k]
        rows.append("| `%s` | %s | %s | %s | %s / %s | %s | %s | %s | %d | %s | %s |" % (
            k.replace("bvc::", "").replace("(bvc::AmpArgs)", "").replace("(bvc::ConvArgs)", ""), r.get("VGPRs"), r.get("AGPRs"),
            r.get("TotalSGPRs"), r.get("SGPRs Spill"), r.get("VGPRs Spill"), r.get("ScratchSize [bytes/lane]"),
            r.get("LDS Size [bytes/block]"), r.get("Occupancy [waves/SIMD]"), len(pstr[k]),
            "equal" if not rdiff else "DIFFERENT: " + ", ".join(rdiff), "identical" if same else "DIFFERENT"))
    if a.markdown:
        print("| kernel | VGPRs | AGPRs | SGPRs | spills S / V | scratch | LDS | occupancy | instructions | resources, branch | stream, branch |")
        print("|---|---|---|---|---|---|---|---|---|---|---|")
        print("\n".join(rows))
        print()
    print("parent: %d kernels, branch: %d kernels, matched: %d" % (len(pstr), len(bstr), len(rows)))
    print("removed on purpose: %s" % (", ".join(expected) or "none"))
    print("missing from the branch: %s" % (", ".join(missing) or "none"))
    print("added by the branch: %s" % (", ".join(added) or "none"))
    print("resources differ: %d" % len(bad_res))
    for k, f in bad_res:
        print("  %s: %s" % (k, "; ".join("%s %s -> %s" % (x, pres[k].get(x), bres[k].get(x)) for x in f)))
    print("instruction streams differ: %d" % len(bad_stream))
    for k in bad_stream:
        pc, bc = counts(pstr[k]), counts(bstr[k])
        print("  %s" % k)
        print("    " + ", ".join("%s %d -> %d" % (c, pc[c], bc[c]) for c in CLASSES))
        if a.show_diff:
            for line in list(difflib.unified_diff(pstr[k], bstr[k], "parent", "branch", lineterm="", n=2))[:a.show_diff]:
                print("      " + line)
    return 1 if (missing or added or bad_res or bad_stream) else 0


if __name__ == "__main__":
    sys.exit(main())
