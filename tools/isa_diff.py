"""Device code of two trees of this repository, kernel by kernel: does a refactor leave the instruction streams alone?

    python tools/isa_diff.py PARENT_TREE NEW_TREE [file.hip ...]        (files of iswm_amd/csrc; default: every .hip of NEW_TREE)

Each file of both trees is compiled for gfx950 with the flags of iswm_amd/build.py plus `--cuda-device-only -S` (no GPU, nothing
is launched).  Per kernel symbol the instruction stream is normalised -- comments and alignment directives dropped, basic-block
labels renumbered in order of appearance, the per-file g_zero_row* / g_dump_* symbol names masked -- and compared:
    identical     equal line by line, register numbers included
    same opcodes  the same opcode sequence, operands (register numbers, immediates) differ
    differs       anything else
followed by the instruction counts and the resource fields of the code-object metadata, parent/new.  A resource field that
is larger in the new tree is marked with `!`.  A kernel left unmatched by mangled symbol (a parameter type was renamed) is paired
by its demangled name without the parameter list when that name is unique in both trees, compared with the mangled names inside
its instruction lines masked, and reported with `(renamed)` appended.  This is the table of profiles/pl2_refactor_isa.txt,
conv_route_refactor_isa.txt, scene_predict_isa.txt and wgrad_refactor_isa.txt.  It compares two trees and nothing else."""
import os
import re
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from iswm_amd.build import FLAGS, _hipcc

FIELDS = (("vgpr", ".vgpr_count"), ("agpr", ".agpr_count"), ("sgpr", ".sgpr_count"), ("scratch", ".private_segment_fixed_size"),
          ("lds", ".group_segment_fixed_size"), ("vspill", ".vgpr_spill_count"), ("sspill", ".sgpr_spill_count"))
MASKED = re.compile(r"\b\w*g_(?:zero_row|dump)\w*")
LABEL = re.compile(r"\.LBB\d+_\d+")
MANGLED = re.compile(r"\b_Z\w+")


def assembly(tree, name, out):
    src = os.path.join(tree, "iswm_amd", "csrc", name)
    cmd = [_hipcc()] + [f for f in FLAGS if f != "-fPIC"] + ["--cuda-device-only", "-S", src, "-o", out]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0:
        raise SystemExit("hipcc failed on %s:\n%s" % (src, r.stderr[-4000:]))
    return open(out).read()


def demangle(symbols):
    try:
        names = subprocess.run(["c++filt"] + symbols, capture_output=True, text=True, check=True).stdout.split("\n")
    except (OSError, subprocess.CalledProcessError):
        names = symbols                                # no demangler: the mangled names serve
    out = {}
    for s, n in zip(symbols, names):
        n = re.sub(r"^void ", "", n)
        depth, cut = 0, len(n)
        for i, ch in enumerate(n):                     # cut the parameter list: the first "(" outside the template arguments
            depth += (ch == "<") - (ch == ">")
            if ch == "(" and depth == 0:
                cut = i
                break
        out[s] = n[:cut].replace("iswm::", "")
    return out


def kernels(text):
    """{mangled kernel symbol: (normalised instruction lines, {field: value})}"""
    meta = {}
    for block in text.split("  - .agpr_count:")[1:]:   # one metadata entry per kernel; .agpr_count is its first key
        block = ".agpr_count:" + block
        sym = re.search(r"^\s*\.symbol:\s*(\S+)\.kd", block, re.M).group(1)
        meta[sym] = dict((k, int(re.search(r"^\s*%s:\s*(\d+)" % re.escape(f), block, re.M).group(1))) for k, f in FIELDS)
    out = {}
    for sym in meta:
        body = text[text.index("\n%s:" % sym) + len(sym) + 2:]
        body = body[:re.search(r"^\.Lfunc_end\d+:", body, re.M).start()]
        labels, lines = {}, []
        for ln in body.split("\n"):
            ln = ln.split(";")[0].strip()
            if not ln or ln.startswith(".p2align") or ln.startswith(".align"):
                continue
            ln = LABEL.sub(lambda m: labels.setdefault(m.group(0), "L%d" % len(labels)), ln)
            lines.append(re.sub(r"\s+", " ", MASKED.sub("G_SYM", ln)))
        out[sym] = (lines, meta[sym])
    return out


def insns(lines):
    return [ln for ln in lines if not ln.endswith(":") and not ln.startswith(".")]


def renamed(a, b, names):
    """{parent symbol: new symbol} of the kernels left unmatched by symbol whose demangled name is unique on both sides"""
    pairs = {}
    for sym in a:
        same = [[t for t in side if names[t] == names[sym]] for side in (a, b)]
        if sym not in b and len(same[0]) == 1 and len(same[1]) == 1 and same[1][0] not in a:
            pairs[sym] = same[1][0]
    return pairs


def compare(name, tmp, parent, new):
    a = kernels(assembly(parent, name, os.path.join(tmp, "a_" + name + ".s")))
    b = kernels(assembly(new, name, os.path.join(tmp, "b_" + name + ".s")))
    return name, a, b


def main(argv):
    if len(argv) < 2:
        raise SystemExit(__doc__)
    parent, new = argv[0], argv[1]
    files = argv[2:] or sorted(f for f in os.listdir(os.path.join(new, "iswm_amd", "csrc")) if f.endswith(".hip"))
    files = [os.path.basename(f) for f in files]
    worse = changed = 0
    print("%-10s %-48s %-13s instructions and resources (parent/new)" % ("file", "kernel", "stream"))
    with tempfile.TemporaryDirectory() as tmp, ThreadPoolExecutor(max_workers=4) as ex:
        for name, a, b in ex.map(lambda f: compare(f, tmp, parent, new), files):
            short = re.sub(r"^conv_|\.hip$", "", name)
            names = demangle(sorted(set(a) | set(b)))
            pairs = renamed(a, b, names)
            for sym in sorted(set(names) - set(pairs.values()), key=names.get):
                if sym not in a or pairs.get(sym, sym) not in b:
                    print("%-10s %-48s %s" % (short, names[sym], "only in parent" if sym in a else "only in new"))
                    changed += 1
                    continue
                (la, ma), (lb, mb) = a[sym], b[pairs.get(sym, sym)]
                if sym in pairs:
                    la, lb = ([MANGLED.sub("Z_SYM", ln) for ln in side] for side in (la, lb))
                ia, ib = insns(la), insns(lb)
                if la == lb:
                    verdict = "identical"
                elif [i.split(" ")[0] for i in ia] == [i.split(" ")[0] for i in ib]:
                    verdict = "same opcodes (%d lines differ)" % sum(x != y for x, y in zip(ia, ib))
                else:
                    verdict = "differs"
                changed += verdict != "identical"
                res = " ".join("%s %d/%d%s" % (k, ma[k], mb[k], "!" if mb[k] > ma[k] else "") for k, _ in FIELDS)
                worse += any(mb[k] > ma[k] for k, _ in FIELDS)
                print("%-10s %-48s %-13s insns %d/%d  %s%s" % (short, names[sym], verdict, len(ia), len(ib), res,
                                                               "  (renamed)" if sym in pairs else ""))
    print("ALL IDENTICAL" if not changed else "%d kernel(s) not identical, %d with a larger resource field" % (changed, worse))


if __name__ == "__main__":
    main(sys.argv[1:])
