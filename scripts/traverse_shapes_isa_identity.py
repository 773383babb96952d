#!/usr/bin/env python3
"""Show that two source trees compile to the same device code: kernel by kernel, the compiler's resource report and the instruction stream.

    python scripts/traverse_shapes_isa_identity.py PARENT_TREE THIS_TREE [SOURCE ...] > report.md

Both trees' sources (api.hip and wavefront.hip unless others are named) are compiled device-side only with the Makefile's flags plus -Rpass-analysis=kernel-resource-usage (no GPU needed), the gfx950 code
objects are disassembled, and every function is paired by its demangled name.  A traverse_kernel spelled with the positional template arguments of before the shape table
(<ANYHIT, COUNT, LEAF_MIN, REFILL_MIN, LDS_DEPTH, NODE_STEPS, INST, MIXED, ALPHA, WPE, ALPHA_MIN, QUADRIC>) is paired with the <Shape, MODE> that has the same values.
Instructions are compared as text without addresses and encodings; the literal of the s_add_u32 behind an s_getpc_b64 (the distance to a callee, a matter of lay-out) is masked
and the s_nop padding behind a function's last instruction is dropped (the order of the functions in the code object may differ).
A function that one tree alone has (a new or a dropped instantiation) is listed with its resources in a table of its own.
Exit status 1 if a function of the parent is missing here or a pair differs in resources or instructions."""
import difflib
import os
import re
import subprocess
import sys
import tempfile

LLVM = os.environ.get("LLVM_BIN", "/opt/rocm/llvm/bin")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
SOURCES = ("api.hip", "wavefront.hip")
FIELDS = ("VGPRs", "TotalSGPRs", "VGPRs Spill", "SGPRs Spill", "ScratchSize [bytes/lane]", "Occupancy [waves/SIMD]", "LDS Size [bytes/block]")

# shape name -> (count, leaf_min, refill_min, lds_depth, node_steps, inst, alpha, wpe, alpha_min, quadric): traverse.h's structs, restated to translate the old spelling
SHAPES = {
    "ph::ShapeFlat": (0, 16, 32, 12, 6, 0, 0, 6, 0, 0),
    "ph::ShapeInst": (0, 24, 12, 11, 5, 1, 0, 5, 0, 0),
    "ph::ShapeFlatAlphaLean": (0, 24, 12, 12, 5, 0, 1, 0, 12, 0),
    "ph::ShapeInstAlphaLean": (0, 16, 12, 11, 5, 1, 1, 5, 12, 0),
    "ph::ShapeAlphaGeneral<false>": (0, 20, 12, 12, 3, 0, 2, 0, 12, 0),
    "ph::ShapeAlphaGeneral<true>": (0, 20, 12, 12, 3, 1, 2, 0, 12, 0),
    "ph::ShapeQuadric": (0, 16, 32, 12, 6, 0, 0, 0, 0, 1),
}
for inst in (0, 1):
    for alpha in (0, 1, 2):
        SHAPES["ph::ShapeCount<%s, %d, false>" % ("true" if inst else "false", alpha)] = (1, 20, 12, 12, 1, inst, alpha, 0, 0, 0)
SHAPES["ph::ShapeCount<false, 0, true>"] = (1, 20, 12, 12, 1, 0, 0, 0, 0, 1)
BY_VALUES = {v: k for k, v in SHAPES.items()}
OLD = re.compile(r"ph::traverse_kernel<((?:\w+, ){11}\w+)>")


def canonical(name):
    """demangled name -> (key both spellings share, the name as it was spelled)"""
    m = OLD.search(name)
    if not m:
        return name, name
    a = [{"true": 1, "false": 0}.get(x, x) for x in m.group(1).split(", ")]
    a = [int(x) for x in a]
    anyhit, count, leaf_min, refill_min, lds_depth, node_steps, inst, mixed, alpha, wpe, alpha_min, quadric = a
    shape = BY_VALUES.get((count, leaf_min, refill_min, lds_depth, node_steps, inst, alpha, wpe, alpha_min, quadric), "(no shape: %s)" % m.group(1))
    mode = 2 if mixed else 1 if anyhit else 0
    return name[:m.start()] + "ph::traverse_kernel<%s, %d>" % (shape, mode) + name[m.end():], "traverse_kernel<%s>" % m.group(1)


def demangle(names):
    out = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True, check=True).stdout.split("\n")
    return dict(zip(names, out))


def build(tree, tmp, tag):
    """-> {canonical name: {"spelled", "res" (kernels only), "isa"}} over both sources"""
    csrc = os.path.join(tree, "pbrt-v3-rs_amd", "csrc")
    flags = re.search(r"^FLAGS = (.*)$", open(os.path.join(csrc, "Makefile")).read(), re.M).group(1).replace("$(ARCH)", "gfx950").replace("$(EXTRA)", "").split()
    funcs = {}
    for src in SOURCES:
        co = os.path.join(tmp, "%s_%s.co" % (tag, src))
        r = subprocess.run([HIPCC] + flags + ["--cuda-device-only", "-Rpass-analysis=kernel-resource-usage", "-c", src, "-o", co], cwd=csrc, capture_output=True, text=True)
        if r.returncode:
            sys.exit(r.stderr)
        res, cur = {}, None
        for line in r.stderr.split("\n"):
            m = re.search(r"remark: +(.*?): (\S+) \[-Rpass-analysis", line)
            if m and m.group(1) == "Function Name":
                cur = res.setdefault(m.group(2), {})
            elif m and cur is not None:
                cur[m.group(1)] = m.group(2)
        subprocess.run([os.path.join(LLVM, "clang-offload-bundler"), "--unbundle", "--type=o", "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", "--input=" + co, "--output=" + co + ".elf"], check=True)
        text = subprocess.run([os.path.join(LLVM, "llvm-objdump"), "-d", co + ".elf"], capture_output=True, text=True, check=True).stdout
        isa, sym = {}, None
        for line in text.split("\n"):
            m = re.match(r"[0-9a-f]+ <(\S+)>:$", line)
            if m:
                sym = isa.setdefault(m.group(1), [])
            elif sym is not None and line.startswith("\t"):
                ins = re.sub(r"\s+", " ", line.split("//")[0].strip())
                if sym and sym[-1].startswith("s_getpc_b64") and ins.startswith("s_add_u32"):
                    ins = re.sub(r"0x[0-9a-f]+$", "<pc-relative>", ins)
                sym.append(ins)
        for sym in isa.values():   # the padding up to the next function's alignment belongs to neither
            while sym and sym[-1] in ("s_nop 0", "..."):
                sym.pop()
        names = demangle(sorted(set(res) | set(isa)))
        for mangled in isa:
            key, spelled = canonical(names[mangled])
            funcs["%s: %s" % (src, key)] = {"spelled": spelled, "res": res.get(mangled), "isa": isa[mangled]}
    return funcs


def n_differing(a, b):
    return sum(max(i2 - i1, j2 - j1) for op, i1, i2, j1, j2 in difflib.SequenceMatcher(None, a, b, autojunk=False).get_opcodes() if op != "equal")


def main():
    global SOURCES
    parent_tree, this_tree = sys.argv[1], sys.argv[2]
    SOURCES = tuple(sys.argv[3:]) or SOURCES
    with tempfile.TemporaryDirectory() as tmp:
        parent, this = build(parent_tree, tmp, "parent"), build(this_tree, tmp, "this")
    bad = 0
    only = sorted(set(parent) ^ set(this))
    trav = [k for k in parent if "traverse_kernel" in k]
    print("# Device code, parent against this tree\n")
    print("`scripts/traverse_shapes_isa_identity.py`: %s compiled device-side for gfx950 with the Makefile's flags and `-Rpass-analysis=kernel-resource-usage`, both code objects disassembled"
          " with `llvm-objdump -d`, functions paired by demangled name (a positionally spelled `traverse_kernel` with the shape that has its values)."
          "  \"differing\" counts instructions that are not common to both streams (addresses and encodings dropped, the pc-relative literal of a call masked, padding between functions dropped).\n" % " and ".join("`%s`" % s for s in SOURCES))
    print("Functions: %d in the parent, %d here; `traverse_kernel` instantiations: %d in the parent, %d here; in one tree only: %s.\n"
          % (len(parent), len(this), len(trav), sum("traverse_kernel" in k for k in this), ", ".join("`%s`" % k for k in only) or "none"))
    gone = [k for k in only if k in parent]   # a function this tree alone has is an addition, listed below with its resources; one the parent alone has is a difference
    bad += len(gone)
    print("| function (this tree's spelling) | parent's spelling | " + " | ".join(f.split(" [")[0] for f in FIELDS) + " | instructions | differing |")
    print("|---|---|" + "---|" * (len(FIELDS) + 2))
    for k in sorted(set(parent) & set(this), key=lambda k: ("traverse_kernel" not in k, k)):
        p, t = parent[k], this[k]
        cells = []
        for f in FIELDS:
            a, b = (p["res"] or {}).get(f, "-"), (t["res"] or {}).get(f, "-")
            cells.append(a if a == b else "**%s -> %s**" % (a, b))
            bad += a != b
        d = 0 if p["isa"] == t["isa"] else n_differing(p["isa"], t["isa"])
        bad += d != 0
        print("| `%s` | %s | %s | %d | %s |" % (k, "`%s`" % p["spelled"] if p["spelled"] != k.split(": ", 1)[1] else "same", " | ".join(cells), len(t["isa"]), d if d == 0 else "**%d**" % d))
    if only:   # a function one tree alone has: its resources, so that a new instantiation is listed with what it costs
        print("\nIn one tree only:\n")
        print("| function | tree | " + " | ".join(f.split(" [")[0] for f in FIELDS) + " | instructions |")
        print("|---|---|" + "---|" * (len(FIELDS) + 1))
        for k in only:
            f1 = parent.get(k) or this[k]
            print("| `%s` | %s | %s | %d |" % (k, "parent" if k in parent else "this", " | ".join((f1["res"] or {}).get(f, "-") for f in FIELDS), len(f1["isa"])))
    added = len(only) - len(gone)
    print("\n%s%s" % ("Every pair has the same resources and the same instructions." if not bad else "%d differences (bold above; functions the parent alone has count)." % bad,
                      "  %d functions are new in this tree." % added if added else ""))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
