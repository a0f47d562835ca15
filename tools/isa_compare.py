#!/usr/bin/env python3
"""Compare the gfx950 code of two trees kernel by kernel (CPU only, no GPU needed).

The check behind a refactor that must not change generated code: every .hip of the
Makefile's SRCS is compiled device-only with the Makefile's flags (the per-file extras such
as -fno-honor-nans included) in the parent tree and in the new one, and for every kernel
the tool reports
  * registers, scratch, LDS and occupancy (-Rpass-analysis=kernel-resource-usage),
  * whether the instruction streams are identical as text (labels renumbered), identical
    only after register names are normalised, or different; then how many instructions
    differ and whether the two streams hold the same instructions in another order.
Normalising replaces every register by its class (v, s, a) and a range by its width, so
"identical after normalising" means the same opcodes in the same order with the same operand
classes: it cannot tell a renumbering from two operands of one class changing places. Such
kernels are counted and listed apart from the identical ones ("register_only").
Kernels that the sources only instantiate from a library header (rocprim) are counted per
file and get a row only if they differ.

usage: python tools/isa_compare.py [--parent REV | --parent-tree DIR] [--new-tree DIR]
                                   [--out FILE.json] [--jobs N] [FILE.hip ...]
The parent defaults to HEAD, extracted with `git archive` into a temporary directory;
the new tree defaults to the working tree this script lives in.
"""
import argparse
import collections
import concurrent.futures
import difflib
import hashlib
import json
import os
import re
import shutil
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join("aa-clip_amd", "csrc")
RESOURCES = ("VGPRs", "AGPRs", "TotalSGPRs", "ScratchSize [bytes/lane]", "LDS Size [bytes/block]",
             "Occupancy [waves/SIMD]", "VGPRs Spill", "SGPRs Spill")


def makefile_plan(tree):
    """SRCS, the compiler, the common flags and the per-file extra flags, read from the Makefile."""
    text = open(os.path.join(tree, CSRC, "Makefile")).read().replace("\\\n", " ")
    var = {m.group(1): m.group(2).strip() for m in re.finditer(r"^(\w+)\s*[:?]?=\s*(.*)$", text, re.M)}
    expand = lambda s: re.sub(r"\$\((\w+)\)", lambda m: var.get(m.group(1), ""), s)
    extra = collections.defaultdict(list)
    for m in re.finditer(r"^((?:build/\S+\.o\s*)+):\s*HIPFLAGS\s*\+=\s*(.*)$", text, re.M):
        for obj in m.group(1).split():
            extra[os.path.basename(obj)[:-2] + ".hip"] += m.group(2).split()
    flags = [f for f in expand(var["HIPFLAGS"]).split() if f != "-fPIC"]
    return var["SRCS"].split(), os.environ.get("HIPCC", expand(var["HIPCC"])), flags, extra


def compile_one(tree, hipcc, flags, src, out_dir):
    """Device-only assembly of one file; returns (assembly path, the compiler's remarks)."""
    asm = os.path.join(out_dir, src[:-4] + ".s")
    cmd = [hipcc, *flags, "--cuda-device-only", "-S", "-Rpass-analysis=kernel-resource-usage", src, "-o", asm]
    r = subprocess.run(cmd, cwd=os.path.join(tree, CSRC), capture_output=True, text=True)
    if r.returncode:
        raise RuntimeError("%s failed in %s:\n%s" % (" ".join(cmd), tree, r.stderr[-4000:]))
    return asm, r.stderr


def resources(remarks):
    """{function: {resource: value, "source": file of its definition}} from the kernel-resource-usage remarks."""
    out, cur = {}, None
    for line in remarks.splitlines():
        m = re.search(r"^(.*?):\d+:\d+: remark: +(.*?) \[-Rpass-analysis", line)
        if not m:
            continue
        key, _, val = m.group(2).partition(": ")
        if key == "Function Name":
            cur = out.setdefault(val.strip(), {"source": m.group(1)})
        elif cur is not None and key.strip() in RESOURCES:
            cur[key.strip()] = int(val)
    return out


def kernel_streams(asm):
    """{kernel: [instruction, ...]} -- comments, directives and label lines dropped."""
    lines = open(asm).read().splitlines()
    kernels = set(re.findall(r"^\s*\.amdhsa_kernel\s+(\S+)", "\n".join(lines), re.M))
    out, cur = {}, None
    for line in lines:
        m = re.match(r"^([\w.$]+):", line)
        if m and m.group(1) in kernels:
            cur = out.setdefault(m.group(1), [])
            continue
        if cur is None:
            continue
        if re.match(r"^\.Lfunc_end\d+:", line):
            cur = None
            continue
        t = line.split(";")[0].strip()
        if t and not t.startswith(".") and not t.endswith(":"):
            cur.append(re.sub(r"\s+", " ", t))
    return out


def normalise(stream, registers):
    """Labels always lose their numbers; registers lose theirs (a range keeps its width) if asked."""
    def width(m):
        return "%s[%d]" % (m.group(1), int(m.group(3)) - int(m.group(2)) + 1)
    out = []
    for t in stream:
        t = re.sub(r"\.L\w+", ".L", t)
        if registers:
            t = re.sub(r"\b([vsa])\[(\d+):(\d+)\]", width, t)
            t = re.sub(r"\b(ttmp|[vsa])\d+\b", r"\1", t)
        out.append(t)
    return out


def compare_streams(a, b):
    ra, rb = normalise(a, False), normalise(b, False)
    if ra == rb:
        return {"stream": "identical"}
    na, nb = normalise(a, True), normalise(b, True)
    if na == nb:
        return {"stream": "identical after normalising registers"}
    ops = [o for o in difflib.SequenceMatcher(None, na, nb, autojunk=False).get_opcodes() if o[0] != "equal"]
    return {"stream": "differs", "same_instruction_count": len(a) == len(b),
            "same_instructions_reordered": collections.Counter(na) == collections.Counter(nb),
            "differing_regions": len(ops), "parent_instructions_in_them": sum(o[2] - o[1] for o in ops),
            "new_instructions_in_them": sum(o[4] - o[3] for o in ops), "first_at": ops[0][1]}


def short_name(mangled, pretty, limit=160):
    """Library kernels (rocprim) demangle to kilobytes: cut them, keep them unique by a hash."""
    pretty = pretty.replace("(anonymous namespace)::", "")
    if len(pretty) <= limit:
        return pretty
    return "%s... #%s" % (pretty[:limit], hashlib.sha1(mangled.encode()).hexdigest()[:10])


def demangle(names):
    filt = shutil.which("llvm-cxxfilt") or shutil.which("c++filt")
    try:
        r = subprocess.run([filt], input="\n".join(names), capture_output=True, text=True, check=True)
        return {n: short_name(n, s) for n, s in zip(names, r.stdout.splitlines())}
    except (TypeError, OSError, subprocess.CalledProcessError):  # no demangler: mangled names
        return {n: n for n in names}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--parent", default="HEAD", help="revision of the parent tree (git archive)")
    ap.add_argument("--parent-tree", help="an extracted parent tree instead of --parent")
    ap.add_argument("--new-tree", default=ROOT)
    ap.add_argument("--out", help="write the JSON report here (default: stdout)")
    ap.add_argument("--jobs", type=int, default=min(8, os.cpu_count() or 1))
    ap.add_argument("files", nargs="*", help="a subset of SRCS (default: all of it)")
    args = ap.parse_args()

    with tempfile.TemporaryDirectory(prefix="isa_compare_") as tmp:
        parent = args.parent_tree
        rev = None
        if not parent:
            parent = os.path.join(tmp, "parent")
            os.mkdir(parent)
            rev = subprocess.run(["git", "rev-parse", args.parent], cwd=ROOT, capture_output=True, text=True,
                                 check=True).stdout.strip()
            tar = subprocess.run(["git", "archive", rev, CSRC, "include"], cwd=ROOT, capture_output=True, check=True)
            subprocess.run(["tar", "-x", "-C", parent], input=tar.stdout, check=True)
        trees = {"parent": parent, "new": args.new_tree}
        srcs, hipcc, flags, extra = makefile_plan(args.new_tree)
        srcs = [s for s in srcs if not args.files or s in args.files]
        jobs = {}
        with concurrent.futures.ThreadPoolExecutor(args.jobs) as pool:
            for side, tree in trees.items():
                os.mkdir(os.path.join(tmp, side + "_s"))
                _, side_hipcc, side_flags, side_extra = makefile_plan(tree)
                for s in srcs:
                    jobs[side, s] = pool.submit(compile_one, tree, side_hipcc, side_flags + side_extra[s], s,
                                                os.path.join(tmp, side + "_s"))
            built = {k: f.result() for k, f in jobs.items()}

        report = {"how": "%s %s --cuda-device-only -S -Rpass-analysis=kernel-resource-usage per file of SRCS "
                         "(+ %s), parent against new; instruction streams compared as text (labels renumbered) "
                         "and after register names are replaced by their class and width"
                         % (os.path.basename(hipcc), " ".join(flags),
                            "; ".join("%s: %s" % (s, " ".join(f)) for s, f in sorted(extra.items()))),
                  "parent": rev or os.path.abspath(parent), "resource_columns": RESOURCES, "files": {}}
        total = collections.Counter()
        for s in srcs:
            side = {}
            for name in trees:
                asm, remarks = built[name, s]
                side[name] = (kernel_streams(asm), resources(remarks))
            names = sorted(set(side["parent"][0]) | set(side["new"][0]))
            pretty = demangle(names)
            rows, library = [], collections.Counter()
            for k in names:
                if k not in side["parent"][0] or k not in side["new"][0]:
                    rows.append({"kernel": pretty[k], "only_in": "parent" if k in side["parent"][0] else "new"})
                    total["unmatched"] += 1
                    continue
                pa, nw = side["parent"][0][k], side["new"][0][k]
                rp, rn = side["parent"][1].get(k, {}), side["new"][1].get(k, {})
                src = rn.pop("source", "")
                rp.pop("source", None)
                cols = lambda r: [r.get(c) for c in RESOURCES]  # "resource_columns" names them
                row = {"kernel": pretty[k], "resources_equal": rp == rn,
                       **({"resources": cols(rn)} if rp == rn else {"parent": cols(rp), "new": cols(rn)}),
                       "instructions": len(nw) if len(pa) == len(nw) else [len(pa), len(nw)],
                       **compare_streams(pa, nw)}
                kind = {"identical": "stream_identical", "differs": "stream_differs"}.get(row["stream"],
                                                                                        "stream_register_only")
                total["kernels"] += 1
                total["resources_equal"] += row["resources_equal"]
                total[kind] += 1
                if os.path.isabs(src):  # defined in a library header, not in csrc
                    library["kernels"] += 1
                    library["unchanged"] += kind == "stream_identical" and row["resources_equal"]
                    if kind == "stream_identical" and row["resources_equal"]:
                        continue
                rows.append(row)
            report["files"][s] = {"kernels": len(names), "library_kernels": dict(library),
                                  "all_resources_equal": all(r.get("resources_equal") for r in rows),
                                  "all_streams_identical": all(r.get("stream") == "identical" for r in rows),
                                  "rows": rows}
        report["summary"] = dict(total)
        listed = lambda pred: [{"file": s, "kernel": r["kernel"]} for s, f in report["files"].items()
                               for r in f["rows"] if pred(r)]
        report["resources_differ"] = listed(lambda r: "stream" in r and not r["resources_equal"])
        report["register_only"] = listed(lambda r: r.get("stream") == "identical after normalising registers")
        report["differing"] = listed(lambda r: r.get("stream", "differs") == "differs")

    # one kernel per line: the report of ~1000 kernels stays readable and small
    files = report.pop("files")
    text = json.dumps(report, indent=1)[:-2] + ',\n "files": {\n' + ",\n".join(
        '  %s: {%s,\n   "rows": [\n%s\n   ]}' % (
            json.dumps(s), json.dumps({k: v for k, v in f.items() if k != "rows"})[1:-1],
            ",\n".join("    " + json.dumps(r) for r in f["rows"])) for s, f in files.items()) + "\n }\n}\n"
    json.loads(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)
        print(json.dumps({k: report[k] for k in ("summary", "resources_differ", "register_only", "differing")}, indent=1))
    else:
        sys.stdout.write(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
