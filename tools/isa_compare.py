"""Device code of two trees, function by function (the method of profiles/kernel_helpers_isa.txt, profiles/device_prep_isa.txt).

    python tools/isa_compare.py PARENT_TREE TREE [REPORT]

Every .hip of build.SOURCES is compiled in both trees with build.FLAGS + --cuda-device-only -S.  Directive lines, comment lines
and the __hip_cuid_* label are dropped and local labels renumbered; what is left of each function is compared.  A kernel's
register, scratch and LDS figures (its .amdhsa_kernel block) are compared beside its instructions.  A function that exists on
one side only is matched by body against the other side's unmatched functions of the same file (a rename).  No GPU needed.
"""
import os
import re
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from score_amd import build          # noqa: E402

FIGURES = ("next_free_vgpr", "next_free_sgpr", "accum_offset", "group_segment_fixed_size", "private_segment_fixed_size")


def assembly(tree, src, out):
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    if not os.path.exists(os.path.join(tree, "score_amd", "csrc", src)):
        return ""                        # (a file one tree does not have: all of its functions count as added / removed)
    subprocess.check_call([hipcc] + build.FLAGS + ["--cuda-device-only", "-S", os.path.join(tree, "score_amd", "csrc", src), "-o", out])
    return open(out).read()


def functions(text):
    """{name: (normalised body, figures or None)} of one assembly file"""
    names = re.findall(r"^\s*\.type\s+(\S+),@function", text, re.M)
    figs = {}
    for m in re.finditer(r"^\s*\.amdhsa_kernel\s+(\S+)\n(.*?)^\s*\.end_amdhsa_kernel", text, re.M | re.S):
        vals = dict(re.findall(r"\.amdhsa_(\w+)\s+(\S+)", m.group(2)))
        figs[m.group(1)] = tuple((k, vals.get(k)) for k in FIGURES)
    out = {}
    for name in names:
        m = re.search(r"^%s:[^\n]*\n(.*?)^\.Lfunc_end\d+:" % re.escape(name), text, re.M | re.S)
        if not m:
            continue
        labels, lines = {}, []
        for line in m.group(1).split("\n"):
            line = line.split(";")[0].strip()
            if not line or (line.startswith(".") and not line.endswith(":")) or line.startswith("__hip_cuid_"):
                continue
            lines.append(line)
        body = "\n".join(lines)
        for lab in re.findall(r"\.L\w+", body):
            labels.setdefault(lab, ".L%d" % len(labels))
        body = re.sub(r"\.L\w+", lambda x: labels[x.group(0)], body)
        out[name] = (body, figs.get(name))
    return out


def main():
    parent, tree = sys.argv[1], sys.argv[2]
    report = open(sys.argv[3], "w") if len(sys.argv) > 3 else sys.stdout
    same, differ, removed, added, renamed = [], [], [], [], []
    with tempfile.TemporaryDirectory() as tmp, ThreadPoolExecutor(max_workers=8) as pool:
        jobs = [(src, pool.submit(assembly, parent, src, os.path.join(tmp, "a_" + src)),
                 pool.submit(assembly, tree, src, os.path.join(tmp, "b_" + src))) for src in build.SOURCES]
        for src, ja, jb in jobs:
            a, b = functions(ja.result()), functions(jb.result())
            gone, new = [n for n in a if n not in b], [n for n in b if n not in a]
            for n in a:
                if n in b:
                    (same if a[n] == b[n] else differ).append((src, n))
            for n in list(gone):
                twin = next((x for x in new if b[x] == a[n]), None)
                if twin is not None:              # (two parent kernels may become one: the twin stays available)
                    renamed.append((src, n, twin))
                    gone.remove(n)
            new = [x for x in new if x not in [r[2] for r in renamed if r[0] == src]]
            removed += [(src, n) for n in gone]
            added += [(src, n) for n in new]
    w = lambda s="": report.write(s + "\n")
    w("Device code comparison, parent vs tree: every .hip of build.SOURCES with build.FLAGS + --cuda-device-only -S,")
    w("directive lines, comment lines and the __hip_cuid_* label dropped, local labels renumbered, function by function;")
    w("per kernel also these figures of its .amdhsa_kernel block:")
    w("  " + ", ".join(FIGURES))
    w()
    w("identical: %d   differing: %d   same body under another name: %d   removed: %d   added: %d"
      % (len(same), len(differ), len(renamed), len(removed), len(added)))
    for title, rows in (("Differing", differ), ("Removed (in the parent only, no body like it in the tree)", removed),
                        ("Added (in the tree only, no body like it in the parent)", added)):
        w()
        w(title + ":")
        for r in rows or [("none",)]:
            w("  " + "  ".join(r))
    w()
    w("Same body (and figures) under another name, parent -> tree:")
    for src, n, twin in renamed or [("none", "", "")]:
        w("  %s  %s -> %s" % (src, n, twin))
    w()
    w("Identical functions:")
    for r in same:
        w("  " + "  ".join(r))
    return 1 if differ else 0


if __name__ == "__main__":
    sys.exit(main())
