#!/usr/bin/env python3
"""Per-kernel comparison of the gfx950 code of two versions of the library: the check that a refactor left every kernel's instruction
stream and resources alone.  OLD and NEW are each a checkout of this repository (its --sources are compiled with that tree's own build.py
flags, device side only) or a directory of `hipcc -S --cuda-device-only` output (*.s).  Kernels are matched by demangled name after
--rename; per kernel the instruction lines (comments stripped, .LBB labels renumbered in order of appearance) and the resource block
(.amdhsa_* directives + the register / spill / scratch / LDS counts of the metadata) are compared.  One line per kernel; exit status 1
on any difference, removal or addition that --differs / --removed / --added does not allow.

usage: tools/kernel_isa_diff.py OLD NEW [--sources REGEX] [--rename 'REGEX=REPL']... [--removed REGEX] [--added REGEX] [--differs REGEX]
e.g.   tools/kernel_isa_diff.py ../parent . --rename 'ffn_fused_kernel<0, (\\w+)>=ffn_fused_kernel<\\1>' --removed 'ffn_fused_kernel<\\d+, false>'"""
import argparse
import glob
import importlib.util
import os
import re
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

META = ("agpr_count", "vgpr_count", "sgpr_count", "vgpr_spill_count", "sgpr_spill_count", "private_segment_fixed_size", "group_segment_fixed_size")


def assembly(path, sources, tmp):
    """the .s texts of a directory of them, or of a checkout's matching sources"""
    build_py = os.path.join(path, "instruct-video-to-video_amd", "build.py")
    if not os.path.exists(build_py):
        return [open(f).read() for f in sorted(glob.glob(os.path.join(path, "*.s")))]
    spec = importlib.util.spec_from_file_location("insv2v_build", build_py)   # (that tree's own SOURCES and flags)
    b = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(b)
    out = tempfile.mkdtemp(dir=tmp)
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    srcs = [s for s in b.SOURCES if re.search(sources, s)]
    def run(src):
        o = os.path.join(out, src + ".s")
        subprocess.check_call([hipcc, *b.FLAGS, *b.EXTRA_FLAGS.get(src, []), "-S", "--cuda-device-only", os.path.join(b.CSRC, src), "-o", o], stderr=subprocess.DEVNULL)
        return open(o).read()
    with ThreadPoolExecutor(max_workers=4) as ex:
        return list(ex.map(run, srcs))


def kernels(texts, renames):
    """{name: (instruction and label lines, resource lines)}"""
    res = {}
    for s in texts:
        meta = {}
        for blk in s.split("- .agpr_count:")[1:]:
            blk = ".agpr_count:" + blk
            get = lambda k: re.search(r"\.%s:\s+(\S+)" % k, blk).group(1)
            meta[get("name")] = ["%s %s" % (k, get(k)) for k in META]
        for m in re.finditer(r"^\t\.amdhsa_kernel (\S+)\n(.*?)^\t\.end_amdhsa_kernel", s, re.S | re.M):
            sym = m.group(1)
            body = s[s.index("\n%s:" % sym):m.start()]
            labels, lines = {}, []
            for ln in body.split("\n")[2:]:
                ln = ln.split(";")[0].strip().replace(sym, "SELF")
                if not ln or ln.startswith(".section") or ln.startswith(".p2align"):
                    continue
                lines.append(re.sub(r"\.LBB\d+_\d+", lambda l: labels.setdefault(l.group(0), ".L%d" % len(labels)), ln))
            name = subprocess.run(["c++filt", sym], capture_output=True, text=True).stdout.strip()
            name = re.sub(r"\(.*\)$", "", re.sub(r"^void ", "", name.replace("(anonymous namespace)::", "")))
            for pat, repl in renames:
                name = re.sub(pat, repl, name)
            assert name not in res, name
            res[name] = (lines, [l.strip() for l in m.group(2).split("\n") if l.strip()] + meta[sym])
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("old")
    ap.add_argument("new")
    ap.add_argument("--sources", default=r"rows", help="checkouts: which of build.py's SOURCES to compile")
    ap.add_argument("--rename", action="append", default=[], help="REGEX=REPL applied to OLD's kernel names")
    ap.add_argument("--removed", default=r"$^", help="kernels of OLD that may be missing from NEW")
    ap.add_argument("--added", default=r"$^", help="kernels of NEW that OLD need not have")
    ap.add_argument("--differs", default=r"$^", help="kernels that may differ")
    a = ap.parse_args()
    with tempfile.TemporaryDirectory() as tmp:
        old = kernels(assembly(a.old, a.sources, tmp), [r.split("=", 1) for r in a.rename])
        new = kernels(assembly(a.new, a.sources, tmp), [])
    ninstr = lambda lines: sum(1 for l in lines if not l.endswith(":") and not l.startswith("."))
    bad = 0
    for name in sorted(set(old) | set(new)):
        if name not in new:
            verdict, ok = "removed", re.search(a.removed, name)
        elif name not in old:
            verdict, ok = "added", re.search(a.added, name)
        elif old[name] == new[name]:
            verdict, ok = "identical", True
        else:
            verdict = "differs (%d -> %d instructions%s)" % (ninstr(old[name][0]), ninstr(new[name][0]), "" if old[name][1] == new[name][1] else "; resources: " +
                      ", ".join("%s -> %s" % (o, n.split()[-1]) for o, n in zip(old[name][1], new[name][1]) if o != n))
            ok = re.search(a.differs, name)
        bad += not ok
        print("%-60s %s%s" % (name, verdict, "" if ok or verdict == "identical" else "   <-- NOT EXPECTED"))
    same = sum(1 for n in old if n in new and old[n] == new[n])
    print("%d kernels before, %d after: %d identical, %d differ, %d removed, %d added; %d not expected" % (
        len(old), len(new), same, sum(1 for n in old if n in new) - same, len(set(old) - set(new)), len(set(new) - set(old)), bad))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
