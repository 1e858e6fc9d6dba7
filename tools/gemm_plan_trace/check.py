#!/usr/bin/env python3
"""Dispatch-trace parity of the GEMM planner (recipe and results: profiles/gemm_plan_parity.txt).
  check.py corpus OUT.txt [product.json]   write the descriptor corpus (tests/gemm_plan_corpus.py sweep, then the product's rows) as text
  check.py plans TRACE.log CUS [product.json]   translate a trace of main.cpp over that corpus into plan fields and compare every
                                                descriptor with insv2v_gemm_plan; print the SHA-256 of the plans' canonical text"""
import hashlib, json, os, re, sys
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [os.path.join(ROOT, "instruct-video-to-video_amd"), os.path.join(ROOT, "tests")]
import gemm_plan_corpus as G

SHAPES = {(2, 2, 2, 2, 1): 1, (2, 2, 1, 2, 1): 2, (2, 2, 2, 1, 1): 3, (2, 2, 1, 1, 1): 4, (4, 2, 1, 2, 1): 5, (4, 2, 2, 2, 1): 6, (4, 2, 1, 1, 1): 7,
          (2, 2, 2, 2, 2): 8, (2, 2, 2, 1, 2): 9}
HALO = {(4, 2, 1, 2, 1, 2): 0, (2, 2, 2, 2, 2, 2): 1, (2, 2, 2, 2, 1, 2): 2, (8, 2, 1, 2, 1, 3): 3}
Q8 = {(0, 1): 0, (0, 0): 1, (2, 1): 2, (3, 1): 3, (4, 1): 4, (4, 0): 5}
W4 = {(1, 4, 4): 0, (2, 2, 4): 1, (2, 4, 2): 2, (4, 2, 2): 3}


def corpus(product=None):
    rows = [d for _, d in G.sweep()]
    if product:
        rows += [dict(zip(G.FIELDS, r["d"])) for r in json.load(open(product))["rows"]]
    return rows


def translate(block, d):
    """Plan fields that the launches of one descriptor show: {field: value}."""
    rc, parts, fuses = map(int, re.match(r"rc (-?\d+) parts (\d+) fuses (\d+)", block[-1]).groups())
    want = dict(rc=rc, gn_fuse=fuses)
    main = [l for l in block[:-1] if "launch_" in l]
    if rc or not main:
        return want, parts
    t = {k: {"true": 1, "false": 0}.get(v, v) for k, v in re.findall(r"(\w+) = (\w+)", main[0].split("[")[1].split("]")[0])}
    t = {k: int(v) for k, v in t.items()}
    M = int(re.search(r"desc\[M=(\d+)", main[0]).group(1))
    if len(main) > 1 or M != d["M"]:
        return dict(want, parts=len(main), units_per_part=M // (d["OH"] * d["OW"]) if d["mode"] else M, ln_finalize=int("ln_finalize" in block[0])), parts
    fin = int(any("ln_finalize" in l for l in block) and " sp=0 " in main[0] and "rs=%x " % G.ADDR["stats_scratch"] in main[0])
    want.update(parts=1, splitk_reduce=int("splitk_reduce" in block[-2]), split_k=int(re.search(r"grid \d+ \d+ (\d+)", main[0]).group(1)), ln_finalize=fin)
    if "launch_cfg" in main[0]:
        want.update(family=1, variant=SHAPES[t["WM"], t["WN"], t["MI"], t["NI"], t["KG"]], ring=t["STAGES"])
    elif "launch_halo" in main[0]:
        want.update(family=2, variant=HALO[t["WM"], t["WN"], t["MI"], t["NI"], t["KG"], t["WS"]], tw_shift=int(main[0].rsplit(" ", 1)[1]))
    elif "launch_q8" in main[0]:
        want.update(family=3, variant=Q8[t["DBG"], t["VAR"]])
    elif "launch_r8" in main[0]:
        want.update(family=4, variant=t["DBG"], cim=t["CIM"])
    else:
        want.update(family=5, variant=W4[t["WM"], t["WN"], t["TM"]] + (10 if t["DBG"] == 2 else 0))
    return want, parts


if __name__ == "__main__":
    if sys.argv[1] == "corpus":
        open(sys.argv[2], "w").write("".join(G.text_line(d) + "\n" for d in corpus(*sys.argv[3:4])))
        sys.exit(0)
    from insv2v import _lib
    lib, rows, cus = _lib.load(), corpus(*sys.argv[4:5]), int(sys.argv[3])
    lib.insv2v_set_operand_window(int(os.environ.get("HARNESS_WINDOW", 0)))   # (the conditions of the trace: this and the INSV2V_* switches)
    blocks = [b.strip().split("\n")[1:] for b in open(sys.argv[2]).read().split("#")[1:]]
    assert len(blocks) == len(rows), (len(blocks), len(rows))
    sha, bad = hashlib.sha256(), 0
    for i, (d, b) in enumerate(zip(rows, blocks)):
        p = G.plan_of(lib, d, cus)
        want, parts = translate(b, d)
        ok = all(p[k] == v for k, v in want.items()) and (-(-d["N"] // p["stats_width"]) if p["stats_width"] else 0) == parts
        if not ok and (bad := bad + 1) <= 10:
            print("MISMATCH row", i, {k: (p[k], v) for k, v in want.items() if p[k] != v}, "parts", parts, b[-1])
        sha.update((G.plan_text(p) + "\n").encode())
    print(f"{len(rows)} descriptors, {bad} plans differ from the trace; sha256 of the plans' text {sha.hexdigest()}")
    sys.exit(1 if bad else 0)
