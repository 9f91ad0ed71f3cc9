"""Where a kernel's spill code sits, basic block by basic block, from a hipcc -save-temps .s: every block that holds a
scratch access, and every block that is a keystream (>= 100 ds_read_b32), a GHASH product (>= 16 ds_read_b128) or
memory I/O (>= 2 global loads or stores), with the loop depth the compiler prints for it (quad.hip: 1 = key segments,
2 = packets, 3 = a packet's groups; a packet's first and last group sit at depth 2).  A kernel whose groups are free of
spill code shows scratch 0 on every keystream and product line and none at depth 3.
usage: python3 tools/isa_blocks.py FILE.s SYMBOL_SUBSTR [...]"""
import re
import sys
from collections import Counter

txt = open(sys.argv[1]).read()
for name in [m.group(1) for m in re.finditer(r"^(_Z\S+):", txt, re.M) if any(p in m.group(1) for p in sys.argv[2:])]:
    i = txt.index(name + ":")
    end = txt.index(".Lfunc_end", i)
    meta = txt[end:end + 4000]
    print(name[:100])
    print("  " + "  ".join(k + "=" + re.search("; " + k + ": ([0-9]+)", meta).group(1)
                           for k in ("NumVgprs", "ScratchSize", "Occupancy")))
    parts = re.split(r"^(\.LBB\d+_\d+):", txt[i:end], flags=re.M)
    blocks = [("entry", parts[0])] + [(parts[j], parts[j + 1]) for j in range(1, len(parts) - 1, 2)]
    tot = hot_scratch = deep_scratch = 0
    for lab, body in blocks:
        lines = [x.strip() for x in body.split("\n")]
        c = Counter(x.split()[0] for x in lines if x and not x.startswith((".", ";")) and not x.endswith(":"))
        depth = re.search(r"Depth=(\d+)", "\n".join(lines[:3]))
        scr = sum(v for k, v in c.items() if k.startswith("scratch_"))
        gl = sum(v for k, v in c.items() if k.startswith("global_load"))
        gs = sum(v for k, v in c.items() if k.startswith("global_store"))
        kind = "keystream" if c["ds_read_b32"] >= 100 else "product" if c["ds_read_b128"] >= 16 else "io" if gl >= 2 or gs >= 2 else ""
        d = int(depth.group(1)) if depth else 0
        tot += scr
        hot_scratch += scr if kind in ("keystream", "product") else 0
        deep_scratch += scr if d >= 3 else 0
        if scr or kind:
            print(f"  {lab:11s} depth {d}  insts {sum(c.values()):5d}  ds_read_b32 {c['ds_read_b32']:4d}  "
                  f"ds_read_b128 {c['ds_read_b128']:3d}  global ld/st {gl:2d}/{gs:2d}  scratch {scr}  {kind}")
    print(f"  scratch accesses: {tot} in all, {hot_scratch} in keystream and product blocks, {deep_scratch} at depth >= 3")
