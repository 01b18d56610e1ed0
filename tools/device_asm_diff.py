#!/usr/bin/env python3
"""Did a host-only change leave the device code alone?

    hipcc <build.py FLAGS> -S --cuda-device-only csrc/X.hip -o a/X.s      (once per tree)
    python tools/device_asm_diff.py [--map REGEX=REPLACEMENT ...] a/X.s b/X.s

 Same kernel symbols, and per kernel the same instruction stream and kernel descriptor, whatever the order
in which the instantiations were emitted (function-numbered local labels and the per-file __hip_cuid hash are normalised).
--map rewrites the first file's text before the comparison, for a kernel whose template parameter list (and so its mangled
name) changed:  --map '(linear_sk_kernelI\w+?)Lb0E(EEv)=\1\2'  drops a trailing `false` argument."""
import re, sys
args, maps = sys.argv[1:], []
while "--map" in args:
    i = args.index("--map"); old, new = args[i + 1].split("=", 1); maps.append((re.compile(old), new)); del args[i:i + 2]
def load(path, maps=()):
    fn, desc, cur, kind = {}, {}, None, None
    for line in open(path):
        for rx, new in maps: line = rx.sub(new, line)
        line = re.sub(r"\.L(BB|func_end|func_begin|tmp|JTI)(\d+)", r".L\1#", line.rstrip("\n"))
        if "__hip_cuid_" in line:
            continue
        full = line
        line = re.sub(r"\s*;.*$", "", line)          # comments carry function-numbered block names and column padding
        if not line.strip() and not re.match(r"^\w+:\s+; @", full):
            continue
        m = re.match(r"^(\w+):\s+; @(\w+)$", full)
        if m and m.group(1) == m.group(2):
            cur, kind = m.group(1), "fn"; fn[cur] = []; continue
        m = re.match(r"^\s+\.amdhsa_kernel (\w+)$", line)
        if m:
            cur, kind = m.group(1), "desc"; desc[cur] = []; continue
        if kind == "fn" and line.startswith(".Lfunc_end#"):
            kind = None; continue
        if kind == "desc" and ".end_amdhsa_kernel" in line:
            kind = None; continue
        if kind == "fn": fn[cur].append(line)
        elif kind == "desc": desc[cur].append(line)
    return fn, desc
fa, da = load(args[0], maps); fb, db = load(args[1])
ok = set(fa) == set(fb) and set(da) == set(db)
bad = [k for k in fa if k in fb and fa[k] != fb[k]] + [k for k in da if k in db and da[k] != db[k]]
print(f"{args[1].split('/')[-1]}: {len(da)} kernels, {len(fa)} functions, {sum(len(v) for v in fa.values())} lines; symbols {'identical' if ok else 'DIFFER'}; "
      f"bodies / descriptors {'identical' if not bad else 'DIFFER: ' + ' '.join(bad[:5])}")
sys.exit(0 if ok and not bad else 1)
