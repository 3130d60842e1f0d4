"""Compare two `make asm` outputs of one source kernel by kernel, whatever their order.
usage: cmp_asm.py parent.s result.s
Checks (1) the sorted kernel names, (2) each kernel's .amdhsa_* descriptor and its entry of
the amdhsa.kernels metadata, (3) each kernel's instruction text with the function number of
local labels (.LBB<n>_<m>, .Lfunc_begin<n> / .Lfunc_end<n>) normalised and the assembler
comments dropped (the loop comments repeat the block labels as BB<n>_<m>)."""
import re
import sys


def kernels(path):
    lines = open(path).read().split("\n")
    desc, text, meta = {}, {}, {}
    i = 0
    while i < len(lines):
        m = re.match(r"\s*\.amdhsa_kernel (\S+)", lines[i])
        if m:
            j = i
            while ".end_amdhsa_kernel" not in lines[j]:
                j += 1
            desc[m.group(1)] = lines[i:j]
            i = j
        i += 1
    label = {n + ":": n for n in desc}
    i = 0
    while i < len(lines):
        n = label.get(lines[i].split(" ")[0].split("\t")[0])
        if n and n not in text:
            j = i
            while not re.match(r"\.Lfunc_end\d+:", lines[j]):
                j += 1
            body = "\n".join(re.sub(r"\s*;.*", "", l) for l in lines[i:j])  # (comments name BB<n>_<m>)
            text[n] = re.sub(r"\.L(BB|func_begin|func_end|tmp)\d+", r".L\1#", body)
            i = j
        i += 1
    a = lines.index("amdhsa.kernels:")
    entry = []
    for l in lines[a + 1:]:
        if l.startswith("  - ") or not l.startswith("  "):
            if entry:
                name = next(x.split()[-1] for x in entry if x.strip().startswith(".name:"))
                meta[name] = entry
            entry = []
            if not l.startswith("  "):
                break
        entry.append(l)
    return desc, text, meta


p, r = kernels(sys.argv[1]), kernels(sys.argv[2])
names = sorted(p[0])
print("kernels: parent %d, result %d, names %s" % (len(p[0]), len(r[0]),
                                                  "identical" if names == sorted(r[0]) else "DIFFER"))
assert len(p[1]) == len(names) and len(p[2]) == len(names), "parse: a kernel without text or metadata"
bad = 0
for what, k in (("descriptor", 0), ("instruction text", 1), ("metadata entry", 2)):
    diff = [n for n in names if p[k][n] != r[k].get(n)]
    bad += len(diff)
    print("%s: %d of %d kernels differ %s" % (what, len(diff), len(names), " ".join(diff[:5])))
order = [n for n in p[0]] == [n for n in r[0]]
print("order of the kernels: %s" % ("the same" if order else "permuted"))
sys.exit(1 if bad or names != sorted(r[0]) else 0)
