#!/usr/bin/env python
"""Resource table of every kernel of one translation unit, at two commits, from hipcc's device assembly.

    hipcc -O3 -std=c++17 -ffp-contract=off --offload-arch=gfx950 -Iinclude -Icontextgs_amd/csrc \
          -S --offload-device-only contextgs_amd/csrc/loss.hip -o new.s          (and the parent's file -> old.s)
    python tools/asm_kernel_table.py old.s new.s | c++filt

Per kernel: VGPRs, AGPRs, SGPRs, spilled VGPRs, scratch bytes, LDS bytes (the `amdhsa.kernels` metadata), the number of
instructions, and `identical` when the kernel's instructions in the two files are the same text (labels renumbered), `CHANGED`
(with the old figures) when not, `new` / `gone` when only one file has it.  Needs no GPU.
"""
import hashlib
import re
import sys


def kernels(path):
    txt = open(path).read()
    out = {}
    for m in re.finditer(r"- \.agpr_count:.*?(?=\n  - \.agpr_count:|\namdhsa\.target|\Z)", txt, flags=re.S):
        blk = m.group(0)
        name = re.search(r"\.name:\s+(\S+)", blk).group(1)
        field = lambda k: int(re.search(r"\.%s:\s+(\d+)" % k, blk).group(1))        # noqa: E731
        out[name] = dict(v=field("vgpr_count"), a=field("agpr_count"), s=field("sgpr_count"), spill=field("vgpr_spill_count"),
                         scr=field("private_segment_fixed_size"), lds=field("group_segment_fixed_size"))
    lines = txt.split("\n")
    for name, k in out.items():
        start = next(i for i, l in enumerate(lines) if l.startswith(name + ":"))
        end = next(i for i in range(start, len(lines)) if lines[i].startswith(".Lfunc_end"))
        body = [l.split(";")[0].strip() for l in lines[start + 1:end]]
        body = [re.sub(r"\.LBB\d+_", ".LBB_", l) for l in body if l and not l.startswith(".")]
        k["n"] = sum(1 for l in body if not l.endswith(":"))
        k["h"] = hashlib.sha256("\n".join(body).encode()).hexdigest()[:12]
    return out


def main():
    old, new = kernels(sys.argv[1]), kernels(sys.argv[2])
    for name in sorted(set(old) | set(new)):
        ka, kb = old.get(name), new.get(name)
        k = kb or ka
        tag = "new      " if ka is None else ("gone     " if kb is None else ("identical" if ka == kb else "CHANGED  "))
        print(f"  {tag}  v{k['v']} a{k['a']} s{k['s']} spill{k['spill']} scr{k['scr']} lds{k['lds']:<6} {k['n']:5d} instr  {name}")
        if tag.startswith("CHANGED"):
            print(f"             was v{ka['v']} a{ka['a']} s{ka['s']} spill{ka['spill']} scr{ka['scr']} lds{ka['lds']} {ka['n']} instr")


if __name__ == "__main__":
    main()
