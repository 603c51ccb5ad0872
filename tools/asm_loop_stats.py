#!/usr/bin/env python
"""Instruction mix of a kernel's hottest loop, from hipcc's device assembly.

    hipcc -O3 -std=c++17 -ffp-contract=off --offload-arch=gfx950 -Iinclude -Icontextgs_amd/csrc \
          -S --offload-device-only contextgs_amd/csrc/mlp3.hip -o mlp3.s
    python tools/asm_loop_stats.py mlp3.s mlp3_bwd_wg_kernelILb1ELb1E

The loop is the one (by LLVM's "Loop: Header=" block comments) that holds the most MFMAs; for the one-wave MLP kernels that
is the tile loop.  Counts are per trip through every block of the loop (both sides of a branch count), so they bound a
trip from above.  `waits before an MFMA` = s_waitcnt whose next non-scalar instruction is an MFMA: the matrix pipe stops
there until the counter drains.
"""
import collections
import re
import sys


def main():
    path, key = sys.argv[1], sys.argv[2]
    lines = open(path).read().split("\n")
    start = next(i for i, l in enumerate(lines) if re.match(r"^_Z\w*:", l) and key in l)
    end = next(i for i in range(start, len(lines)) if lines[i].startswith(".Lfunc_end"))
    name = lines[start].split(":")[0]
    blocks, cur = collections.OrderedDict(), ("entry", None)
    blocks[cur] = []
    for l in lines[start + 1:end]:
        m = re.match(r"^(\.LBB\d+_\d+):\s*(;.*)?$", l)
        if m:
            c = m.group(2) or ""
            h = re.search(r"Header=(BB\d+_\d+)", c)
            hdr = h.group(1) if h else (m.group(1)[2:] if "Loop Header" in c else None)
            cur = (m.group(1), hdr)
            blocks[cur] = []
            continue
        s = l.split(";")[0].strip()
        if s and not s.startswith(".") and not s.endswith(":"):
            blocks[cur].append(s)
    per = collections.defaultdict(list)
    for (lab, hdr), ins in blocks.items():
        if hdr:
            per[hdr] += ins
    hdr = max(per, key=lambda h: sum(i.startswith("v_mfma") for i in per[h]))
    ins = per[hdr]
    cnt = collections.Counter()
    for k, i in enumerate(ins):
        op = i.split()[0]
        if op.startswith("v_mfma"):
            cnt["mfma"] += 1
        elif op.startswith("v_accvgpr"):
            cnt["agpr moves"] += 1
        elif op.startswith("v_"):
            cnt["valu"] += 1
        elif op.startswith("ds_"):
            cnt["lds ops"] += 1
            cnt["lds reads" if "read" in op or "load" in op else "lds writes"] += 1
        elif op.startswith(("buffer_", "global_", "flat_")):
            cnt["vmem"] += 1
        elif op.startswith("scratch_"):
            cnt["scratch ops"] += 1
        elif op == "s_waitcnt":
            cnt["s_waitcnt"] += 1
            if "lgkmcnt" in i:
                cnt["s_waitcnt lgkmcnt"] += 1
            if "vmcnt" in i:
                cnt["s_waitcnt vmcnt"] += 1
            if "lgkmcnt(0)" in i:
                cnt["s_waitcnt lgkmcnt(0)"] += 1
            for j in ins[k + 1:]:
                if j.startswith("s_"):
                    continue
                if j.startswith("v_mfma"):
                    cnt["waits before an MFMA"] += 1
                break
        elif op == "s_nop":
            cnt["s_nop"] += 1
    meta = {}
    for l in lines[end:]:
        if ".name:" in l and meta.get("hit") is None and l.split()[-1] == name:
            meta["hit"] = True
    # the metadata block of the kernel: the fields precede and follow .name inside one YAML item
    txt = "\n".join(lines[end:])
    item = next(b for b in txt.split("\n  - .agpr_count:") if re.search(r"\.name:\s+" + re.escape(name) + r"\s", b))
    for f in ("vgpr_count", "sgpr_count", "private_segment_fixed_size", "vgpr_spill_count", "sgpr_spill_count"):
        m = re.search(r"\." + f + r":\s+(\d+)", item)
        meta[f] = int(m.group(1)) if m else None
    meta["agpr_count"] = int(item.split("\n")[0])
    print(f"{name}\n  loop header {hdr}, {len(ins)} instructions")
    for k in ("mfma", "valu", "agpr moves", "lds ops", "lds reads", "lds writes", "vmem", "scratch ops", "s_waitcnt",
              "s_waitcnt lgkmcnt", "s_waitcnt lgkmcnt(0)", "s_waitcnt vmcnt", "waits before an MFMA", "s_nop"):
        print(f"  {k:24s} {cnt[k]}")
    print(f"  registers: {meta['vgpr_count']} unified ({meta['agpr_count']} AGPRs), {meta['sgpr_count']} SGPRs; "
          f"scratch {meta['private_segment_fixed_size']} B, VGPR spills {meta['vgpr_spill_count']}, SGPR spills {meta['sgpr_spill_count']}")


if __name__ == "__main__":
    main()
