#!/usr/bin/env python3
"""Print the generator refill loop of one demand_v3_kernel instantiation from an assembly listing
(hipcc -S --offload-device-only of csrc/demand_v3.hip) with its instruction counts per draw, and the
register and scratch figures of every instantiation in the file.

  python tools/gen_loop_listing.py demand_v3.s [Li5ELi3ELb0E]

The loop is the second innermost loop of the kernel that writes the ring twice (ds_write_b64): the
first is the initial fill, the second the per-chunk refill."""
import re
import sys


def main() -> int:
    path = sys.argv[1]
    inst = sys.argv[2] if len(sys.argv) > 2 else "Li5ELi3ELb0E"
    lines = open(path).read().splitlines()
    start = next(i for i, l in enumerate(lines) if l.startswith("_ZN3msc16demand_v3_kernelI" + inst) and l.rstrip().endswith("E"))
    end = next(i for i in range(start, len(lines)) if lines[i].strip().startswith("s_endpgm"))
    loops, cur = [], None
    for i in range(start, end):
        l = lines[i]
        if re.match(r"^\.LBB\d+_\d+:", l):
            cur = i
        m = re.match(r"\s+s_cbranch_\w+ (\.LBB\d+_\d+)", l)
        if m and cur is not None and lines[cur].startswith(m.group(1) + ":"):
            body = lines[cur:i + 1]
            if sum("ds_write_b64" in b for b in body) == 2:
                loops.append(body)
    body = loops[1]
    ops = [b.split()[0] for b in body if b.startswith("\t") and not b.strip().startswith(";")]
    valu = [o for o in ops if o.startswith("v_")]
    print(f"; {inst}: refill loop, per draw: {len(valu)} VALU, {sum(o.startswith('ds_') for o in ops)} LDS, "
          f"{sum(o.startswith('s_') for o in ops)} scalar (of them {sum(o == 's_nop' for o in ops)} s_nop)")
    kinds = {}
    for o in valu:
        kinds[o] = kinds.get(o, 0) + 1
    print(";   " + ", ".join(f"{n} {o}" for o, n in sorted(kinds.items(), key=lambda kv: (-kv[1], kv[0]))))
    print("\n".join(body))
    print("\n; every instantiation: vgpr_count, vgpr_spill_count, private_segment_fixed_size")
    name = None
    vals = {}
    for l in lines:
        m = re.match(r"\s+\.name:\s+(\S+)", l)
        if m:
            name, vals = m.group(1), {}
        for k in ("private_segment_fixed_size", "vgpr_count", "vgpr_spill_count"):
            m = re.match(r"\s+\." + k + r":\s+(\d+)", l)
            if m:
                vals[k] = int(m.group(1))
        if name and "demand_v3_kernel" in name and len(vals) == 3:
            print(f";   {name}: {vals['vgpr_count']} {vals['vgpr_spill_count']} {vals['private_segment_fixed_size']}")
            name = None
    return 0


if __name__ == "__main__":
    sys.exit(main())
