"""The chain of memory round trips of one kernel, read off the compiler's listing.

    python scripts/isa_load_chain.py LISTING.s [--kernel k_setupILb1ELb1E]

LISTING.s is the gfx950 assembly the Makefile's flags produce (hipcc ... -save-temps -c rasterize.hip leaves it beside the object as
rasterize-hip-amdgcn-amd-amdhsa-gfx950.s; -S --cuda-device-only gives the same text).  For the named kernel -- a substring of its mangled
name -- the script prints, in PROGRAM ORDER, every vector-memory load with its width, every atomic that returns a value, every
`s_waitcnt vmcnt(N)` and every barrier, each with its line in the listing, and every vector store with the hops in front of it.  A latency-bound kernel costs one
memory round trip per wait that some later load's ADDRESS depends on: loads between two waits are in flight together (one hop), a load
behind a wait is the next hop.  The summary counts the waits in front of the first store behind a wait that have at least one load issued since the
previous wait -- an upper bound of the dependent hops, exact where every group's addresses come from the group before, as in k_setup --
and prints the kernel's register, scratch and occupancy figures from the listing's own footer.

Program order is not execution order where the kernel branches: a loop body or a rarely taken branch appears once, in place.
"""
import argparse
import re
import sys

LOAD = re.compile(r"^(global|flat|buffer|scratch)_load_(\w+)")
ATOMIC = re.compile(r"^(global|flat|buffer)_atomic_(\w+)")
STORE = re.compile(r"^(global|flat|buffer|scratch)_store_(\w+)")
WIDTH = {"ubyte": 1, "sbyte": 1, "ushort": 2, "sshort": 2, "short": 2, "dword": 4, "dwordx2": 8, "dwordx3": 12, "dwordx4": 16,
         "ubyte_d16": 1, "ubyte_d16_hi": 1, "sbyte_d16": 1, "sbyte_d16_hi": 1, "short_d16": 2, "short_d16_hi": 2,
         "lds_dword": 4, "lds_dwordx3": 12, "lds_dwordx4": 16}


def kernel_span(lines, name):
    """(first, last) line indices of the kernel whose mangled label contains `name`; its footer comments follow `last`."""
    starts = [i for i, l in enumerate(lines) if re.match(r"^[A-Za-z_]\S*:", l) and name in l.split(":")[0] and not l.startswith(".L")]
    if not starts:
        sys.exit(f"no kernel matching {name!r} in the listing")
    if len(starts) > 1:
        sys.exit(f"{name!r} matches {len(starts)} kernels: " + ", ".join(lines[i].split(':')[0] for i in starts))
    start = starts[0]
    end = next(i for i in range(start, len(lines)) if lines[i].startswith(".Lfunc_end"))
    return start, end


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("listing")
    ap.add_argument("--kernel", default="k_setupILb1ELb1E", help="substring of the mangled kernel name")
    ap.add_argument("--store", default="", help="the summary counts the hops in front of the first store behind a wait whose mnemonic contains "
                                                "this (k_setup's record store: dwordx4; default: any store)")
    a = ap.parse_args()
    lines = open(a.listing).read().split("\n")
    start, end = kernel_span(lines, a.kernel)
    print(f"kernel {lines[start].split(':')[0]}")
    n_load = n_bytes = hops = since_wait = n_wait = n_barrier = n_atomic = 0
    first_store = None
    hops_at_store = loads_at_store = None
    for i in range(start + 1, end):
        t = lines[i].split(";")[0].strip()
        if not t or t.startswith(".") or t.endswith(":"):
            continue
        op = t.split()[0]
        rest = t[len(op):].strip()
        m = LOAD.match(op)
        if m:
            w = WIDTH.get(m.group(2))
            off = re.search(r"offset:(-?\d+)", rest)
            n_load += 1
            n_bytes += w or 0
            since_wait += 1
            print(f"  {i + 1:6d}  load    {op:26s} {str(w) + ' B' if w else '?':>5s}{'  offset:' + off.group(1) if off else ''}")
            continue
        m = ATOMIC.match(op)
        if m:
            returning = " sc0" in " " + rest or " glc" in " " + rest
            if returning:
                n_atomic += 1
                since_wait += 1
                print(f"  {i + 1:6d}  atomic  {op:26s} (returns)")
            continue
        if op == "s_waitcnt" and "vmcnt" in rest:
            n_wait += 1
            new_hop = since_wait > 0
            hops += new_hop
            print(f"  {i + 1:6d}  wait    {rest:32s}{'<- hop ' + str(hops) + ' (' + str(since_wait) + ' in flight since the last wait)' if new_hop else ''}")
            since_wait = 0
            continue
        if op in ("s_barrier", "s_barrier_wait", "s_barrier_signal"):
            n_barrier += 1
            print(f"  {i + 1:6d}  barrier {op}")
            continue
        if STORE.match(op):      # (a store in front of every wait -- a zero-fill at the kernel's head -- depends on no load)
            print(f"  {i + 1:6d}  store   {op:26s} ({hops} hop(s), {n_load} load(s) in front of it)")
            if first_store is None and hops > 0 and a.store in op:
                first_store = i + 1
                hops_at_store, loads_at_store = hops, n_load
    foot = {}
    for l in lines[end:end + 60]:
        m = re.match(r";\s*(NumVgprs|NumAgprs|TotalNumVgprs|ScratchSize|Occupancy|LDSByteSize|NumSgprs):\s*(\d+)", l)
        if m and m.group(1) not in foot:
            foot[m.group(1)] = int(m.group(2))
    scratch_ops = sum(1 for i in range(start + 1, end) if re.match(r"\s*scratch_", lines[i]))
    print(f"summary: {n_load} vector loads ({n_bytes} B per lane), {n_atomic} returning atomics, {n_wait} vmcnt waits, {n_barrier} barriers; "
          f"in front of the first {a.store + ' ' if a.store else ''}store behind a wait: {loads_at_store} loads in {hops_at_store} hop(s)" if first_store else
          f"summary: {n_load} vector loads ({n_bytes} B per lane), {n_atomic} returning atomics, {n_wait} vmcnt waits, {n_barrier} barriers; no vector store")
    print("resources: " + ", ".join(f"{k} {v}" for k, v in foot.items()) + f"; scratch_ instructions: {scratch_ops}")


if __name__ == "__main__":
    main()
