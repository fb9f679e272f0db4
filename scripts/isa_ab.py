"""Kernel-by-kernel A/B of the gfx950 instruction streams of two builds of one object.

    python scripts/isa_ab.py OLD.o NEW.o [NAME_REGEX]

Unbundles the device image of each hipcc object, disassembles it, and compares every kernel whose name matches NAME_REGEX (default: all)
after stripping what a move of source text changes without changing the code: symbol names (the anonymous namespace's hash, template
arguments' spelling), addresses, encodings and comments.  Prints identical / DIFFERENT with the instruction counts, and VGPR / SGPR /
LDS / private-segment figures of both from the code-object notes.  ISA_AB_RENAME="old=new,..." compares a renamed kernel pairwise (short
names as printed); ISA_AB_DIFF=N prints the first N lines of each difference.  Needs no GPU."""
import difflib
import os
import re
import subprocess
import sys
import tempfile

LLVM = "/opt/rocm/lib/llvm/bin"


def device_image(obj, tmp, tag):
    fb, co = os.path.join(tmp, tag + ".fb"), os.path.join(tmp, tag + ".co")
    subprocess.check_call([f"{LLVM}/llvm-objcopy", f"--dump-section=.hip_fatbin={fb}", obj], stderr=subprocess.DEVNULL)
    subprocess.check_call([f"{LLVM}/clang-offload-bundler", "--type=o", "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", f"--input={fb}",
                           f"--output={co}", "--unbundle"], stderr=subprocess.DEVNULL)
    return co


def short(name):
    """k_name or k_name<0|1> of a mangled kernel symbol (one bool template argument at the most); anything else as it is"""
    m = re.search(r"(?:_GLOBAL__N_1|^_Z)(\d+)(k_\w+)", name)
    if not m:
        return name
    n = int(m.group(1))
    t = re.match(r"IL[bi]([01])E", m.group(2)[n:])
    return m.group(2)[:n] + (f"<{t.group(1)}>" if t else "")


def kernels(co):
    """{short name: [instruction, ...]} and {short name: resources} of a code object"""
    notes = subprocess.check_output([f"{LLVM}/llvm-readelf", "--notes", co], text=True)
    res = {}
    for blk in re.split(r"\n\s*- \.agpr_count", notes)[1:]:
        g = lambda k: int(re.search(r"\." + k + r":\s*(\d+)", blk).group(1))
        res[short(re.search(r"\.name:\s*(\S+)", blk).group(1))] = (
            f"vgpr {g('vgpr_count')} sgpr {g('sgpr_count')} lds {g('group_segment_fixed_size')} private {g('private_segment_fixed_size')}")
    dis = subprocess.check_output([f"{LLVM}/llvm-objdump", "-d", "--no-show-raw-insn", "--no-leading-addr", co], text=True)
    code, cur = {}, None
    for line in dis.splitlines():
        m = re.match(r"^(?:[0-9a-f]+ )?<(\S+)>:$", line.strip())
        if m:
            cur = short(m.group(1)) if not m.group(1).startswith("L") else cur
            if cur is not None and not m.group(1).startswith("L"):
                code[cur] = []
            continue
        ins = re.sub(r"\s*//.*$", "", line).strip()
        if cur is None or not ins:
            continue
        ins = re.sub(r"<[^>]*>", "<L>", ins)              # branch targets by symbol
        ins = re.sub(r"\s+", " ", ins)
        code[cur].append(ins)
    for v in code.values():                               # the padding behind a kernel's last instruction
        while v and v[-1] in ("s_nop 0", "..."):
            v.pop()
    return {k: v for k, v in code.items() if k in res}, res


def main():
    old, new = sys.argv[1], sys.argv[2]
    pat = re.compile(sys.argv[3] if len(sys.argv) > 3 else ".")
    with tempfile.TemporaryDirectory() as tmp:
        co, ro = kernels(device_image(old, tmp, "old"))
        cn, rn = kernels(device_image(new, tmp, "new"))
    for pair in filter(None, os.environ.get("ISA_AB_RENAME", "").split(",")):      # a kernel of OLD under its name in NEW
        was, now = pair.split("=")
        co[now], ro[now] = co.pop(was), ro.pop(was)
    same = True
    for k in sorted(set(co) | set(cn)):
        if not pat.search(k):
            continue
        a, b = co.get(k), cn.get(k)
        if a is None or b is None:
            print(f"{k:32s} only in {'old' if b is None else 'new'}")
            same = False
            continue
        verdict = "identical" if a == b else "DIFFERENT"
        same = same and a == b
        print(f"{k:32s} {verdict:9s} instructions {len(a)} -> {len(b)}   old: {ro[k]}   new: {rn[k]}")
        if a != b and os.environ.get("ISA_AB_DIFF"):
            for l in list(difflib.unified_diff(a, b, "old", "new", n=2, lineterm=""))[:int(os.environ["ISA_AB_DIFF"])]:
                print("    " + l)
    return 0 if same else 1


if __name__ == "__main__":
    sys.exit(main())
