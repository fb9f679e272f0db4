"""The kernel notes of a built HIP object, for the tests that hold a kernel to its private segment and its LDS.  Reads the
build products only: imports nothing of fpc_diffrend_amd, so the *_ref test files may use it."""
import os
import re
import shutil
import subprocess
import tempfile

LLVM = "/opt/rocm/lib/llvm/bin"
BUILD = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "fpc_diffrend_amd", "csrc", "_build")


def kernels(obj):
    """[(name, private_segment_fixed_size, group_segment_fixed_size)] of every kernel in the gfx950 code object of csrc/_build/<obj>, or
    None when the object or the llvm tools are missing (the caller skips)."""
    path = os.path.join(BUILD, obj)
    if not (os.path.exists(path) and os.path.exists(os.path.join(LLVM, "llvm-readelf"))):
        return None
    tmp = tempfile.mkdtemp()
    try:
        subprocess.check_call([f"{LLVM}/llvm-objcopy", f"--dump-section=.hip_fatbin={tmp}/fb.bin", path], stderr=subprocess.DEVNULL)
        subprocess.check_call([f"{LLVM}/clang-offload-bundler", "--type=o", "--targets=hipv4-amdgcn-amd-amdhsa--gfx950",
                               f"--input={tmp}/fb.bin", f"--output={tmp}/dev.co", "--unbundle"], stderr=subprocess.DEVNULL)
        notes = subprocess.check_output([f"{LLVM}/llvm-readelf", "--notes", f"{tmp}/dev.co"], text=True)
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    field = lambda blk, key: re.search(r"\." + key + r":\s*(\S+)", blk).group(1)
    return [(field(blk, "name"), int(field(blk, "private_segment_fixed_size")), int(field(blk, "group_segment_fixed_size")))
            for blk in re.split(r"\n\s*- \.agpr_count", notes)[1:]]
