#!/usr/bin/env python3
"""device_code_diff.py OLD_DIR NEW_DIR: do two versions of the library compile to the same gfx950 kernels?

OLD_DIR / NEW_DIR are two checkouts (or their acr_wsss_amd/csrc directories).  Every *.hip of each is compiled device-only with
the Makefile's flags, unbundled, and every kernel (a FUNC symbol with a `<name>.kd` OBJECT) is reduced to the bytes of its
function in .text plus its 64-byte descriptor with bytes 16..23 masked (the descriptor-to-entry offset moves with layout).
Kernels are keyed by mangled name over the union of translation units, so a kernel may change file.  Reports kernels only in
OLD, only in NEW, emitted by more than one translation unit, whose code or descriptor differ, and FUNC symbols that are not
kernels (a helper that was not inlined).  The 32-bit literals of an `s_getpc_b64; s_add_u32; s_addc_u32` address of a data symbol
are masked as well (the distance to the symbol moves with layout; crf.hip's rocprim sort has the library's only one).
Exit status 0 only if nothing differs.  Host only: no GPU, nothing but the ROCm tools."""
import glob
import os
import re
import struct
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

ROCM = os.environ.get("ROCM_PATH", "/opt/rocm")
HIPCC, LLVM = os.path.join(ROCM, "bin", "hipcc"), os.path.join(ROCM, "llvm", "bin")
TARGET = "hipv4-amdgcn-amd-amdhsa--gfx950"
FLAGS = ["-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-ffp-contract=off", "-Wall", "-Wno-unused-function"]   # csrc/Makefile


def csrc_of(d):
    sub = os.path.join(d, "acr_wsss_amd", "csrc")
    return os.path.abspath(sub if os.path.isdir(sub) else d)


def kernels_of(src, tmp):
    """{mangled name: (code bytes, masked descriptor)} and the non-kernel FUNC names of one translation unit."""
    stem = os.path.join(tmp, os.path.basename(src))
    subprocess.check_call([HIPCC, *FLAGS, "--offload-device-only", "-c", src, "-o", stem + ".bundle"], cwd=os.path.dirname(src))
    subprocess.check_call([os.path.join(LLVM, "clang-offload-bundler"), "--unbundle", "--type=o", "--targets=" + TARGET,
                           "--input=" + stem + ".bundle", "--output=" + stem + ".elf"])
    readelf = lambda opt: subprocess.check_output([os.path.join(LLVM, "llvm-readelf"), opt, stem + ".elf"], text=True)
    sect = {}                                   # section index -> (address, file offset)
    for m in re.finditer(r"^\s*\[\s*(\d+)\]\s+\S+\s+\S+\s+([0-9a-f]+)\s+([0-9a-f]+)\s+[0-9a-f]+", readelf("-SW"), re.M):
        sect[m.group(1)] = (int(m.group(2), 16), int(m.group(3), 16))
    blob = open(stem + ".elf", "rb").read()
    funcs, descs = {}, {}
    for line in readelf("-sW").splitlines():
        f = line.split()
        if len(f) == 8 and f[3] in ("FUNC", "OBJECT") and f[6] in sect:
            addr, off = sect[f[6]]
            at = int(f[1], 16) - addr + off
            (funcs if f[3] == "FUNC" else descs)[f[7]] = blob[at:at + int(f[2], 0)]
    out = {}
    for name, code in funcs.items():
        kd = descs.get(name + ".kd")
        if kd is not None and len(kd) == 64:
            out[name] = (mask_pcrel(code), kd[:16] + bytes(8) + kd[24:])
    return out, sorted(set(funcs) - set(out))


def mask_pcrel(code):
    """code with the literals of `s_getpc_b64 s[n:n+1]; s_add_u32 .., literal; s_addc_u32 .., literal` zeroed"""
    w = list(struct.unpack("<%dI" % (len(code) // 4), code))
    for i in range(len(w) - 4):
        if (w[i] & 0xff80ffff) == 0xbe801c00 and w[i + 1] >> 23 == 0x100 and w[i + 3] >> 23 == 0x104 and (w[i + 1] >> 8) & 255 == (w[i + 3] >> 8) & 255 == 255:
            w[i + 2] = w[i + 4] = 0
    return struct.pack("<%dI" % len(w), *w)


def library(d, tmp, pool):
    tmp = tempfile.mkdtemp(dir=tmp)
    srcs = sorted(glob.glob(os.path.join(csrc_of(d), "*.hip")))
    kernels, emitted, stray = {}, {}, []
    for src, (ks, other) in zip(srcs, pool.map(lambda s: kernels_of(s, tmp), srcs)):
        stray += ["%s: %s" % (os.path.basename(src), n) for n in other]
        for name, k in ks.items():
            emitted.setdefault(name, []).append(os.path.basename(src))
            kernels.setdefault(name, k)
            if kernels[name] != k:
                stray.append("%s: %s differs from its copy in %s" % (os.path.basename(src), name, emitted[name][0]))
    return kernels, emitted, stray


def resources(kd):
    """VGPR / SGPR granule fields, LDS and scratch bytes of a kernel descriptor (amdhsa_kernel_descriptor_t)."""
    lds, scratch = struct.unpack_from("<II", kd, 0)
    rsrc1 = struct.unpack_from("<I", kd, 48)[0]
    return "vgpr_gran=%d sgpr_gran=%d lds=%d scratch=%d" % (rsrc1 & 63, (rsrc1 >> 6) & 15, lds, scratch)


def main():
    if len(sys.argv) != 3:
        sys.exit(__doc__)
    with tempfile.TemporaryDirectory() as tmp, ThreadPoolExecutor(min(16, os.cpu_count() or 1)) as pool:
        (old, old_tu, old_stray), (new, new_tu, new_stray) = (library(d, tmp, pool) for d in sys.argv[1:])
    bad = 0
    for tag, names in (("only in OLD", set(old) - set(new)), ("only in NEW", set(new) - set(old))):
        for n in sorted(names):
            bad += 1
            print("%s: %s" % (tag, n))
    for tag, msgs in (("OLD", old_stray), ("NEW", new_stray)):
        for m in msgs:
            bad += 1
            print("%s, FUNC that is not one kernel: %s" % (tag, m))
    for n in sorted(set(old_tu) | set(new_tu)):
        a, b = old_tu.get(n, []), new_tu.get(n, [])
        if len(a) > 1 or len(b) > 1:
            bad += len(b) > 1
            print("emitted by %d translation units in OLD, %d in NEW: %s" % (len(a), len(b), n))
    for n in sorted(set(old) & set(new)):
        if old[n] != new[n]:
            bad += 1
            print("differs: %s\n  OLD code %d B, %s\n  NEW code %d B, %s" %
                  (n, len(old[n][0]), resources(old[n][1]), len(new[n][0]), resources(new[n][1])))
    print("%d kernels in OLD, %d in NEW, %d findings" % (len(old), len(new), bad))
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
