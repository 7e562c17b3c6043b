#!/usr/bin/env python3
"""tools_dev/kernel_meta.py LIB.so [OTHER.so] -- the code-object metadata of every kernel in a built library, without a GPU.

Takes the library's .hip_fatbin section apart (one clang offload bundle per translation unit), reads the notes and the symbol
table of each gfx950 code object with the ROCm llvm tools and prints one line per kernel: VGPRs, AGPRs, SGPRs, LDS bytes, scratch
bytes, code bytes.  With two libraries: the kernels of the first that the second lacks, has in addition, or holds with other figures
-- `identical` is what a change that must not touch the production kernels has to show (profiles/tests/libm_hooks_kernel_meta.txt).
"""
import os
import re
import struct
import subprocess
import sys
import tempfile

LLVM = os.environ.get("ROCM_LLVM", "/opt/rocm/llvm/bin")
MAGIC = b"__CLANG_OFFLOAD_BUNDLE__"
FIELDS = ("vgpr", "agpr", "sgpr", "lds", "scratch", "code")


def code_objects(lib, arch="gfx950"):
    with tempfile.TemporaryDirectory() as tmp:
        fat = os.path.join(tmp, "fatbin")
        subprocess.check_call([os.path.join(LLVM, "llvm-objcopy"), "--dump-section", ".hip_fatbin=" + fat, lib, os.path.join(tmp, "copy")])
        data = open(fat, "rb").read()
    for m in re.finditer(re.escape(MAGIC), data):
        at = m.start()
        (count,) = struct.unpack_from("<Q", data, at + len(MAGIC))
        pos = at + len(MAGIC) + 8
        for _ in range(count):
            off, size, tlen = struct.unpack_from("<QQQ", data, pos)
            triple = data[pos + 24: pos + 24 + tlen].decode()
            pos += 24 + tlen
            if triple.startswith("hip") and triple.endswith(arch) and size:
                yield data[at + off: at + off + size]


def kernels(lib):
    out = {}
    for elf in code_objects(lib):
        with tempfile.NamedTemporaryFile(suffix=".co") as f:
            f.write(elf)
            f.flush()
            notes = subprocess.check_output([os.path.join(LLVM, "llvm-readelf"), "--notes", f.name], text=True)
            syms = subprocess.check_output([os.path.join(LLVM, "llvm-readelf"), "-sW", f.name], text=True)
        size = {}
        for line in syms.splitlines():
            p = line.split()
            if len(p) == 8 and p[3] == "FUNC":
                size[p[7]] = int(p[2], 0)
        for block in notes.split("  - .agpr_count:")[1:]:
            get = lambda key: int(re.search(r"\.%s:\s+(\d+)" % key, block).group(1))  # noqa: E731
            name = re.search(r"\.name:\s+(\S+)", block).group(1)
            key, copy = name, 1
            while key in out:  # a template kernel that several translation units instantiate: one copy per code object, in link order
                copy += 1
                key = "%s [copy %d]" % (name, copy)
            out[key] = (get("vgpr_count"), int(block.split()[0]), get("sgpr_count"), get("group_segment_fixed_size"),
                         get("private_segment_fixed_size"), size[name])
    return out


def demangle(names):
    for tool in (os.path.join(LLVM, "llvm-cxxfilt"), "c++filt"):
        try:
            txt = subprocess.run([tool], input="\n".join(names), capture_output=True, text=True)
        except OSError:
            continue
        if txt.returncode == 0 and len(txt.stdout.splitlines()) == len(names):
            return dict(zip(names, txt.stdout.splitlines()))
    return {n: n for n in names}  # no demangler on this machine: the mangled names


def main(argv):
    a = kernels(argv[1])
    nice = demangle(sorted(a))
    if len(argv) == 2:
        print("%-6s %-6s %-6s %-8s %-8s %-8s kernel" % FIELDS)
        for n in sorted(a, key=nice.get):
            print("%-6d %-6d %-6d %-8d %-8d %-8d %s" % (a[n] + (nice[n],)))
        return 0
    b = kernels(argv[2])
    nice.update(demangle(sorted(set(b) - set(a))))
    changed = [n for n in a if n in b and a[n] != b[n]]
    print("%d kernels in %s, %d in %s" % (len(a), argv[1], len(b), argv[2]))
    for n in sorted(set(a) - set(b)):
        print("only in the first:  %s" % nice[n])
    for n in sorted(set(b) - set(a)):
        print("only in the second: %s  %s" % (nice[n], dict(zip(FIELDS, b[n]))))
    for n in changed:
        print("differs: %s\n  first  %s\n  second %s" % (nice[n], dict(zip(FIELDS, a[n])), dict(zip(FIELDS, b[n]))))
    print("the %d kernels of the first that the second has: %s" % (len(set(a) & set(b)), "DIFFER in %d" % len(changed) if changed else "identical"))
    return 1 if changed or set(a) - set(b) else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
