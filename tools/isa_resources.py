"""Per-kernel resources of the built library (pixelrec_amd/libpxr.so): scratch bytes (.private_segment_fixed_size), VGPRs, SGPRs,
static LDS -- read from the AMDGPU metadata notes of the gfx950 code objects inside the fat binary (clang offload bundles, one per
translation unit), through llvm-readelf.  usage: python tools/isa_resources.py [regex]      (also imported by tests/test_abi.py)"""
import os
import re
import struct
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
READELF = "/opt/rocm/lib/llvm/bin/llvm-readelf"
CXXFILT = "c++filt"               # binutils (this image has no llvm-cxxfilt)
MAGIC = b"__CLANG_OFFLOAD_BUNDLE__"


def code_objects(so_path):
    """[(bytes of a gfx950 code object)] of every offload bundle in the shared library."""
    data = open(so_path, "rb").read()
    out = []
    for m in re.finditer(MAGIC, data):
        o = m.start()
        n = struct.unpack_from("<Q", data, o + 24)[0]
        p = o + 32
        for _ in range(n):
            off, size, tl = struct.unpack_from("<QQQ", data, p)
            p += 24
            triple = data[p:p + tl].decode()
            p += tl
            if "gfx950" in triple and size:
                out.append(data[o + off:o + off + size])
    return out


def kernel_resources(so_path=None):
    """{demangled kernel name: dict(scratch=bytes per lane, vgpr=, agpr=, sgpr=, lds=static bytes)}."""
    so_path = so_path or os.path.join(ROOT, "pixelrec_amd", "libpxr.so")
    res = {}
    for blob in code_objects(so_path):
        with tempfile.NamedTemporaryFile(suffix=".co") as f:
            f.write(blob)
            f.flush()
            txt = subprocess.run([READELF, "--notes", f.name], capture_output=True, text=True, check=True).stdout
        # the metadata is YAML-like: one "- .agpr_count: ..." block per kernel; keys are sorted, .name sits in the middle
        for block in re.split(r"\n\s*- \.agpr_count:", txt)[1:]:
            block = ".agpr_count:" + block
            get = lambda key, default=0: (lambda mm: int(mm.group(1)) if mm else default)(re.search(r"\.%s:\s+(\d+)" % key, block))
            name = re.search(r"\n\s*\.name:\s+(\S+)", block)
            if not name:
                continue
            res[name.group(1)] = dict(scratch=get("private_segment_fixed_size"), vgpr=get("vgpr_count"), agpr=get("agpr_count"),
                                      sgpr=get("sgpr_count"), lds=get("group_segment_fixed_size"))
    names = list(res)
    dem = subprocess.run([CXXFILT], input="\n".join(names), capture_output=True, text=True, check=True).stdout.splitlines()
    return {d: res[n] for n, d in zip(names, dem)}


def kernel_code(path):
    """{demangled kernel name: (code bytes, sha256 of them)} of the gfx950 code objects in `path` (the library or one object file):
    the bytes of .text that each kernel's function symbol spans.  Equal hashes = the same instructions, byte for byte."""
    import hashlib

    code = {}
    for blob in code_objects(path):
        with tempfile.NamedTemporaryFile(suffix=".co") as f:
            f.write(blob)
            f.flush()
            txt = subprocess.run([READELF, "-S", "--symbols", "--wide", f.name], capture_output=True, text=True, check=True).stdout
        sec = re.search(r"\]\s+\.text\s+PROGBITS\s+([0-9a-f]+)\s+([0-9a-f]+)\s+([0-9a-f]+)", txt)
        if not sec:
            continue
        addr, off = int(sec.group(1), 16), int(sec.group(2), 16)
        kernels = set(re.findall(r"\s(\S+)\.kd\s*$", txt, re.M))
        for m in re.finditer(r"^\s*\d+:\s+([0-9a-f]+)\s+(\d+)\s+FUNC\s+\S+\s+\S+\s+\d+\s+(\S+)\s*$", txt, re.M):
            if m.group(3) in kernels:
                b = blob[off + int(m.group(1), 16) - addr:][:int(m.group(2))]
                code[m.group(3)] = (len(b), hashlib.sha256(b).hexdigest()[:16])
    names = list(code)
    dem = subprocess.run([CXXFILT], input="\n".join(names), capture_output=True, text=True, check=True).stdout.splitlines()
    return {d: code[n] for n, d in zip(names, dem)}


if __name__ == "__main__":
    # usage: isa_resources.py [--file PATH]... [regex]: with --file, the named libraries / object files, code hashes included
    args, files = sys.argv[1:], []
    while args[:1] == ["--file"]:
        files.append(args[1])
        args = args[2:]
    pat = re.compile(args[0]) if args else None
    rows = {}
    for path in files or [None]:
        res, code = kernel_resources(path), (kernel_code(path) if files else {})
        rows.update({name: (r, code.get(name)) for name, r in res.items()})
    for name, (r, c) in sorted(rows.items(), key=lambda kv: (-kv[1][0]["scratch"], kv[0])):
        if pat is None or pat.search(name):
            tail = "  %6d B code %s" % c if c else ""
            print("%5d B scratch  %3d vgpr %3d agpr %3d sgpr %6d lds%s  %s" % (r["scratch"], r["vgpr"], r["agpr"], r["sgpr"], r["lds"], tail, name[:150]))
