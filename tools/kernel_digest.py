#!/usr/bin/env python3
"""Per-kernel digests of a gfx950 device code object, and a comparison against a parent's.  CPU only.

    tools/kernel_digest.py tokenreduction_amd/csrc/tr_attention.hip
    tools/kernel_digest.py tokenreduction_amd/csrc/tr_attention.hip --against parent.o \\
        --rename 'attention_kernel<(\\d), false, true, true>=attention_policy_kernel<\\1>'

A .hip argument is compiled device-only with the flags csrc/Makefile uses for that file; a device ELF is read as it is.
One line per kernel: code size, sha256 of its code bytes, sha256 of its 64-byte kernel descriptor (.kd), demangled name.
Descriptor bytes 16..23 -- the code-entry offset, which moves when neighbouring kernels come or go -- are zeroed before
hashing.  A refactor that must not move bits or speed shows it here before any GPU run: every kernel it keeps is "identical".

--against pairs each kernel with the parent's: by name, then by the --rename table (OLD=NEW, OLD a regular expression that
must match a parent kernel's whole name, without namespace and parameter list), then by identical (size, digests).
Exit status 1 if any kernel is differing or new.
"""
import argparse
import hashlib
import os
import re
import shutil
import subprocess
import sys
import tempfile

LLVM = os.environ.get("ROCM_LLVM_BIN", "/opt/rocm/llvm/bin")
CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tokenreduction_amd", "csrc")


def makefile_flags(hip_path):
    """CXXFLAGS of csrc/Makefile for this file, target-specific additions included."""
    text = open(os.path.join(CSRC, "Makefile")).read()
    var = lambda name, default: (re.search(rf"^{name}\s*\?=\s*(.*)$", text, re.M) or [None, default])[1].strip()
    flags = re.search(r"^CXXFLAGS\s*=\s*(.*)$", text, re.M).group(1)
    stem = os.path.splitext(os.path.basename(hip_path))[0]
    for extra in re.findall(rf"^{re.escape(stem)}\.o:\s*CXXFLAGS\s*\+=\s*(.*)$", text, re.M):
        flags += " " + extra
    hipcc = os.environ.get("HIPCC", var("HIPCC", "/opt/rocm/bin/hipcc"))
    return hipcc, flags.replace("$(ARCH)", os.environ.get("ARCH", var("ARCH", "gfx950"))).split()


def device_elf(path, tmp):
    with open(path, "rb") as f:
        if f.read(4) == b"\x7fELF":
            return path
    hipcc, flags = makefile_flags(path)
    out = os.path.join(tmp, os.path.basename(path) + ".device.o")
    subprocess.run([hipcc, *flags, "--cuda-device-only", "--no-gpu-bundle-output", "-c", os.path.abspath(path), "-o", out],
                   check=True, cwd=os.path.dirname(os.path.abspath(path)))
    return out


def readelf(*args):
    return subprocess.run([os.path.join(LLVM, "llvm-readelf"), "--wide", *args], check=True, capture_output=True, text=True).stdout


def kernels(elf):
    """{short demangled name: (code size, code sha256, descriptor sha256)}"""
    sections = {}          # index -> (address, file offset)
    for m in re.finditer(r"^\s*\[\s*(\d+)\]\s+\S*\s+\S+\s+([0-9a-f]{16})\s+([0-9a-f]+)\s+[0-9a-f]+", readelf("-S", elf), re.M):
        sections[int(m.group(1))] = (int(m.group(2), 16), int(m.group(3), 16))
    syms = {}              # mangled name -> (value, size, section index)
    for m in re.finditer(r"^\s*\d+:\s+([0-9a-f]{16})\s+(\d+)\s+(FUNC|OBJECT)\s+\S+\s+\S+\s+(\d+)\s+(\S+)$", readelf("-s", elf), re.M):
        syms[m.group(5)] = (int(m.group(1), 16), int(m.group(2)), int(m.group(4)))
    names = sorted(n[:-3] for n in syms if n.endswith(".kd") and n[:-3] in syms)
    cxxfilt = shutil.which("llvm-cxxfilt", path=LLVM) or shutil.which("llvm-cxxfilt") or shutil.which("c++filt")
    plain = subprocess.run([cxxfilt], input="\n".join(names), check=True, capture_output=True, text=True).stdout.split("\n")
    blob = open(elf, "rb").read()

    def content(sym):
        value, size, ndx = syms[sym]
        addr, off = sections[ndx]
        return blob[off + value - addr: off + value - addr + size]

    out = {}
    for mangled, full in zip(names, plain):
        kd = bytearray(content(mangled + ".kd"))
        assert len(kd) == 64, (mangled, len(kd))
        kd[16:24] = bytes(8)
        code = content(mangled)
        out[short_name(full)] = (len(code), hashlib.sha256(code).hexdigest(), hashlib.sha256(kd).hexdigest())
    return out


def short_name(demangled):
    """without the parameter list and the anonymous namespace: attention16_kernel<7, false, true, true>"""
    name = demangled.replace("(anonymous namespace)::", "")
    depth = 0
    for i, c in enumerate(name):
        depth += (c == "<") - (c == ">")
        if c == "(" and depth == 0:
            return name[:i].split(" ", 1)[-1] if name.startswith("void ") else name[:i]
    return name


def line(name, k):
    return f"{k[0]:7d}  {k[1][:16]}  {k[2][:16]}  {name}"


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("file", help=".hip source (compiled with the Makefile's flags) or device ELF")
    ap.add_argument("--against", metavar="PARENT", help="the parent's .hip source or device ELF")
    ap.add_argument("--rename", action="append", default=[], metavar="OLD=NEW", help="parent kernel name (regular expression) = its name here")
    args = ap.parse_args()
    with tempfile.TemporaryDirectory() as tmp:
        mine = kernels(device_elf(args.file, tmp))
        if not args.against:
            for name in sorted(mine):
                print(line(name, mine[name]))
            return 0
        parent = kernels(device_elf(args.against, tmp))
    pairs = {n: n for n in parent if n in mine}                       # parent name -> name here
    for rule in args.rename:
        old, new = rule.split("=", 1)
        for n in parent:
            m = re.fullmatch(old, n)
            if m and n not in pairs and m.expand(new) in mine and m.expand(new) not in pairs.values():
                pairs[n] = m.expand(new)
    for n in sorted(set(parent) - set(pairs)):
        twins = [k for k in sorted(mine) if k not in pairs.values() and mine[k] == parent[n]]
        if twins:
            pairs[n] = twins[0]
    groups = {"identical": [], "differing": [], "gone": [], "new": []}
    for n in sorted(parent):
        if n not in pairs:
            groups["gone"].append(line(n, parent[n]))
        else:
            same = parent[n] == mine[pairs[n]]
            renamed = "" if pairs[n] == n else f"   (parent: {n})"
            groups["identical" if same else "differing"].append(line(pairs[n], mine[pairs[n]]) + renamed)
            if not same:
                groups["differing"].append(line("  parent's", parent[n]))
    groups["new"] = [line(n, mine[n]) for n in sorted(set(mine) - set(pairs.values()))]
    for title, rows in groups.items():
        print(f"== {title}: {len(rows) if title != 'differing' else len(rows) // 2}")
        for r in rows:
            print(r)
    return 1 if groups["differing"] or groups["new"] else 0


if __name__ == "__main__":
    sys.exit(main())
