#!/usr/bin/env python3
"""(CPU) Is the device code of a HIP source the same at a revision and in the working tree?

    python tools/device_code_diff.py <rev> <file.hip>

Compiles `<file.hip>` to device assembly (the Makefile's compiler and flags plus `--cuda-device-only -S`) twice: from
`git archive <rev>` of its directory and `include/`, unpacked into a temporary directory, and from the working tree. The
`__hip_cuid_<hash>` symbol (a hash of the source file) is normalised; then the two outputs must be the same text. If only
the ORDER of the functions differs (a changed order of template instantiation), the per-function blocks, with the function
ordinal taken out of their local labels, are compared as a set. Prints "identical" (exit 0) or the first function that
differs (exit 1). The check behind every "host-only change" of a kernel file."""
from __future__ import annotations

import io
import os
import re
import subprocess
import sys
import tarfile
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def makefile_flags(csrc: str) -> tuple[str, list[str]]:
    """-> (compiler, flags) as `make` would use them for a .hip file of `csrc`."""
    text = open(os.path.join(csrc, "Makefile")).read()
    var = {k: v.strip() for k, v in re.findall(r"^(\w+)\s*\??=\s*(.*)$", text, re.M)}
    flags = re.sub(r"\$\((\w+)\)", lambda m: var[m.group(1)], var["CXXFLAGS"])
    return os.environ.get("HIPCC", var["HIPCC"]), flags.split()


def device_asm(src: str, out: str) -> str:
    hipcc, flags = makefile_flags(os.path.dirname(src))
    subprocess.run([hipcc, *flags, "--cuda-device-only", "-S", os.path.basename(src), "-o", out],
                   cwd=os.path.dirname(src), check=True)
    text = open(out).read()
    return re.sub(r"__hip_cuid_[0-9a-f]+", "__hip_cuid_", text)


def blocks(text: str) -> dict[str, str]:
    """function name -> its text with the function ordinal removed from local labels; "" -> everything before the first
    function; "<metadata>" -> the sorted per-kernel entries of the trailing metadata."""
    pieces = re.split(r"^(?=\t\.globl\t\S+\s*; -- Begin function)", text, flags=re.M)
    for i in range(len(pieces) - 1):   # a function's own `.section .text.<name>` / `.text` line precedes its `.globl`
        m = re.search(r"(?:\t\.section\t\.text\S*|\t\.text)\n\Z", pieces[i])
        if m:
            pieces[i], pieces[i + 1] = pieces[i][:m.start()], m.group(0) + pieces[i + 1]
    out = {"": pieces[0]}
    for blk in pieces[1:]:
        name = re.search(r"^\t\.globl\t(\S+)", blk, re.M).group(1)
        if "\t.amdgpu_metadata" in blk:   # the last function carries the module's tail
            blk, meta = blk.split("\t.amdgpu_metadata", 1)
            out["<metadata>"] = "\n".join(sorted(re.split(r"^(?=  - \.)", meta, flags=re.M)))
        blk = re.sub(r"\.(LBB|Lfunc_end|Lfunc_begin|Ltmp)\d+", r".\1", blk)
        out[name] = re.sub(r"\bBB\d+_", "BB_", blk)   # (the same ordinal in the block comments)
    return out


def main() -> int:
    if len(sys.argv) != 3:
        print(__doc__)
        return 2
    rev, path = sys.argv[1], os.path.relpath(os.path.abspath(sys.argv[2]), ROOT)
    with tempfile.TemporaryDirectory() as tmp:
        tar = subprocess.run(["git", "archive", rev, os.path.dirname(path), "include"], cwd=ROOT, check=True,
                             capture_output=True).stdout
        tarfile.open(fileobj=io.BytesIO(tar)).extractall(os.path.join(tmp, "rev"))
        old = device_asm(os.path.join(tmp, "rev", path), os.path.join(tmp, "old.s"))
        new = device_asm(os.path.join(ROOT, path), os.path.join(tmp, "new.s"))
    n_fn = len(re.findall(r"^\t\.amdhsa_kernel ", new, re.M))
    if old == new:
        print(f"identical: {path} at {rev} and in the working tree ({n_fn} kernels, {new.count(chr(10))} lines)")
        return 0
    a, b = blocks(old), blocks(new)
    for name in sorted(set(a) | set(b)):
        if a.get(name) != b.get(name):
            what = "only at " + rev if name not in b else "only in the working tree" if name not in a else "differs"
            print(f"DIFFERENT: {name or '<module preamble>'} {what}")
            return 1
    print(f"identical up to the order of the functions: {path} at {rev} and in the working tree ({n_fn} kernels)")
    return 0


if __name__ == "__main__":
    sys.exit(main())
