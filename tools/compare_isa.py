#!/usr/bin/env python3
"""Per-kernel comparison of the device code of two builds of libtt_hip.so (a refactor's gate: same machine code).

    python3 tools/compare_isa.py OLD/libtt_hip.so NEW/libtt_hip.so

Disassembles both libraries (csrc/check_isa.device_disassembly), splits the text at the `<symbol>:` lines and compares the
instruction streams symbol by symbol: mnemonics, operands and encodings, without the addresses.  A symbol that several
translation units define (a kernel in an anonymous namespace of a file compiled twice) is compared as a multiset of bodies.
Prints the counts and every symbol that is new, gone or different; exit status 1 when any body differs.
"""
from __future__ import annotations

import collections
import os
import re
import sys
import tempfile

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tensor-truth_amd", "csrc"))
import check_isa  # noqa: E402

SYMBOL = re.compile(r"^[0-9a-f]+ <(.+)>:$")
ADDRESS = re.compile(r"//\s*[0-9A-Fa-f]+:")
TARGET = re.compile(r"\s*<[^>]+\+0x[0-9a-f]+>$")     # a branch target's label (the offset is in the encoding)


def kernels(lib: str) -> dict:
    with tempfile.TemporaryDirectory() as tmp:
        text = check_isa.device_disassembly(lib, tmp)
    out, name, body = collections.defaultdict(list), None, []
    for line in text.splitlines():
        if "file format" in line or not line.strip() or line.startswith("Disassembly of section"):
            continue
        if line.strip() == "...":     # llvm-objdump's mark for zero padding behind a function: depends on where its neighbour starts
            continue
        m = SYMBOL.match(line)
        if m:
            if name is not None:
                out[name].append("\n".join(body))
            name, body = m.group(1), []
        elif name is not None:
            body.append(TARGET.sub("", ADDRESS.sub("//", line).strip()))
    if name is not None:
        out[name].append("\n".join(body))
    return out


def main(argv) -> int:
    old, new = kernels(argv[1]), kernels(argv[2])
    gone = sorted(set(old) - set(new))
    added = sorted(set(new) - set(old))
    differ = sorted(n for n in set(old) & set(new) if sorted(old[n]) != sorted(new[n]))
    same = len(set(old) & set(new)) - len(differ)
    print(f"symbols: old {len(old)} ({sum(map(len, old.values()))} bodies), new {len(new)} ({sum(map(len, new.values()))} bodies); "
          f"identical {same}, different {len(differ)}, gone {len(gone)}, new {len(added)}")
    for title, names in (("different", differ), ("gone", gone), ("new", added)):
        for n in names:
            print(f"  {title}: {n}")
    # a symbol that is gone and one that is new with the same body: a renamed or moved kernel
    for g in gone:
        for a in added:
            if sorted(old[g]) and set(old[g]) & set(new[a]):
                print(f"  same body: {g} -> {a}")
    return 1 if differ else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
