"""CPU: the ctypes mirrors of the encoder weight structs have the layout include/tt_hip.h gives them.

A small C program compiled with the host C compiler prints ``sizeof`` and every field's ``offsetof`` and size for the eight
encoder structs; each must equal its ctypes ``Structure``, field by field and in order.  No GPU and no built library needed."""
import ctypes
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INCLUDE = os.path.join(ROOT, "include")

# header struct -> (module, name) of its ctypes mirror; each layer struct is the type the weights struct's ``layer`` points to
WEIGHT_STRUCTS = {
    "tt_encoder_weights": ("encoder", "_EncW"),
    "tt_encoder_weights_f32": ("encoder_f32", "_EncWF"),
    "tt_encoder_weights_x3": ("encoder_x3", "_EncWX"),
    "tt_encoder_weights_f16c": ("encoder_f16c", "_EncWC"),
}


def _mirrors():
    import importlib

    import tensor_truth_amd  # noqa: F401

    out = {}
    for c_name, (mod, attr) in WEIGHT_STRUCTS.items():
        S = getattr(importlib.import_module("tensor_truth_amd." + mod), attr)
        out[c_name] = S
        out[c_name.replace("encoder", "layer")] = dict(S._fields_)["layer"]._type_
    return out


def _c_fields(header: str, name: str):
    """Field names of ``typedef struct name {...} name;`` in declaration order."""
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), header, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    return [re.findall(r"\w+", d)[-1] for decl in body.split(";") if decl.strip() for d in decl.split(",")]


def _c_layouts(tmp_path, cc, fields):
    """-> {struct: (sizeof, [(field, offsetof, sizeof), ...])} as the C compiler lays them out."""
    lines = ["#include <stdio.h>", "#include <stddef.h>", '#include "tt_hip.h"', "int main(void) {"]
    for s, names in fields.items():
        lines.append(f'    printf("{s} - %zu\\n", sizeof({s}));')
        lines += [f'    printf("{s} {f} %zu %zu\\n", offsetof({s}, {f}), sizeof((({s}*)0)->{f}));' for f in names]
    lines += ["    return 0;", "}"]
    src, exe = tmp_path / "layouts.c", tmp_path / "layouts"
    src.write_text("\n".join(lines) + "\n")
    subprocess.run([cc, "-std=c99", "-I", INCLUDE, str(src), "-o", str(exe)], check=True)
    out = {s: [None, []] for s in fields}
    for line in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines():
        s, f, *nums = line.split()
        if f == "-":
            out[s][0] = int(nums[0])
        else:
            out[s][1].append((f, int(nums[0]), int(nums[1])))
    return {s: tuple(v) for s, v in out.items()}


def test_ctypes_mirrors_match_tt_hip_h(tmp_path):
    cc = next((c for c in (os.environ.get("CC"), "cc", "gcc", "clang") if c and shutil.which(c)), None)
    if cc is None:
        pytest.skip("no host C compiler")
    mirrors = _mirrors()
    assert len(mirrors) == 8
    header = open(os.path.join(INCLUDE, "tt_hip.h")).read()
    want = _c_layouts(tmp_path, cc, {s: _c_fields(header, s) for s in mirrors})
    for s, S in mirrors.items():
        got = (ctypes.sizeof(S), [(f, getattr(S, f).offset, getattr(S, f).size) for f, _ in S._fields_])
        assert got == want[s], f"{S.__name__} does not match {s} in include/tt_hip.h"
