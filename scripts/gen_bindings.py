#!/usr/bin/env python3
"""Derive the host-side FFI declarations from include/rmhip.h - the one hand-written description of the C ABI.

    python scripts/gen_bindings.py            # rewrite runmat_amd/_abi.py and shim/rmhip_sys.rs
    python scripts/gen_bindings.py --check    # exit 1 if either file is stale (tests/test_bindings.py runs this)

Emits
  runmat_amd/_abi.py   ctypes Structures, the SIGNATURES table (name -> restype, argtypes), enum / #define constants and the
                       `@serves` map (C entry point -> AccelProvider methods it implements)
  shim/rmhip_sys.rs    `#[repr(C)]` structs, the `extern "C"` block and the constants for the Rust binding
The C++ mirror (include/rmhip_provider.hpp) includes rmhip.h itself and needs no generated declarations.  What stays
hand-written is what cannot be derived: the bodies of `impl AccelProvider for HipProvider` (shim/hip_provider.rs), the
HipProvider methods (runmat_amd/provider.py) and the C++ class - tests/test_bindings.py checks that each of them
implements every method a `@serves` tag names.
"""
from __future__ import annotations

import re
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
HEADER = ROOT / "include" / "rmhip.h"
PY_OUT = ROOT / "runmat_amd" / "_abi.py"
RS_OUT = ROOT / "shim" / "rmhip_sys.rs"


def strip_comments(text: str) -> str:
    return re.sub(r"/\*.*?\*/", " ", text, flags=re.S)


def camel(typedef: str) -> str:
    core = typedef[len("rmhip_"):] if typedef.startswith("rmhip_") else typedef
    core = core[:-2] if core.endswith("_t") else core
    return "".join(p.capitalize() for p in core.split("_"))


def parse(text: str):
    serves = {}
    for m in re.finditer(r"/\*\s*@serves\s+(.*?)\s*\*/\s*RMHIP_API\s+[^;(]*?\b(rmhip_[a-z0-9_]+)\s*\(", text, flags=re.S):
        names = m.group(1).split()
        serves[m.group(2)] = [] if names == ["-"] else names
    code = strip_comments(text)
    defines = {m.group(1): int(m.group(2)) for m in re.finditer(r"#define\s+(RMHIP_[A-Z0-9_]+)\s+(\d+)\b", code)}
    enums = {}
    for m in re.finditer(r"enum\s+(rmhip_[a-z0-9_]+)\s*\{(.*?)\}\s*;", code, flags=re.S):
        vals, nxt = {}, 0
        for item in m.group(2).split(","):
            item = item.strip()
            if not item:
                continue
            if "=" in item:
                k, v = [x.strip() for x in item.split("=")]
                nxt = int(v)
            else:
                k = item
            vals[k] = nxt
            nxt += 1
        enums[m.group(1)] = vals
    structs = {}
    for m in re.finditer(r"typedef\s+struct\s+(rmhip_[a-z0-9_]+)\s*\{(.*?)\}\s*(rmhip_[a-z0-9_]+)\s*;", code, flags=re.S):
        fields = []
        for decl in m.group(2).split(";"):
            decl = " ".join(decl.split())
            if not decl:
                continue
            fm = re.match(r"((?:unsigned |long )*\w+)\s+(.*)$", decl)  # `double alpha, beta` / `char name[128]`
            ty, names = fm.group(1), [n.strip() for n in fm.group(2).split(",")]
            for n in names:
                am = re.match(r"(\w+)\[(\d+)\]$", n)
                fields.append((ty, am.group(1), int(am.group(2))) if am else (ty, n, None))
        structs[m.group(3)] = fields
    funcs = []
    for m in re.finditer(r"^RMHIP_API\s+(.*?)\b(rmhip_[a-z0-9_]+)\s*\((.*?)\)\s*;", code, flags=re.S | re.M):
        ret = " ".join(m.group(1).split())
        args = []
        raw = " ".join(m.group(3).split())
        if raw != "void":
            for a in raw.split(","):
                a = a.strip()
                am = re.match(r"(.*?)(\w+)\[\d*\]$", a)  # rmhip_buf out5[5]
                if am:
                    args.append((am.group(1).strip() + "*", am.group(2)))
                    continue
                am = re.match(r"(.*?[\s\*])(\w+)$", a)
                args.append((am.group(1).replace(" *", "*").strip(), am.group(2)))
        funcs.append((m.group(2), ret, args))
    return serves, defines, enums, structs, funcs


# ---- ctypes ------------------------------------------------------------------------------------------------------------
PY_SCALAR = {"int": "C.c_int", "unsigned": "C.c_uint", "uint32_t": "C.c_uint32", "uint64_t": "C.c_uint64", "rmhip_buf": "C.c_uint64",
             "size_t": "C.c_size_t", "double": "C.c_double", "long long": "C.c_longlong", "unsigned long long": "C.c_ulonglong", "char": "C.c_char", "unsigned char": "C.c_ubyte"}


def py_type(ty: str, structs) -> str:
    ty = ty.replace("const ", "").strip()
    if ty.endswith("**"):
        return "C.POINTER(C.c_void_p)"
    if ty.endswith("*"):
        base = ty[:-1].strip()
        if base in ("void", "rmhip_ctx"):
            return "C.c_void_p"
        if base == "char":
            return "C.c_char_p"
        if base in structs:
            return f"C.POINTER({camel(base)})"
        return f"C.POINTER({PY_SCALAR[base]})"
    return PY_SCALAR[ty]


def emit_python(serves, defines, enums, structs, funcs) -> str:
    out = ['"""GENERATED by scripts/gen_bindings.py from include/rmhip.h - do not edit.', "",
           "ctypes view of the C ABI of librmhip.so: structures, the SIGNATURES table, the enum / #define constants and the",
           "`@serves` map (C entry point -> AccelProvider methods, crates/runmat-accelerate-api/src/lib.rs:1386-3151).", '"""',
           "import ctypes as C", ""]
    for name, fields in structs.items():
        out.append("")
        out.append(f"class {camel(name)}(C.Structure):")
        out.append(f'    """{name}"""')
        out.append("    _fields_ = [")
        for ty, fname, arr in fields:
            if ty in structs:
                t = camel(ty)
            else:
                t = PY_SCALAR[ty]
            out.append(f'        ("{fname}", {t}{" * %d" % arr if arr else ""}),')
        out.append("    ]")
        out.append("")
    out.append("")
    out.append("SIGNATURES = {")
    for name, ret, args in funcs:
        r = "C.c_int" if ret == "int" else "C.c_char_p" if ret == "const char*" else "C.c_void_p"
        out.append(f'    "{name}": ({r}, [{", ".join(py_type(t, structs) for t, _ in args)}]),')
    out.append("}")
    out.append("")
    out.append("ARG_NAMES = {")
    for name, ret, args in funcs:
        out.append(f'    "{name}": ({", ".join(repr(n) for _, n in args)}{"," if len(args) == 1 else ""}),')
    out.append("}")
    out.append("")
    out.append("ENUMS = {")
    for ename, vals in enums.items():
        out.append(f'    "{ename}": {{{", ".join(f"{k!r}: {v}" for k, v in vals.items())}}},')
    out.append("}")
    out.append("")
    out.append("CONSTANTS = {" + ", ".join(f"{k!r}: {v}" for k, v in defines.items()) + "}")
    out.append("for _e in ENUMS.values():")
    out.append("    CONSTANTS.update(_e)")
    out.append("")
    out.append("SERVES = {")
    for name, _, _ in funcs:
        out.append(f'    "{name}": {tuple(serves.get(name, []))!r},')
    out.append("}")
    out.append("")
    return "\n".join(out)


# ---- Rust --------------------------------------------------------------------------------------------------------------
RS_SCALAR = {"int": "c_int", "unsigned": "c_uint", "uint32_t": "u32", "uint64_t": "u64", "rmhip_buf": "u64", "size_t": "usize",
             "double": "c_double", "long long": "c_longlong", "unsigned long long": "c_ulonglong", "char": "c_char", "unsigned char": "u8"}
RS_KEYWORDS = {"async", "in", "type", "ref", "move", "box", "loop", "match", "fn", "use", "mod", "self"}


def rs_type(ty: str, structs) -> str:
    const = "const " in ty
    ty = ty.replace("const ", "").strip()
    if ty.endswith("**"):
        return "*mut *mut RmhipCtx"
    if ty.endswith("*"):
        base = ty[:-1].strip()
        ptr = "*const " if const else "*mut "
        if base == "rmhip_ctx":
            return "*mut RmhipCtx"
        if base == "void":
            return ptr + "c_void"
        if base in structs:
            return ptr + "Rmhip" + camel(base)
        return ptr + RS_SCALAR[base]
    return RS_SCALAR[ty]


def emit_rust(serves, defines, enums, structs, funcs) -> str:
    out = ["// GENERATED by scripts/gen_bindings.py from include/rmhip.h - do not edit.",
           "// The raw FFI surface of librmhip.so: `#[repr(C)]` structs, constants and the `extern \"C\"` block.  shim/hip_provider.rs",
           "// (`impl AccelProvider for HipProvider`) is the hand-written half and `include!`s this file.",
           "#![allow(non_upper_case_globals, dead_code)]",
           "use std::ffi::{c_char, c_double, c_int, c_longlong, c_uint, c_ulonglong, c_void};", "",
           "#[repr(C)]", "pub struct RmhipCtx {", "    _private: [u8; 0],", "}", ""]
    for name, fields in structs.items():
        out.append(f"/// `{name}`")
        out.append("#[repr(C)]")
        out.append("#[derive(Clone, Copy)]")
        out.append(f"pub struct Rmhip{camel(name)} {{")
        for ty, fname, arr in fields:
            t = ("Rmhip" + camel(ty)) if ty in structs else RS_SCALAR[ty]
            out.append(f"    pub {fname}: {'[%s; %d]' % (t, arr) if arr else t},")
        out.append("}")
        out.append("")
    for k, v in defines.items():
        out.append(f"pub const {k}: usize = {v};")
    for ename, vals in enums.items():
        out.append(f"// enum {ename}")
        for k, v in vals.items():
            out.append(f"pub const {k}: c_int = {v};")
    out.append("")
    out.append('#[link(name = "rmhip")]')
    out.append('extern "C" {')
    for name, ret, args in funcs:
        r = "c_int" if ret == "int" else "*const c_char" if ret == "const char*" else "*mut c_void"
        a = ", ".join(f"{(n + '_') if n in RS_KEYWORDS else n}: {rs_type(t, structs)}" for t, n in args)
        tag = serves.get(name)
        if tag:
            out.append(f"    /// serves: {' '.join(tag)}")
        out.append(f"    pub fn {name}({a}) -> {r};")
    out.append("}")
    out.append("")
    return "\n".join(out)


def main() -> int:
    parsed = parse(HEADER.read_text())
    py, rs = emit_python(*parsed), emit_rust(*parsed)
    if "--check" in sys.argv:
        stale = [str(p.relative_to(ROOT)) for p, want in ((PY_OUT, py), (RS_OUT, rs)) if not p.exists() or p.read_text() != want]
        if stale:
            print("stale generated bindings (run scripts/gen_bindings.py):", ", ".join(stale))
            return 1
        return 0
    PY_OUT.write_text(py)
    RS_OUT.write_text(rs)
    print(f"wrote {PY_OUT.relative_to(ROOT)} ({len(parsed[4])} functions, {len(parsed[3])} structs) and {RS_OUT.relative_to(ROOT)}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
