"""A small parser for the project's C headers (include/*.h, csrc/host/rbq_build.h), shared by test_rust_shim.py (the Rust
side of the boundary), test_abi_prototypes.py (the ctypes side) and the host tests that list a header's entry points.  Every
function takes the header's text.  It reads what these headers use: /* */ comments, `typedef struct [tag] { ... } name;`,
function-pointer typedefs, plain prototypes, integer #defines.

A type is canonical: a scalar name of C_SCALARS (Rust spelling, as integration/gpu_ivf.rs writes it), or nested
('ptr', 'const' | 'mut', inner) around one.

  strip_c_comments  the text without comments
  c_type            'const float*' -> ('ptr', 'const', 'f32')
  c_functions       {name: (return type | None, [(parameter name, type)])} of every prototype
  c_fn_typedefs     the same for `typedef int (*rbq_write_fn)(...)`
  c_structs         {canonical struct name: [(field name, type)]}
  c_defines         {name: int} of the #defines whose value is a decimal integer
"""
import re

C_SCALARS = {"uint8_t": "u8", "uint16_t": "u16", "uint32_t": "u32", "uint64_t": "u64", "int": "c_int", "size_t": "usize",
             "float": "f32", "double": "f64", "void": "c_void", "char": "c_char",
             # opaque handles
             "rbq_index": "RbqIndex", "rbq_builder": "RbqBuilder", "rbq_bf_index": "RbqBfIndex", "rbq_hclustered": "RbqHclustered",
             "rbq_built": "RbqBuilt", "rbq_bf_built": "RbqBfBuilt",
             # data-contract structs
             "rbq_header": "RbqHeader", "rbq_list_view": "RbqListView", "rbq_diag": "RbqDiag", "rbq_bf_view": "RbqBfView",
             "rbq_mstg_config": "RbqMstgConfig",
             # function-pointer typedefs (passed by value)
             "rbq_write_fn": "RbqWriteFn", "rbq_read_fn": "RbqReadFn"}


def strip_c_comments(s):
    return re.sub(r"/\*.*?\*/", " ", s, flags=re.S)


def c_type(tokens):
    """canonical form of a C type: nested ('ptr', 'const'|'mut', inner) around a scalar name"""
    toks = [t for t in re.findall(r"\w+|\*", tokens)]
    # leading type (with optional const either side), then a chain of '*' each optionally followed by const
    const = False
    base = None
    i = 0
    while i < len(toks) and toks[i] != "*":
        if toks[i] == "const":
            const = True
        elif toks[i] in ("struct", "unsigned", "signed"):
            pass
        else:
            base = toks[i]
        i += 1
    assert base in C_SCALARS, (tokens, base)
    t = C_SCALARS[base]
    while i < len(toks):
        assert toks[i] == "*", tokens
        t = ("ptr", "const" if const else "mut", t)
        const = False
        i += 1
        if i < len(toks) and toks[i] == "const":
            const = True
            i += 1
    return t


def split_args(s):
    return [a.strip() for a in s.split(",") if a.strip()]


def _params(args):
    params = []
    if args and args != "void":
        for a in split_args(args):
            mm = re.match(r"(.*?)(\w+)$", a.strip())
            params.append((mm.group(2), c_type(mm.group(1))))
    return params


def c_functions(text):
    src = strip_c_comments(text)
    out = {}
    for m in re.finditer(r"([\w\s\*]+?)\b(rbq_\w+)\s*\(([^;{}]*?)\)\s*;", src):
        ret, name, args = m.group(1).strip(), m.group(2), m.group(3).strip()
        if "typedef" in ret:
            continue
        out[name] = (None if ret == "void" else c_type(ret), _params(args))
    return out


def c_fn_typedefs(text):
    out = {}
    for m in re.finditer(r"typedef\s+([\w\s\*]+?)\(\s*\*\s*(rbq_\w+)\s*\)\s*\(([^;{}]*?)\)\s*;", strip_c_comments(text)):
        ret = m.group(1).strip()
        out[m.group(2)] = (None if ret == "void" else c_type(ret), _params(m.group(3).strip()))
    return out


def c_structs(text):
    src = strip_c_comments(text)
    out = {}
    for m in re.finditer(r"typedef\s+struct\s*\w*\s*\{(.*?)\}\s*(rbq_\w+)\s*;", src, flags=re.S):
        fields = []
        for decl in m.group(1).split(";"):
            decl = decl.strip()
            if not decl:
                continue
            mm = re.match(r"(.*?)(\w+)$", decl)
            fields.append((mm.group(2), c_type(mm.group(1))))
        out[C_SCALARS[m.group(2)]] = fields
    return out


def c_defines(text):
    return {k: int(v) for k, v in re.findall(r"^[ \t]*#define[ \t]+(\w+)[ \t]+(\d+)\b", strip_c_comments(text), flags=re.M)}
