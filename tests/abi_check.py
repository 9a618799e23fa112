"""The hand-written ctypes mirror of a C header, checked against the header in full (tests/test_abi_cpu.py runs it on
upnerf_amd/_lib.py and include/upnerf_hip.h).  Every function takes the ctypes side and the header's path and returns the
disagreements as a list of strings; an empty list means the two agree.  gcc does the reading of C: the header is only searched
for the NAMES of its typedefs, their fields, its prototypes and constants, never parsed for a layout or a parameter list.

A ctypes class `FieldBwdArgs` mirrors the typedef `upnerf_field_bwd_args`: prefix + snake_case of the class name (c_name).

What the prototype check cannot see: a ctypes argument NARROWER than the header's parameter (an int handed to a long long
converts without a warning), and which address a `void*` argument carries."""
import ctypes
import os
import re
import subprocess
import tempfile

PREFIX = "upnerf_"
SCALARS = {ctypes.c_int: "int", ctypes.c_float: "float", ctypes.c_longlong: "long long", ctypes.c_uint64: "uint64_t",
           ctypes.c_int64: "int64_t", ctypes.c_void_p: "void*"}


def header_text(path):
    """The header without comments and without the entry points of the diagnostic build (-DUPNERF_STAMPS), which are not part
    of the shipped library."""
    src = re.sub(r"#ifdef UPNERF_STAMPS.*?#endif", "", open(path).read(), flags=re.S)
    return re.sub(r"/\*.*?\*/|//[^\n]*", "", src, flags=re.S)


def c_name(cls):
    return PREFIX + re.sub(r"(?<!^)(?=[A-Z])", "_", cls.__name__).lower()


def struct_classes(module):
    return [v for v in vars(module).values()
            if isinstance(v, type) and issubclass(v, ctypes.Structure) and v.__module__ == module.__name__]


def typedefs(path):
    """{typedef name: the names of its fields} of every `typedef struct ... { ... } name;` of the header."""
    field = lambda decl: re.search(r"(\w+)\s*(?:\[[^\]]*\]\s*)*$", decl).group(1)
    return {n: [field(d) for decl in body.split(";") if decl.strip() for d in decl.split(",")]
            for body, n in re.findall(r"typedef\s+struct\s*\w*\s*\{([^{}]*)\}\s*(\w+)\s*;", header_text(path))}


def prototypes(path):
    """{name: return type} of the header's entry points."""
    return {n: r for r, n in re.findall(rf"^(int|long long)\s+({PREFIX}\w+)\s*\(", header_text(path), flags=re.M)}


def constants(path):
    """{NAME: value} of every `#define UPNERF_<NAME> <integer>` and every enumerator UPNERF_<NAME> of the header."""
    src = header_text(path)
    out = {n: int(v) for n, v in re.findall(rf"^#define\s+{PREFIX.upper()}(\w+)[ \t]+\(?(-?\d+)\)?[ \t]*$", src, flags=re.M)}
    for body in re.findall(r"\benum\s*\w*\s*\{([^{}]*)\}", src):
        value = -1
        for item in filter(None, (s.strip() for s in body.split(","))):
            name, _, given = (s.strip() for s in item.partition("="))
            value = int(given, 0) if given else value + 1
            out[name[len(PREFIX):]] = value
    return out


def _gcc(path, body, *flags):
    """Compiles `body` behind the header; (None, compiler's error lines) if it does not compile, else (stdout of the program --
    "" under -fsyntax-only --, [])."""
    with tempfile.TemporaryDirectory() as d:
        src, exe = os.path.join(d, "abi.c"), os.path.join(d, "abi")
        with open(src, "w") as f:
            f.write(f'#include <stddef.h>\n#include <stdio.h>\n#include "{os.path.basename(path)}"\n#line 1\n' + body)
        r = subprocess.run(["gcc", "-I", os.path.dirname(os.path.abspath(path)), *flags, src, "-o", exe], capture_output=True, text=True)
        if r.returncode:
            return None, [line for line in r.stderr.splitlines() if " error: " in line]
        return ("" if "-fsyntax-only" in flags else subprocess.run([exe], capture_output=True, text=True, check=True).stdout), []


def check_structs(classes, path):
    """Class <-> typedef one to one under c_name; sizeof of every struct, offsetof and sizeof of every ctypes field; and no field
    of the header left out of its mirror (by name: alignment padding can take a dropped field's place without moving anything)."""
    have, by_name = typedefs(path), {c_name(c): c for c in classes}
    bad = [f"{c.__name__}: the header has no typedef {n}" for n, c in by_name.items() if n not in have]
    bad += [f"{n}: no ctypes class mirrors it" for n in have if n not in by_name]
    pairs = [(n, c) for n, c in by_name.items() if n in have]
    bad += [f"{n}.{f}: not in the mirror {c.__name__}" for n, c in pairs for f in have[n] if not hasattr(c, f)]
    lines = []
    for n, c in pairs:
        lines.append(f'printf("%zu\\n", sizeof({n}));')
        lines += [f'printf("%zu %zu\\n", offsetof({n}, {f}), sizeof((({n}*)0)->{f}));' for f, *_ in c._fields_]
    out, errors = _gcc(path, "int main(void){\n" + "\n".join(lines) + "\nreturn 0;}\n")
    if out is None:  # a ctypes field the C struct lacks (gcc names both)
        return bad + [e.split(" error: ", 1)[1] for e in errors]
    rows = iter(out.split("\n"))
    for n, c in pairs:
        size = int(next(rows))
        if ctypes.sizeof(c) != size:
            bad.append(f"{c.__name__}: sizeof is {ctypes.sizeof(c)}, sizeof({n}) is {size}")
        for f, *_ in c._fields_:
            off, width = map(int, next(rows).split())
            mine = getattr(c, f)
            if (mine.offset, mine.size) != (off, width):
                bad.append(f"{c.__name__}.{f}: at {mine.offset} with {mine.size} bytes, {n}.{f} at {off} with {width}")
    return bad


def _c_type(t):
    """(declaration of a dummy parameter of ctypes type t, the argument made of it); KeyError if t has no C spelling here."""
    if t in SCALARS:
        return SCALARS[t] + " a{}", "a{}"
    if issubclass(t._type_, ctypes.Structure):
        return c_name(t._type_) + " a{}", "&a{}"
    return SCALARS[t._type_] + "* a{}", "a{}"


def check_prototypes(signatures, longlong, path):
    """One typed call per entry of `signatures` ({name: argtypes}), its result assigned to long long for the names in `longlong`
    and to int otherwise, compiled with -Werror -Wconversion; and `longlong` = the prototypes that return long long."""
    protos = prototypes(path)
    wide = {n for n, r in protos.items() if r == "long long"}
    bad = [f"{n}: returns long long in the header, but is bound as returning int" for n in sorted(wide - set(longlong))]
    bad += [f"{n}: bound as returning long long, but the header says {protos.get(n, 'nothing of it')}" for n in sorted(set(longlong) - wide)]
    calls = []  # one function per line: the compiler's line number names the entry point (an undeclared one is an error too)
    for n, argtypes in signatures.items():
        args = [_c_type(t) for t in argtypes]
        params = ", ".join(a[0].format(i) for i, a in enumerate(args)) or "void"
        result = "long long" if n in longlong else "int"
        calls.append((n, f"void call_{n}({params}){{ {result} r = {n}({', '.join(a[1].format(i) for i, a in enumerate(args))}); (void)r; }}"))
    _, errors = _gcc(path, "\n".join(c for _, c in calls) + "\n", "-fsyntax-only", "-Werror", "-Wconversion")
    for e in errors:
        m = re.match(r".*abi\.c:(\d+):\d+: error: (.*)", e)  # (an error inside the header itself is passed on as it is)
        bad.append(f"{calls[int(m.group(1)) - 1][0]}: {m.group(2)}" if m else e)
    return bad


def check_constants(namespace, path, unmirrored):
    """Every integer constant of the header is either in `namespace` under its name without the prefix, with the same value, or
    named in `unmirrored` -- not both, not neither."""
    consts = constants(path)
    bad = [f"{n}: listed as unmirrored, but the header does not define it" for n in unmirrored if n not in consts]
    for n, v in consts.items():
        if n in namespace and n in unmirrored:
            bad.append(f"{n}: listed as unmirrored, but mirrored")
        elif n in namespace and namespace[n] != v:
            bad.append(f"{n}: {namespace[n]} in Python, {PREFIX.upper()}{n} is {v}")
        elif n not in namespace and n not in unmirrored:
            bad.append(f"{n}: {PREFIX.upper()}{n} = {v} has no mirror and is not listed as unmirrored")
    return bad
