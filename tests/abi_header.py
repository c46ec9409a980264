"""include/roft_engine.h as data, for the tests: the comment-stripped text, the function prototypes, the struct typedefs and the
integer defines.  Two regular expressions over a header that is plain C declarations; nothing here knows the binding."""
import collections
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INCLUDE = os.path.join(ROOT, "include")
HEADER = os.path.join(INCLUDE, "roft_engine.h")

# a C type as the binding has to see it: the base type without qualifiers, and how many pointer / array levels sit on it
CType = collections.namedtuple("CType", "base depth")
Prototype = collections.namedtuple("Prototype", "name ret params")   # params: [(parameter name, CType)]
Struct = collections.namedtuple("Struct", "name fields")             # fields: names in declaration order

_cache = {}


def code():
    """the header without its comments (each replaced by a blank, so that no two tokens join)"""
    if "code" not in _cache:
        _cache["code"] = re.sub(r"/\*.*?\*/", " ", open(HEADER).read(), flags=re.S)
    return _cache["code"]


def _ctype(decl):
    """'const double x[6]' -> ('x', CType('double', 1)); 'const char*' (a return type) -> (None, CType('char', 1))"""
    depth = decl.count("*") + decl.count("[")
    words = re.sub(r"\[[^\]]*\]|\*|\bconst\b", " ", decl).split()
    name = None
    if len(words) > 1 and words[-1] not in ("int", "long", "char", "void", "float", "double"):
        name = words.pop()
    return name, CType(" ".join(words), depth)


def prototypes():
    """every function the header declares, in its order"""
    text = re.sub(r"typedef\s+struct\s*\{[^{}]*\}\s*\w+\s*;", ";", code())   # (struct bodies hold no prototypes)
    text = re.sub(r"^[ \t]*#.*$", ";", text, flags=re.M)                      # (nor do preprocessor lines)
    out = []
    for statement in re.split(r"[;{}]", text):
        m = re.fullmatch(r"\s*([\w\s\*]+?)\b(roft_\w+)\s*\(([^()]*)\)\s*", statement)
        if m:
            ret, name, params = m.groups()
            params = [] if params.strip() == "void" else [_ctype(p) for p in params.split(",")]
            out.append(Prototype(name, _ctype(ret)[1], params))
    return out


def structs():
    """every `typedef struct { ... } roft_x;` of the header, in its order, with the names of its fields"""
    out = []
    for body, name in re.findall(r"typedef\s+struct\s*\{([^{}]*)\}\s*(roft_\w+)\s*;", code()):
        fields = []
        for decl in filter(None, (d.strip() for d in body.split(";"))):
            first, *more = decl.split(",")          # 'int cols, rows' / 'double a[3], b[3]': the type stands once
            fields.append(_ctype(first)[0])
            fields += [re.sub(r"\[[^\]]*\]|\*", "", m).strip() for m in more]
        out.append(Struct(name, fields))
    return out


def opaque_handles():
    """the types declared as `typedef struct roft_x roft_x;`: passed around as pointers only"""
    return re.findall(r"typedef\s+struct\s+(roft_\w+)\s+\1\s*;", code())


def defines():
    """({ROFT_X: int} of every define whose value is an integer, the names of all other ROFT_ defines)"""
    values, others = {}, []
    for name, value in re.findall(r"^[ \t]*#[ \t]*define[ \t]+(ROFT_\w+)[ \t]*(.*?)[ \t]*$", code(), flags=re.M):
        m = re.fullmatch(r"\(?\s*(-?\d+)\s*\)?", value)
        if m:
            values[name] = int(m.group(1))
        else:
            others.append(name)
    return values, others


def layouts(tmp_path):
    """{struct: (sizeof, {field: (offsetof, sizeof)})} as gcc lays the header's structs out: one generated program for all of them"""
    lines = ["#include <stdio.h>", "#include <stddef.h>", '#include "roft_engine.h"', "int main(void) {"]
    for s in structs():
        lines.append('  printf("%s %%zu\\n", sizeof(%s));' % (s.name, s.name))
        lines += ['  printf("%s.%s %%zu %%zu\\n", offsetof(%s, %s), sizeof(((%s*)0)->%s));' % (s.name, f, s.name, f, s.name, f) for f in s.fields]
    lines += ["  return 0;", "}"]
    src, exe = os.path.join(str(tmp_path), "layouts.c"), os.path.join(str(tmp_path), "layouts")
    open(src, "w").write("\n".join(lines) + "\n")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", INCLUDE, src, "-o", exe])
    out = {}
    for line in subprocess.check_output([exe]).decode().splitlines():
        key, *numbers = line.split()
        if "." in key:
            struct, field = key.split(".")
            out[struct][1][field] = tuple(int(n) for n in numbers)
        else:
            out[key] = (int(numbers[0]), {})
    return out
