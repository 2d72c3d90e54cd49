"""Layout of include/kgan_hip.h as a C compiler sees it, for the tests that compare the ctypes mirrors of
kinetic-gan_amd/_native.py with it: ONE generated C program prints sizeof of every struct, offsetof of every field and the
value of every ``#define KG_*``; it is compiled with gcc and run once per test session (cached).

The naming rule has no exception: ``_native._FooArgs`` mirrors ``KgFooArgs`` and carries the header's field names."""
import ctypes
import functools
import os
import re
import subprocess
import tempfile

from kinetic_gan_amd import _native

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "kgan_hip.h")


def _code():
    return re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)


def header_structs():
    """names of the header's struct typedefs"""
    return sorted(set(re.findall(r"\}\s*(Kg\w+)\s*;", _code())))


def header_defines():
    """names of the header's ``#define KG_*`` constants"""
    return sorted(set(re.findall(r"^[ \t]*#[ \t]*define[ \t]+(KG_\w+)[ \t]+\S", _code(), flags=re.M)))


def mirrors():
    """{header name: ctypes class} of every ctypes.Structure subclass defined in _native (``_Foo`` -> ``KgFoo``)"""
    return {"Kg" + n[1:]: t for n, t in vars(_native).items()
            if isinstance(t, type) and issubclass(t, ctypes.Structure) and t.__module__ == _native.__name__}


def mirror_layout(t):
    """{"sizeof": n, field: offset, ...} of a ctypes mirror"""
    return dict({"sizeof": ctypes.sizeof(t)}, **{n: getattr(t, n).offset for n, *_ in t._fields_})


@functools.lru_cache(maxsize=None)
def _compiled(structs):
    """structs: a tuple of (header name, field names); returns the program's output as {key: int}"""
    lines = ["#include <stdio.h>", "#include <stddef.h>", '#include "kgan_hip.h"', "int main(void){"]
    for cname, fields in structs:
        lines.append('printf("%s.sizeof %%zu\\n", sizeof(%s));' % (cname, cname))
        lines += ['printf("%s.%s %%zu\\n", offsetof(%s, %s));' % (cname, f, cname, f) for f in fields]
    lines += ['printf("%s %%lld\\n", (long long)(%s));' % (d, d) for d in header_defines()]
    lines.append("return 0; }")
    with tempfile.TemporaryDirectory() as d:
        c, exe = os.path.join(d, "layout.c"), os.path.join(d, "layout")
        open(c, "w").write("\n".join(lines) + "\n")
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), c, "-o", exe])
        out = subprocess.check_output([exe], text=True)
    return {k: int(v) for k, v in (ln.split() for ln in out.splitlines())}


def _all():
    return _compiled(tuple((cname, tuple(n for n, *_ in t._fields_)) for cname, t in sorted(mirrors().items())))


def header_layout(cname):
    """{"sizeof": n, field: offset, ...} of the header's struct ``cname``, for the fields its mirror names (a field the header
    lacks does not compile: the error names it)"""
    pre = cname + "."
    return {k[len(pre):]: v for k, v in _all().items() if k.startswith(pre)}


def header_constants():
    """{name: value} of every ``#define KG_*`` integer constant, evaluated by the compiler"""
    return {k: v for k, v in _all().items() if "." not in k}


def assert_mirror(cname):
    """the mirror of ``cname`` has the header's size and every field offset; the message names struct and field"""
    want, got = header_layout(cname), mirror_layout(mirrors()[cname])
    bad = {f: (want[f], got[f]) for f in want if want[f] != got[f]}
    assert not bad, "%s: (header, _native) differ at %s" % (cname, bad)
