"""One way to compile a HIP-free model of the library's host code with g++: as a program of its own, or as a shared library
the test loads with ctypes.  A test passes the options it wants; what is the same everywhere - finding the compiler, skipping
without it, reporting a failed compile - is here.  Sanitizers are for programs with their own main: library() takes no such
option."""
import os
import shutil
import subprocess

import pytest

# the sanitizers of a model program (a test that wants symbolised reports adds "-g")
SANITIZE = ("-fsanitize=address,undefined", "-fno-omit-frame-pointer", "-fno-sanitize-recover=undefined")


def gxx():
    """The compiler, or a skip.  (tools/leaf_cull_potential.py builds its model through this module too, and
    tools/node_visit_depths.py imports it with the cases: both need pytest installed, and without g++ the former ends with
    pytest's Skipped exception, which names the reason.)"""
    found = shutil.which("g++")
    if not found:
        pytest.skip("g++ not installed")
    return found


def sanitizer_runtimes_or_skip():
    """Skips where g++ could not link a program built with SANITIZE."""
    found = [subprocess.run([gxx(), ask], capture_output=True, text=True).stdout.strip()
             for ask in ("-print-file-name=libasan.so", "-print-file-name=libubsan.so")]
    if not all(os.path.isabs(p) and os.path.exists(p) for p in found):
        pytest.skip("libasan / libubsan not installed")


def _compile(sources, folder, name, flags, includes):
    out = os.path.join(str(folder), name)
    cmd = [gxx(), "-std=c++17", *flags, *("-I" + str(p) for p in includes), *map(str, sources), "-o", out]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    return out


def _flags(opt, werror, fp_strict):
    """opt: what follows -std, "-O1" or several flags; werror: True -Wall -Wextra -Werror, False -Wall, None no warnings;
    fp_strict: no contraction into FMA, as the library is built (the numerics contract)"""
    warnings = {True: ["-Wall", "-Wextra", "-Werror"], False: ["-Wall"], None: []}[werror]
    return ([opt] if isinstance(opt, str) else list(opt)), warnings + (["-ffp-contract=off", "-fno-fast-math"] if fp_strict else [])


def program(sources, folder, name, *, opt="-O1", werror=True, fp_strict=False, sanitize=(), includes=(), extra=()):
    """-> the path of the executable folder/name.  Arguments in this order: opt, warnings, fp_strict, sanitize, extra, includes."""
    first, rest = _flags(opt, werror, fp_strict)
    return _compile(sources, folder, name, [*first, *rest, *sanitize, *extra], includes)


def library(sources, folder, name, *, opt="-O2", werror=False, fp_strict=False, includes=(), extra=()):
    """-> the path of the shared library folder/name, to be loaded with ctypes; its argtypes stay with the test that loads it."""
    first, rest = _flags(opt, werror, fp_strict)
    return _compile(sources, folder, name, [*first, "-fPIC", "-shared", *rest, *extra], includes)
