"""What the ABI tests share (test_abi.py and the test_*_model.py of every call family): the symbols include/ptmi.h declares,
the symbols the built library exports, and values of the header as a C compiler sees them.  No product code is involved."""
import os
import re
import subprocess
import tempfile

from opencl_pathtracer_amd import backend

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PROBE = r"""
#include <stddef.h>
#include <stdio.h>
#include "ptmi.h"
#define VALUE(name, v) printf("%%s %%lld\n", name, (long long)(v))
#define SIZE(type) VALUE(#type, sizeof(type))
#define OFFSET(type, field) VALUE(#type "." #field, offsetof(type, field))
int main(void)
{
%s
    return 0;
}
"""


def declared_symbols():
    text = open(os.path.join(ROOT, "include", "ptmi.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(ptmi_[a-z_]+)\s*\(", text)))


def exported_symbols():
    """Every function the built library defines and exports (C++ ones, mangled, included)."""
    out = subprocess.run(["nm", "-D", "--defined-only", backend.library_path()], capture_output=True, text=True, check=True).stdout
    return {l.split()[-1] for l in out.splitlines() if " T " in l}


def header_values(lines_of_C):
    """{name: int} of a C11 program that includes ptmi.h and runs the statements given: VALUE("name", expression), SIZE(type)
    -> "type", OFFSET(type, field) -> "type.field"."""
    with tempfile.TemporaryDirectory() as tmp:
        src, exe = os.path.join(tmp, "probe.c"), os.path.join(tmp, "probe")
        with open(src, "w") as f:
            f.write(PROBE % "\n".join("    " + line for line in lines_of_C))
        subprocess.run(["gcc", "-std=c11", "-I", os.path.join(ROOT, "include"), src, "-o", exe], check=True)
        out = subprocess.run([exe], capture_output=True, text=True, check=True).stdout
    return {k: int(v) for k, v in (line.rsplit(" ", 1) for line in out.splitlines())}
