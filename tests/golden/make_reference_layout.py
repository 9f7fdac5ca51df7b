"""Data fixtures taken from the reference's own files, so that the tests comparing the product with them run without the
reference tree (test_super_sampling.py, test_shim.py).  Made where the tree exists:

    python tests/golden/make_reference_layout.py /path/to/reference

* x2inv_reference.npy           the 1001 floats of Kernel/X2inv.cl, as the reference writes them, rounded to float32
* backend_layout_reference.json offsetof / sizeof of the reference's GlobalVars and scene structs
                                (Controleur/PathTracer_Structs.h), compiled for x86-64 by the ROCm clang++ below
"""
import json
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
CLANGXX = "/opt/rocm/lib/llvm/bin/clang++"
# the fields of PathTracerNS::GlobalVars the shim hands over (the mirror in include/pathtracer_backend.hpp must match)
GLOBALVARS_FIELDS = ["window", "importer", "cameraDirection", "cameraRight", "cameraUp", "cameraPosition", "bvh", "triangulation",
                     "lights", "materiaux", "textures", "texturesData", "bvhSize", "triangulationSize", "lightsSize",
                     "materiauxSize", "texturesSize", "texturesDataSize", "bvhMaxDepth", "sampler", "printLogInfos",
                     "superSampling", "sky", "imageWidth", "imageHeight", "imageSize", "rayMaxDepth", "imageColor", "imageRayNb",
                     "rayDepths", "rayIntersectedBBx", "rayIntersectedTri"]
SCENE_STRUCTS = ["Triangle", "Node", "Material", "Light", "Sky", "Texture"]


def x2inv_table(ref):
    txt = open(os.path.join(ref, "Kernel", "X2inv.cl")).read()
    body = txt[txt.index("{") + 1:txt.rindex("}")]
    return np.array([float(v.strip().rstrip("f")) for v in body.split(",") if v.strip()], np.float32)


def layout(ref):
    lines = ['#include <cstddef>', '#include <climits>', '#include <cstring>', '#include <cstdio>', '#include "PathTracer_Structs.h"',
             'int main() {', '  std::printf("{\\"GlobalVars\\": {\\"sizeof\\": %zu", sizeof(PathTracerNS::GlobalVars));']
    lines += [f'  std::printf(", \\"{f}\\": %zu", offsetof(PathTracerNS::GlobalVars, {f}));' for f in GLOBALVARS_FIELDS]
    lines += ['  std::printf("}, \\"sizeof\\": {");']
    lines += [f'  std::printf("{", " if i else ""}\\"{s}\\": %zu", sizeof(PathTracerNS::{s}));' for i, s in enumerate(SCENE_STRUCTS)]
    lines += ['  std::printf("}}\\n");', '  return 0;', '}']
    with tempfile.TemporaryDirectory() as d:
        src, exe = os.path.join(d, "layout.cpp"), os.path.join(d, "layout")
        open(src, "w").write("\n".join(lines) + "\n")
        subprocess.run([CLANGXX, "-std=c++14", "-fms-extensions", "-I", os.path.join(ref, "Controleur"), src, "-o", exe], check=True)
        return json.loads(subprocess.run([exe], check=True, capture_output=True, text=True).stdout)


def main(ref):
    np.save(os.path.join(HERE, "x2inv_reference.npy"), x2inv_table(ref))
    with open(os.path.join(HERE, "backend_layout_reference.json"), "w") as f:
        json.dump(layout(ref), f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main(sys.argv[1])
