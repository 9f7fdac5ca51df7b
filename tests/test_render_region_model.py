"""The rectangle a launch renders (csrc/render_region.h: ptmi_render_region), checked without a GPU.

tests/render_region_model.cpp plays the header's one copy of the slot <-> (pixel, iteration) mapping, of the job hand-out's tile
cover and of check_region - the copy the kernels and the launch code compile.  For images 1 x 1, 8 x 8, 43 x 29 and 64 x 48,
EVERY region of 43 x 29 (411 510 of them, in six shares) and of the two small images, and a seeded sample of those of 64 x 48,
each with n = 1, 3 and 32 iterations per launch:
- slot -> (gx, gy, it) -> slot is the identity, and region_pixel names that pixel in the image;
- the slots of a launch are exactly 0 .. w * h * n - 1 (as many distinct slots as paths, all below that bound);
- the tile cover from the region's origin reaches every pixel of the region once and no pixel outside it.
check_region refuses x + width > W by one, y + height > H by one and the 32-bit wrap (x = 0xFFFFFFFF, width = 2), and accepts
empty regions.  The program is compiled with -Wall -Wextra -Werror, and a second time with the address and undefined-behaviour
sanitizers, which runs a thinner share of the same.  The binding: sizeof(ptmi_region) == 16, both symbols declared, exported
and bound.
"""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import model_build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODEL_SRC = os.path.join(ROOT, "tests", "render_region_model.cpp")
CSRC = os.path.join(ROOT, "opencl_pathtracer_amd", "csrc")
ALL_43x29 = (43 * 44 // 2) * (29 * 30 // 2)
SHARES = 6


def _compile(tmp, name, sanitize=()):
    return model_build.program([MODEL_SRC], tmp, name, opt="-O2", werror=True, sanitize=sanitize, includes=[CSRC])


@pytest.fixture(scope="module")
def model(tmp_path_factory):
    return _compile(tmp_path_factory.mktemp("render_region"), "render_region_model")


def run(exe, *args):
    r = subprocess.run([exe, *map(str, args)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    m = re.fullmatch(r"ok \w+ (\d+)(?: regions (\d+) paths (\d+) tiles)?\n", r.stdout)
    assert m, r.stdout
    return tuple(int(g) for g in m.groups() if g is not None)


@pytest.mark.parametrize("share", range(SHARES))
def test_every_region_of_43x29(model, share):
    regions, paths, tiles = run(model, "every", 43, 29, SHARES, share)
    assert regions == len(range(share, ALL_43x29, SHARES)) and paths > 36 * regions and tiles >= regions


@pytest.mark.parametrize("w, h", [(1, 1), (8, 8)])
def test_every_region_of_the_small_images(model, w, h):
    regions, paths, _ = run(model, "every", w, h, 1, 0)
    assert regions == (w * (w + 1) // 2) * (h * (h + 1) // 2)
    # every region is rendered with n = 1, 3 and 32: 36 paths per pixel of it
    assert paths == 36 * sum(rw * rh * (w - rw + 1) * (h - rh + 1) for rw in range(1, w + 1) for rh in range(1, h + 1))


@pytest.mark.parametrize("w, h", [(64, 48), (43, 29), (8, 8), (1, 1)])
def test_a_seeded_sample_of_regions(model, w, h):
    regions, _, _ = run(model, "sample", w, h, 400, 11)
    assert regions == 401  # (the whole image first)


def test_check_region(model):
    assert run(model, "check")[0] >= 18


def test_the_model_under_the_sanitizers(tmp_path):
    exe = _compile(tmp_path, "render_region_model_san", ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])
    assert run(exe, "every", 43, 29, 32, 5)[0] == len(range(5, ALL_43x29, 32))
    run(exe, "every", 8, 8, 1, 0)
    run(exe, "every", 1, 1, 1, 0)
    run(exe, "sample", 64, 48, 100, 3)
    run(exe, "check")


def test_the_header_needs_no_hip_and_nothing_else_of_the_library(tmp_path):
    """render_region.h alone, by g++: what lets the model above be the kernels' own copy"""
    src = tmp_path / "alone.cpp"
    src.write_text('#include "render_region.h"\nint main() { return ptmi_internal::region_tiles(ptmi_internal::whole_image(43, 29)) == 24u ? 0 : 1; }\n')
    assert subprocess.run([model_build.program([src], tmp_path, "alone", opt=(), werror=True, includes=[CSRC])]).returncode == 0


def test_the_binding():
    from opencl_pathtracer_amd import backend, structs as S
    assert S.REGION.itemsize == 16 and S.REGION.names == ("x", "y", "width", "height")
    r = backend.Backend.region(3, 5, 7, 11)
    assert r.dtype == S.REGION and r.nbytes == 16 and r.view(np.uint32).tolist() == [3, 5, 7, 11]
    header = open(os.path.join(ROOT, "include", "ptmi.h")).read()
    assert re.search(r"typedef struct ptmi_region \{ uint32_t x, y, width, height; \} ptmi_region;", header)
    names = {"ptmi_render_region", "ptmi_read_region"}
    assert names <= set(backend.ABI_SYMBOLS)
    for n in names:
        assert re.search(r"^int " + n + r"\(ptmi_ctx\* ctx, const ptmi_region\* region, ", header, re.M), n
    if not os.path.exists(backend.library_path()):
        pytest.skip("libptmi.so not built")
    lib = backend.load_library()
    for n in names:
        assert getattr(lib, n).argtypes is not None and len(getattr(lib, n).argtypes) == 4, n
    exported = subprocess.run(["nm", "-D", "--defined-only", backend.library_path()], capture_output=True, text=True).stdout
    assert all(re.search(r" T " + n + r"$", exported, re.M) for n in names)


def test_sizeof_ptmi_region_is_16(tmp_path):
    gcc = shutil.which("gcc")
    if gcc is None:
        pytest.skip("gcc not installed")
    src = tmp_path / "size.c"
    src.write_text('#include <stddef.h>\n#include "ptmi.h"\n_Static_assert(sizeof(ptmi_region) == 16 && offsetof(ptmi_region, height) == 12, "ptmi_region");\n'
                   'int main(void) { return 0; }\n')
    subprocess.run([gcc, "-std=c11", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "include"), str(src), "-o", str(tmp_path / "size")], check=True)
