"""CPU test of csrc/orient.h, the store remap both photo decoders' finish kernels share: tests/orient_host.cpp holds it to
the two functions it replaced and to apply_orientation of host/image_io.cpp, for every width and height in 1..9, all
eight orientations and the values 0 and 9."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "matrix-eyes_amd")
SOURCES = [os.path.join(ROOT, "tests", "orient_host.cpp")] + [os.path.join(PKG, "host", name) for name in
                                                            ("image_io.cpp", "png_decoder.cpp", "jpeg_decoder.cpp", "jpeg_encoder.cpp")]


def test_the_shared_header_is_plain():
    text = open(os.path.join(PKG, "csrc", "orient.h")).read()
    assert [line for line in text.splitlines() if line.startswith("#include")] == ["#include <stdint.h>"]
    for name in ("jpeg_recon.h", "png_recon.h"):
        other = open(os.path.join(PKG, "csrc", name)).read()
        assert '#include "orient.h"' in other and "case 7:" not in other, name      # no second copy of the switch


def test_one_remap_equals_both_it_replaced_and_apply_orientation(tmp_path):
    exe = str(tmp_path / "orient_host")
    basis = os.path.join(PKG, "csrc", "jpeg_basis.cpp")
    r = subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-Wextra", "-o", exe, *SOURCES, basis, "-lz"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    checks, failed = int(r.stdout.split()[0]), int(r.stdout.split()[2])
    # 81 shapes x 10 orientations: four comparisons per pixel, one per destination pixel, the size and the picture
    pixels = sum(w * h for w in range(1, 10) for h in range(1, 10))
    assert failed == 0 and checks == 10 * (5 * pixels + 2 * 81), r.stdout
