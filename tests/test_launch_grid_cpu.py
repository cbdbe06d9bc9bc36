"""The grid arithmetic of the persistent kernels (csrc/launch_grid.h) on the host: g++ alone compiles the header -- it includes
nothing of HIP -- into tests/launch_grid_host.cpp, once plainly and once with the address and undefined-behaviour sanitizers, and
both programs must give the values below.  They are the formulas the GEMM, convolution and attention launchers each carried
before the header existed, evaluated by hand for a 256-CU device: occupancy x CUs (or the CUs a masked stream may use) in whole
XCD rounds of 8, then min(tiles, resident), the fused LayerNorm's whole rounds, ME_GEMM_GRID_LIMIT and GemmParams::grid_cap.
This table is also all that covers the CU-mask path: no GPU test creates a stream with a CU mask."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (per_cu, cus, cu_granted) -> resident workgroups
RESIDENT = [
    ((1, 256, 0), 256),
    ((2, 256, 0), 512),
    ((0, 256, 0), 256),      # an occupancy below 1 counts as 1
    ((1, 256, 100), 96),     # a CU mask: 100 CUs, whole rounds of 8
    ((1, 256, 300), 256),    # a grant beyond the device changes nothing
    ((1, 4, 0), 8),          # never below one round
    ((1, 0, 0), 8),
]

NO_FIT = -1
# (ntiles, resident, unit, limit, cap) -> grid
GRID = [
    ((340, 256, 0, 0, 0), 256),
    ((40, 256, 0, 0, 0), 40),          # fewer tiles than resident workgroups: not rounded
    ((256, 256, 32, 0, 0), 256),
    ((256, 96, 32, 0, 0), 96),
    ((256, 104, 32, 0, 0), 96),        # whole LayerNorm rounds
    ((256, 24, 32, 0, 0), NO_FIT),     # a round that is not resident at once would wait for ever
    ((8, 256, 8, 0, 0), 8),
    ((256, 256, 32, 8, 0), 8),         # the forced-time-out test's setting: the limit splits a round
    ((256, 256, 32, 100, 0), 96),
    ((256, 256, 32, 7, 0), 256),       # a limit below 8 is none
    ((340, 256, 0, 0, 128), 128),
    ((340, 256, 0, 0, 130), 128),
    ((256, 256, 32, 0, 128), 256),     # a LayerNorm round ignores the cap
    ((340, 256, 0, 200, 128), 128),
    ((340, 256, 0, 0, 4), 256),        # a cap below 8 is none
]


@pytest.fixture(scope="module", params=[["-O2"], ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]],
                ids=["plain", "asan_ubsan"])
def results(request, tmp_path_factory):
    """The program's answers to both tables, in order."""
    exe = str(tmp_path_factory.mktemp("launch_grid") / "launch_grid_host")
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", *request.param, "-o", exe,
                        os.path.join(ROOT, "tests", "launch_grid_host.cpp")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    lines = ["r %d %d %d" % args for args, _ in RESIDENT] + ["g %d %d %d %d %d" % args for args, _ in GRID]
    r = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True)
    assert r.returncode == 0 and r.stderr == "", (r.returncode, r.stderr)
    out = [int(v) for v in r.stdout.split()]
    assert len(out) == len(lines)
    return out


def test_resident_workgroups(results):
    got = results[:len(RESIDENT)]
    assert got == [want for _, want in RESIDENT], list(zip(RESIDENT, got))


def test_persistent_grid(results):
    got = results[len(RESIDENT):]
    assert got == [want for _, want in GRID], list(zip(GRID, got))


def test_header_has_no_hip():
    """g++ above is the proof; this names the reason should someone add an include."""
    text = open(os.path.join(ROOT, "matrix-eyes_amd", "csrc", "launch_grid.h")).read()
    includes = [ln.split()[1] for ln in text.splitlines() if ln.startswith("#include")]
    assert includes == ["<stdint.h>"], includes
