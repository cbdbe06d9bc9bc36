"""The tile choice (csrc/tile_choice.h) on the host: g++ alone compiles the header -- it includes nothing of HIP and never asks the
environment -- into tests/tile_choice_host.cpp, once plainly and once with the address and undefined-behaviour sanitizers, and both
programs must give, for every case of tests/tile_choice_cases.py, the answer the rules gave where they stood before the header
existed (tests/golden/tile_choice_table.txt: pick_config, gemm_launch's halo promotions, K < 128 demotion and segment check, the
dispatch arms, gemm_all / resid_all with launch_with_short_tail and tall_tile_wins, maybe_split_k, fp8_tall_wins), and for the worked
examples of the rules' comments the answers the comments state.  No GPU test reads a decision; this table is what does."""
import os
import subprocess

import pytest

import tile_choice_cases as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module", params=[["-O2"], ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]],
                ids=["plain", "asan_ubsan"])
def answers(request, tmp_path_factory):
    """case -> the program's answer, for CASES and the anchors"""
    exe = str(tmp_path_factory.mktemp("tile_choice") / "tile_choice_host")
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", *request.param, "-o", exe,
                        os.path.join(ROOT, "tests", "tile_choice_host.cpp")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    lines = T.CASES + [c for c, _ in T.ANCHORS]
    r = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True)
    assert r.returncode == 0 and r.stderr == "", (r.returncode, r.stderr)
    out = r.stdout.splitlines()
    assert len(out) == len(lines)
    return dict(zip(lines, out))


def test_table_covers_the_case_list():
    """the stored answers are for exactly this case list (its digest is stored with them): neither can change alone"""
    digest, want = T.table()
    assert digest == T.case_list_digest() and len(want) == len(T.CASES)


def test_decisions_are_the_recorded_ones(answers):
    _, want = T.table()
    bad = [(c, w, answers[c]) for c, w in zip(T.CASES, want) if answers[c] != w]
    assert not bad, (len(bad), bad[:10])


def test_worked_examples_of_the_comments(answers):
    bad = [(c, want, answers[c]) for c, want in T.ANCHORS if answers[c] != want]
    assert not bad, bad


def test_config_table_matches_the_dispatch_arms(answers):
    """name, rows, columns, segment alignment, two-slab, admitted pairs and epilogue modes of each id; ADMITS / TWO_SLAB of the case
    module (what tests/test_gpu_ops.py expects of the me_op_* entries) say the same"""
    for i in range(T.CFG_COUNT):
        name, rows, cols, align, two_slab, admits, cf = answers["n %d" % i].split()
        assert int(admits, 16) == sum(1 << (a * 8 + e) for a, e in T.ADMITS[i]), (i, admits)
        assert (int(two_slab) == 1) == (i in T.TWO_SLAB), (i, two_slab)
        assert (int(cf) == 1) == (i != T.CFG_PP352), (i, cf)       # the tap-bias mode: every id that admits a 3x3 convolution has it
        assert name.startswith("%sx%s" % (rows, cols)) or (i in T.HALO_IDS and int(rows) == 16 * T.HALO_IDS[i][0] and
                                                           int(cols) == T.HALO_IDS[i][1]), (i, name, rows, cols)
    assert all(T.ADMITS[i] == {(T.A_CONV, T.EPI_STORE)} for i in T.HALO_IDS)


def test_header_has_no_hip():
    """g++ above is the proof; this names the reason should someone add an include -- or a look at the environment."""
    text = open(os.path.join(ROOT, "matrix-eyes_amd", "csrc", "tile_choice.h")).read()
    includes = [ln.split()[1] for ln in text.splitlines() if ln.startswith("#include")]
    assert includes == ["<stdint.h>"], includes
    assert "getenv(" not in text
