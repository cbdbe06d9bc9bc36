"""Launch admission (csrc/admission.h) on the host: g++ alone compiles the header and the descriptors it judges (csrc/gemm_params.h)
-- neither includes anything of HIP or of the context, neither asks the environment -- into tests/admission_host.cpp, once plainly
and once with the address and undefined-behaviour sanitizers, and both programs must give, for every case of
tests/admission_cases.py, the code and the message the checks gave where they stood before the header existed
(tests/golden/admission_table.txt: gemm_launch, gemm_fp8_launch, attention_launch and the me_op_* entries of api.hip).  The GPU
tests show that a refused call launches nothing; this table is what says WHICH calls are refused, and with what words."""
import os
import subprocess

import pytest

import admission_cases as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "matrix-eyes_amd", "csrc")


@pytest.fixture(scope="module", params=[["-O2"], ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]],
                ids=["plain", "asan_ubsan"])
def answers(request, tmp_path_factory):
    """the program's answers, in the order of CASES"""
    exe = str(tmp_path_factory.mktemp("admission") / "admission_host")
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", *request.param, "-o", exe,
                        os.path.join(ROOT, "tests", "admission_host.cpp")], capture_output=True, text=True)
    assert r.returncode == 0 and r.stderr == "", r.stderr
    r = subprocess.run([exe], input="\n".join(T.CASES) + "\n", capture_output=True, text=True)
    assert r.returncode == 0 and r.stderr == "", (r.returncode, r.stderr)
    out = r.stdout.splitlines()
    assert len(out) == len(T.CASES)
    return out


def test_table_covers_the_case_list():
    """the stored answers are for exactly this case list (its digest is stored with them): neither can change alone"""
    digest, want = T.table()
    assert digest == T.case_list_digest() and len(want) == len(T.CASES)


def test_refusals_are_the_recorded_ones(answers):
    """every case: admitted where it was admitted, refused with the same code and the same message where it was refused"""
    _, want = T.table()
    bad = [(c, w, a) for c, w, a in zip(T.CASES, want, answers) if a != w]
    assert not bad, (len(bad), bad[:10])


def test_table_has_both_answers_for_every_rule():
    """a table of one answer would hold nothing: every message of the header is in it, and admitted neighbours beside them"""
    _, want = T.table()
    assert sum(w == "0" for w in want) > 100
    refused = [w.split("\t", 1) for w in want if w != "0"]
    assert {c for c, _ in refused} == {"1", "2"}          # ME_ERR_BAD_ARG, ME_ERR_BAD_SHAPE
    import re
    code = "\n".join(ln.split("//")[0] for ln in open(os.path.join(CSRC, "admission.h")).read().splitlines() if not ln.startswith("#"))
    # the literal start of every message in the header, up to its first conversion (a "%s: " prefix is the caller's name)
    heads = {re.sub(r"^%s: ", "", s).split("%")[0] for s in re.findall(r'"((?:[^"\\]|\\.)*)"', code)}
    heads = {h for h in heads if len(h) >= 6}
    assert len(heads) > 60, sorted(heads)
    missing = sorted(h for h in heads if not any(h in msg for _, msg in refused))
    assert not missing, missing


def test_headers_have_no_hip():
    """g++ above is the proof; this names the reason should someone add an include -- or a look at the environment."""
    allowed = {"admission.h": ['"gemm_params.h"'],
               "gemm_params.h": ["<math.h>", "<stdint.h>", '"../../include/matrix_eyes_hip.h"', '"error.h"', '"tile_choice.h"'],
               "error.h": ["<stdint.h>", "<string>"]}
    for name, want in allowed.items():
        text = open(os.path.join(CSRC, name)).read()
        includes = [ln.split()[1] for ln in text.splitlines() if ln.startswith("#include")]
        assert includes == want, (name, includes)
        assert "getenv(" not in text, name
    assert "GemmParams {" not in open(os.path.join(CSRC, "common.h")).read()
