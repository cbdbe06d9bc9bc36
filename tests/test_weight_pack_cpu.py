"""CPU tests of the weight packer and the arena cache's plain parts: the host packer (me_op_weight_pack_host: the loops that
moved out of load_weight into csrc/weight_pack.h) against the numpy / torch restatement of tests/weight_pack_cases.py; the
host build of the same header, driven lane by lane the way the kernels run it (tests/weight_pack_host.cpp), plain and under
the address and undefined-behaviour sanitizers, against the host packer byte for byte; the cache header's reader and
writer on every damaged and stale form; the cache file's name; null contexts on every new entry."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import weight_pack_cases as W  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SOURCE = os.path.join(ROOT, "tests", "weight_pack_host.cpp")
HEADER = os.path.join(ROOT, "matrix-eyes_amd", "csrc", "weight_pack.h")
SRC_DTYPES = [W.W_F16, W.W_BF16, W.W_F32, W.W_F64]


def _build(exe, *flags):
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", *flags, "-o", exe, SOURCE], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return exe


@pytest.fixture(scope="module", params=[[], ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]], ids=["plain", "asan_ubsan"])
def twin(request, tmp_path_factory):
    return _build(str(tmp_path_factory.mktemp("weight_pack") / "weight_pack_host"), *request.param)


def test_the_shared_header_is_plain_text():
    text = open(HEADER).read()
    assert "hip_runtime" not in text and "hipLaunch" not in text and "__global__" not in text
    for name in ("float_to_half", "float_to_bf16", "src_index", "pack_host", "conv_tile_load", "convt_tile_store",
                 "arena_header_check", "ME_ARENA_FORMAT", "checksum_term"):
        assert name in text, name


def _host_pack(lib, ctx_dtype, kind, dims, dup, src, src_dtype):
    out = np.full(W.dst_elems(kind, dims, dup), 0xAAAA if W.dst_dtype(kind) == np.uint16 else 0xAAAAAAAA, dtype=W.dst_dtype(kind))
    cdims = (C.c_int64 * len(dims))(*dims)
    rc = lib.me_op_weight_pack_host(W.CTX_DTYPES[ctx_dtype], kind, dup, cdims, len(dims), C.c_void_p(src.ctypes.data), src_dtype,
                                    C.c_void_p(out.ctypes.data))
    assert rc == 0, rc
    return out


@pytest.mark.parametrize("ctx_dtype", ["f16", "bf16"])
@pytest.mark.parametrize("src_dtype", SRC_DTYPES, ids=[W.SRC_NAMES[d] for d in SRC_DTYPES])
@pytest.mark.parametrize("case", W.CASES, ids=W.CASE_IDS)
def test_host_packer_matches_the_restatement(lib, case, src_dtype, ctx_dtype):
    _, kind, dims, dup = case
    src = W.source(dims, src_dtype, seed=len(dims) * 100 + src_dtype)
    W.check(_host_pack(lib, ctx_dtype, kind, dims, dup, src, src_dtype), kind, dims, dup, src, src_dtype, ctx_dtype)


def test_the_double_rounding_of_f64_is_the_contract(lib):
    """an f64 value just above an f16 tie: rounded directly it goes up, through f32 it lands on the tie and goes to even"""
    v = np.array([1 + 2.0 ** -11 + 2.0 ** -30, 65520.0 - 2.0 ** -20], dtype=np.float64)
    with np.errstate(over="ignore"):
        direct = v.astype(np.float16).view(np.uint16)
        through = v.astype(np.float32).astype(np.float16).view(np.uint16)
    assert list(direct) == [0x3C01, 0x7BFF] and list(through) == [0x3C00, 0x7C00]
    got = _host_pack(lib, "f16", W.K_MAT_16, (1, 2), 0, v, W.W_F64)
    assert list(got) == list(through)


def test_host_packer_rejects_what_does_not_fit(lib):
    src = np.zeros(64, np.float32)
    out = np.zeros(256, np.uint16)
    def call(dtype, kind, dims, s=src, o=out, sd=W.W_F32):
        cd = (C.c_int64 * len(dims))(*dims)
        return lib.me_op_weight_pack_host(dtype, kind, 0, cd, len(dims), C.c_void_p(s.ctypes.data) if s is not None else None, sd,
                                          C.c_void_p(o.ctypes.data) if o is not None else None)
    assert call(0, W.K_MAT_16, (2, 3)) == 0
    assert call(0, W.K_MAT_16, (2, 3), s=None) == -1 and call(0, W.K_MAT_16, (2, 3), o=None) == -1
    assert call(2, W.K_MAT_16, (2, 3)) == -2 and call(0, W.K_MAT_16, (2, 3), sd=4) == -2
    assert call(0, W.K_CONVT_16, (2, 3, 3, 3)) == -3         # a ConvTranspose kernel is 2 x 2
    assert call(0, W.K_CONV_16, (2, 3)) == -3 and call(0, W.K_CONVK_F32, (2, 3, 1, 1)) == -3
    assert call(0, W.K_CONV_16, (1, 1, 9, 9)) == -3          # more taps than the kernel's tile holds
    assert call(0, 7, (2, 3)) == -3 and call(0, W.K_MAT_16, (2, 0)) == -3


@pytest.mark.parametrize("ctx_dtype", ["f16", "bf16"])
@pytest.mark.parametrize("case", W.CASES, ids=W.CASE_IDS)
def test_lane_by_lane_twin_writes_the_host_packers_bytes(twin, tmp_path, case, ctx_dtype):
    _, kind, dims, dup = case
    for src_dtype in SRC_DTYPES:
        src = W.source(dims, src_dtype, seed=7 + src_dtype)
        paths = [str(tmp_path / n) for n in ("src.bin", "host.bin", "lanes.bin")]
        src.tofile(paths[0])
        r = subprocess.run([twin, "pack", str(W.CTX_DTYPES[ctx_dtype]), str(kind), str(dup), str(src_dtype), str(len(dims)),
                            *map(str, dims), *paths], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        host, lanes = (np.fromfile(p, dtype=W.dst_dtype(kind)) for p in paths[1:])
        assert np.array_equal(host, lanes), (W.SRC_NAMES[src_dtype], np.flatnonzero(host != lanes)[:5])
        W.check(lanes, kind, dims, dup, src, src_dtype, ctx_dtype)


def test_cache_header_round_trip_and_every_damaged_form(twin):
    r = subprocess.run([twin, "header"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = dict(line.split(": ", 1) for line in r.stdout.strip().splitlines())
    assert lines["round trip"].endswith("(0)") and lines["checkpoint absent"].endswith("(0)")
    assert lines["another format constant"].endswith("(1)") and lines["another size"].endswith("(2)") and lines["another mtime"].endswith("(2)")
    for damaged in ("short header", "truncated payload", "trailing bytes", "wrong magic", "another header size", "another layout hash",
                    "another arena size", "another split mask", "another dtype", "another configuration"):
        assert int(lines[damaged].rsplit("(", 1)[1].rstrip(")")) >= 10, damaged
    assert lines["checksum"] == "ok"


@pytest.mark.parametrize("checkpoint,want", [
    ("checkpoints/depth_pro.pt", "checkpoints/depth_pro-f16-00000000deadbeef.mearena"),
    ("depth_pro.pt", "depth_pro-f16-00000000deadbeef.mearena"),
    ("/a.b/model", "/a.b/model-f16-00000000deadbeef.mearena"),
    ("dir/.hidden", "dir/.hidden-f16-00000000deadbeef.mearena"),
    ("x.tar.pt", "x.tar-f16-00000000deadbeef.mearena"),
])
def test_cache_file_name(twin, checkpoint, want):
    r = subprocess.run([twin, "path", checkpoint, "f16", "deadbeef"], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip() == want, r.stdout + r.stderr


def test_new_entries_reject_a_null_context(lib):
    buf = C.create_string_buffer(64)
    info, ms, where = (C.c_int64 * 4)(), (C.c_double * 5)(), C.c_int32()
    dims = (C.c_int64 * 2)(2, 3)
    assert lib.me_ctx_set_weight_packer(None, 1) == 1
    assert lib.me_save_weight_arena(None, b"x.mearena", None) == 1
    assert lib.me_load_weight_arena(None, b"x.mearena", None) == 1
    assert lib.me_weight_cache_path(None, b"x.pt", buf, 64) == -1
    assert lib.me_load_checkpoint_cached(None, b"x.pt", 1, C.byref(where)) == 1
    assert lib.me_last_weight_load(None, info, ms) == 1
    assert lib.me_op_weight_pack(None, 1, 0, dims, 2, buf, 0, buf) == 1
    assert not os.path.exists("x.mearena")
