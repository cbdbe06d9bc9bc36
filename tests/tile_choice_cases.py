"""The case list of tests/test_tile_choice_cpu.py: one line per question to tests/tile_choice_host.cpp (its header has the formats).
A plain module: no test lives here.

Three sources.  (1) The recorded problems of tests/golden/tile_choice_launches.txt -- every GEMM and convolution of the full-size
step and of the sweep configurations as the launchers saw them --, asked as launched, the step's also under each knob flipped, and
turned into the questions the ViT linears, split-K and the fp8 GEMM ask.  (2) For every inequality of every rule a case on each
side of it, and grids across the thresholds.  (3) ANCHORS: the worked examples the comments of the rules state, with the
comments' answers written here by hand.

The answers to (1) and (2) are tests/golden/tile_choice_table.txt: the output of the functions as they stood in gemm.hip,
pipeline.hip, gemm_fp8.hip and gemm_core.h's dispatch before csrc/tile_choice.h existed, cut verbatim into a host program with
stubs and run over this list, stored many to a line beside the digest of the list.  The header is held to that table, not the other
way round.

ADMITS (the (A-mode, epilogue) pairs each id is compiled for) and TWO_SLAB are also what tests/test_gpu_ops.py expects of the
me_op_* entries; they are written out here from the dispatch arms, and the table's `n` rows check the header's against the same."""
import os

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

A_PLAIN, A_CONV = 0, 1
EPI_STORE, EPI_RESID_SCALE, EPI_PATCH_EMBED, EPI_CONVT, EPI_HEAD_FINAL, EPI_HEAD_COMPOSED = 0, 1, 2, 4, 5, 6
(CFG_PP256, CFG_128, CFG_64, CFG_160, CFG_RING64, CFG_PP192, CFG_8PH, CFG_PP96, CFG_RING128, CFG_HALO, CFG_PP352, CFG_HALO12,
 CFG_HALO_N128, CFG_COUNT) = range(14)

_PLAIN_LINEAR = {(A_PLAIN, EPI_STORE), (A_PLAIN, EPI_RESID_SCALE)}
_CONV_STORE = {(A_CONV, EPI_STORE)}
_ANY = _PLAIN_LINEAR | {(A_PLAIN, EPI_PATCH_EMBED), (A_PLAIN, EPI_CONVT)} | _CONV_STORE
ADMITS = {CFG_PP256: _ANY, CFG_128: _ANY, CFG_64: _ANY, CFG_160: _ANY, CFG_RING64: _ANY, CFG_PP192: _ANY, CFG_8PH: _PLAIN_LINEAR,
          CFG_PP96: _PLAIN_LINEAR | _CONV_STORE, CFG_RING128: _PLAIN_LINEAR | _CONV_STORE, CFG_HALO: _CONV_STORE,
          CFG_PP352: _PLAIN_LINEAR, CFG_HALO12: _CONV_STORE, CFG_HALO_N128: _CONV_STORE}
TWO_SLAB = {CFG_PP256, CFG_PP192, CFG_8PH, CFG_PP96, CFG_PP352}    # K < 128 runs on CFG_128 instead
HALO_IDS = {CFG_HALO: (16, 256), CFG_HALO12: (12, 256), CFG_HALO_N128: (16, 128)}   # id -> (tile rows of pixels, channel multiple)


def r(force=-1, M=0, N=0, K=0, seg1=0, seg2=0, am=A_PLAIN, ep=EPI_STORE, KH=0, KW=0, st=0, oH=0, oW=0, Cin=0, tap=0, ln=0,
      dyn=0, halo=1, halo12=1, halo128=1):
    return "r %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d" % (
        force, M, N, K, seg1, seg2, am, ep, KH, KW, st, oH, oW, Cin, tap, ln, dyn, halo, halo12, halo128)


def conv3(force=-1, B=1, H=48, W=48, Cin=64, N=256, ep=EPI_STORE, **kw):
    return r(force, B * H * W, N, 9 * Cin, am=A_CONV, ep=ep, KH=3, KW=3, st=1, oH=H, oW=W, Cin=Cin, **kw)


def v(M, N, K, seg1=0, seg2=0, C=None, resid=0, lnw=0, lnf=0, tall=1, bias="0.95", tail96=1, pp192=0):
    C = (N if resid else K) if C is None else C
    return "v %d %d %d %d %d %d %d %d %d %d %s %d %d" % (M, N, K, seg1, seg2, C, resid, lnw, lnf, tall, bias, tail96, pp192)


def s(rpi, M, N, K, on=1, min_k=4096):
    return "s %d %d %d %d %d %d" % (rpi, M, N, K, on, min_k)


def f(M, N, seg1=0, seg2=0, knob=-1):
    return "f %d %d %d %d %d" % (M, N, seg1, seg2, knob)


def recorded():
    """The problems of tile_choice_launches.txt as (section, kind, [ints]): section 'step' or 'sweep', kind 'r' (16 ints) or 'f' (4)."""
    out, section = [], None
    for ln in open(os.path.join(GOLDEN, "tile_choice_launches.txt")):
        if ln.startswith("# ["):
            section = ln[3:ln.index("]")]
        elif ln.strip() and not ln.startswith("#"):
            for item in ln.split(";"):
                w = item.split()
                out.append((section, w[0], [int(x) for x in w[1:]]))
    return out


# ---- (3) the comments' own examples: (case, answer) ----
ONE_IMAGE = dict(seg1=768, seg2=1536)   # 21760 rows: three ViTs' segments at one image
ANCHORS = [
    # pick_config's comment, M = 20195: qkv / fc1 -> 256x256; proj / fc2 at N = 1024 -> 160x128 (1016 tiles = 2 rounds of 512)
    (r(M=20195, N=3072, K=1024), "ok %d" % CFG_PP256),
    (r(M=20195, N=4096, K=1024), "ok %d" % CFG_PP256),
    (r(M=20195, N=1024, K=1024), "ok %d" % CFG_160),
    (r(M=20195, N=1024, K=4096), "ok %d" % CFG_160),
    # ... the 64x64 tile for the single-window ViTs (M = 577); its fc2 (160 tiles x 64 slabs) on the six-slot ring
    (r(M=577, N=3072, K=1024), "ok %d" % CFG_64),
    (r(M=577, N=1024, K=4096), "ok %d" % CFG_RING64),
    # ... the 256-channel convolutions at 768^2 and 384^2 -> 256x256, which is where the halo tiles take over: 384 x 384 is three
    # full rounds of 12-row tiles instead of 2.25 of 16-row ones
    (conv3(H=768, W=768, Cin=256, halo=0), "ok %d" % CFG_PP256),
    (conv3(H=384, W=384, Cin=256, halo=0), "ok %d" % CFG_PP256),
    (conv3(H=768, W=768, Cin=256), "ok %d" % CFG_HALO),
    (conv3(H=384, W=384, Cin=256), "ok %d" % CFG_HALO12),
    (conv3(H=768, W=768, Cin=256, N=128), "ok %d" % CFG_HALO_N128),
    # launch_with_short_tail's comment: fc1 at one image is five whole rounds + 224 short tiles (rows1 = 5 * 16 * 256); proj / fc2
    # (340 tiles) one round + a tail; qkv's N = 3072 does not divide the round
    (v(21760, 4096, 1024, tall=0, **ONE_IMAGE), "tail 20480"),
    (v(21760, 1024, 4096, resid=1, tall=0, **ONE_IMAGE), "tail 16384"),
    (v(21760, 3072, 1024, tall=0, **ONE_IMAGE), "single -1"),
    # tall_tile_wins' comment: proj / fc2 at one image are ONE exact round of 352-row tiles; qkv's 768 tall tiles (1056) against 1020
    # tiles of 256 x 256 (1024) is the near-tie the 0.95 gives to the tall tile
    (v(21760, 1024, 1024, resid=1, **ONE_IMAGE), "tall"),
    (v(21760, 3072, 1024, **ONE_IMAGE), "tall"),
    (v(21760, 3072, 1024, bias="1.0", **ONE_IMAGE), "single -1"),
    # fp8_tall_wins' comment: fc1 at one image, 1408 : 1536, stays on the 256-row tile
    (f(21760, 4096, **ONE_IMAGE), "0"),
    (f(21760, 1024, **ONE_IMAGE), "1"),
]


def _cases():
    c = []
    c += ["n %d" % i for i in range(CFG_COUNT)]
    # ---- (1) the recorded problems: each as it was launched; those of the full-size step also under each knob flipped and as the
    # questions split-K asks; the ViT linears among them as the questions gemm_all / resid_all ask (all knob settings for the step's,
    # the tall tile on and off for the sweep's) ----
    vit = []
    for section, kind, a in recorded():
        step = section == "step"
        if kind == "f":
            c += [f(*a, knob=k) for k in (-1, 0, 1)]
            continue
        c.append("r " + " ".join(map(str, a)) + " 0 1 1 1")
        force, M, N, K, seg1, seg2, am, ep = a[:8]
        if step:
            auto = " ".join(map(str, [-1] + a[1:]))
            c += ["r " + auto + " " + knobs for knobs in ("1 1 1 1", "0 0 1 1", "0 1 0 1", "0 1 1 0")]    # dynamic order; halo, halo12, halo128 off
            if am == A_CONV or ep == EPI_STORE:
                c += [s(a[11] * a[12] if am == A_CONV else M, M, N, K, 1, mk) for mk in (4096, 512)]
        if am == A_PLAIN and ep in (EPI_STORE, EPI_RESID_SCALE):
            if force == CFG_PP96:       # the tail of a 256 + 96 split: its rows belong to the launch before it
                vit[-1] = (vit[-1][0] + M,) + vit[-1][1:]
            else:
                vit.append((M, N, K, seg1, seg2, ep, step))
    for M, N, K, seg1, seg2, ep, step in dict.fromkeys(vit):
        resid = int(ep == EPI_RESID_SCALE)
        settings = (dict(), dict(tall=0), dict(tall=0, tail96=0), dict(pp192=1), dict(bias="1.0")) if step else (dict(), dict(tall=0))
        for lnw, lnf in ((0, 0), (1, 1), (1, 0)) if resid and step else ((0, 0),):
            c += [v(M, N, K, seg1, seg2, resid=resid, lnw=lnw, lnf=lnf, **knobs) for knobs in settings]
    # ---- (2) each side of each inequality ----
    # pick_config: t1 255 / 256; N below 128; 512 / 513 small tiles at K 2047 / 2048
    c += [r(M=255 * 128, N=128, K=256), r(M=256 * 128, N=128, K=256), r(M=100000, N=64, K=256), r(M=100000, N=124, K=4096)]
    c += [r(M=Mt * 64, N=64, K=K) for Mt in (512, 513) for K in (2047, 2048)]
    # ... candidates: N below a tile's columns, K < 128 on the two-group tiles, segments off a tile's rows, the residual-only 192-row tile
    # at K 1024 / 1088, static and dynamic order at 256 / 257 and 512 / 513 tiles
    for dyn in (0, 1):
        c += [r(M=M, N=N, K=K, dyn=dyn) for M in (32768, 65536, 65537, 21760) for N in (128, 192, 256, 1024) for K in (64, 128)]
        c += [r(M=M, N=1024, K=K, ep=EPI_RESID_SCALE, dyn=dyn) for M in (21760, 21504, 80780) for K in (1024, 1088, 4096)]
        c += [r(M=21760, N=1024, K=1024, seg1=s1, seg2=s2, ep=ep, dyn=dyn) for s1, s2 in ((768, 1536), (160, 320), (128, 256), (192, 384), (256, 0), (16, 32))
              for ep in (EPI_STORE, EPI_RESID_SCALE)]
        c += [r(M=128 * t, N=256, K=512, dyn=dyn) for t in (255, 256, 257, 511, 512, 513)]
        c += [r(M=160 * t, N=256, K=512, dyn=dyn) for t in (255, 256, 257, 511, 512, 513)]
    # halo promotion: the 0.78-vs-0.97 comparison over batches of 48-multiples, maps that are multiples of 16 or of 12 only, strides, 1x1
    for B in (1, 2, 3, 8):
        c += [conv3(B=B, H=H, W=H, Cin=256) for H in (144, 192, 240, 384, 768)]
    c += [conv3(H=H, W=W, Cin=256) for H, W in ((384, 380), (380, 384), (372, 384), (256, 256), (252, 256))]
    c += [r(M=384 * 384, N=256, K=2304, am=A_CONV, KH=3, KW=3, st=2, oH=384, oW=384, Cin=256),
          r(M=384 * 384, N=256, K=256, am=A_CONV, KH=1, KW=1, st=1, oH=384, oW=384, Cin=256),
          conv3(H=384, W=384, Cin=256, N=512), conv3(H=384, W=384, Cin=256, N=384), conv3(H=384, W=384, Cin=256, N=192)]
    # halo128: 255 / 256 pixel tiles; N a multiple of 256 is the other tile's
    c += [conv3(H=240, W=272, Cin=256, N=128), conv3(H=256, W=256, Cin=256, N=128), conv3(H=256, W=256, Cin=256, N=128, halo128=0),
          conv3(H=256, W=256, Cin=256, N=128, halo=0), conv3(H=256, W=256, Cin=256, N=384), conv3(H=256, W=250, Cin=256, N=128)]
    # K = 64 and K = 128 on every id
    c += [r(i, M=704, N=256, K=K) for i in range(CFG_COUNT) for K in (64, 128)]
    # every (id, A-mode, epilogue): plain linears, the convolution forms, the head's final layers, pairs nothing is compiled for; ids
    # out of range; negative ids are the automatic choice
    for i in list(range(CFG_COUNT)) + [CFG_COUNT, -1, -2]:
        c += [r(i, M=1056, N=256, K=128, ep=ep) for ep in (EPI_STORE, EPI_RESID_SCALE, EPI_PATCH_EMBED, EPI_CONVT, EPI_HEAD_FINAL, EPI_HEAD_COMPOSED)]
        c += [conv3(i, ep=ep) for ep in (EPI_STORE, EPI_RESID_SCALE, EPI_PATCH_EMBED, EPI_CONVT, EPI_HEAD_COMPOSED)]
        c += [conv3(i, H=16, W=16), conv3(i, H=12, W=16), conv3(i, H=8, W=8), conv3(i, N=128)]
        c += [conv3(i, Cin=128, N=32, ep=EPI_HEAD_FINAL), conv3(i, Cin=128, N=32, ep=EPI_HEAD_FINAL, seg1=128)]
    # row segments against each id's alignment
    c += [r(i, M=21760, N=1024, K=1024, seg1=s1, seg2=s2) for i in range(CFG_COUNT)
          for s1, s2 in ((256, 512), (128, 256), (64, 128), (160, 320), (192, 384), (96, 192), (16, 32), (512, 256))]
    # the tap-bias mode and the fused LayerNorm against each id
    c += [conv3(i, H=768, W=768, Cin=256, N=128, tap=1) for i in range(-1, CFG_COUNT + 1)]
    c += [r(i, M=21760, N=1024, K=K, ep=ep, ln=1, **ONE_IMAGE) for i in range(-1, CFG_COUNT + 1) for K in (64, 128) for ep in (EPI_RESID_SCALE, EPI_STORE)]
    c += [conv3(CFG_HALO, H=8, W=8, ln=1), conv3(CFG_PP352, ln=1, ep=EPI_RESID_SCALE)]
    # the ViT linears: grids over the rows across whole rounds, with each knob; C below 256; K below 128; the 192-row tile's K and segments
    for N in (256, 512, 1024, 3072, 4096):
        for M in list(range(256, 256 * 200, 256 * 23)) + [21761, 577]:
            for resid in (0, 1):
                if resid and N > 1024:
                    continue
                K = N if resid else 1024
                c += [v(M, N, K, resid=resid), v(M, N, K, resid=resid, tall=0), v(M, N, K, resid=resid, tall=0, tail96=0)]
    # ... short tail: rem from 0 to past half a round for each column count (2 * rem against per_round, the count of 96-row tiles), less
    # than one round, a last segment beyond the whole rounds
    for N in (256, 512, 1024, 2048, 4096, 3072):
        per_round = 256 // (N // 256) if 256 % (N // 256) == 0 else 21
        for rounds in (0, 1):
            for rem in sorted({0, 1, 96 // (N // 256), 96 // (N // 256) + 1, per_round // 2, per_round // 2 + 1, per_round - 1}):
                M = 256 * (rounds * per_round + rem)
                if M:
                    c += [v(M, N, 1024, C=1024, tall=0), v(M, N, 1024, C=1024, tall=1), v(M, N, 1024, C=1024, tall=0, tail96=0)]
    c += [v(21760, 1024, 1024, seg1=768, seg2=s2, resid=1, tall=0) for s2 in (1536, 16384, 16640)]
    c += [v(21760, 1024, 1024, seg1=s1, resid=1, tall=0) for s1 in (16384, 16640)]
    c += [v(21760, N, K, C=C, resid=resid, tall=tall, **ONE_IMAGE) for N, K, C, resid in ((1024, 64, 1024, 1), (1024, 64, 1024, 0), (192, 192, 192, 1),
                                                                                    (768, 192, 192, 0), (255 * 4, 255, 255, 0), (1024, 1024, 255, 0))
          for tall in (0, 1)]
    c += [v(M, 1024, K, seg1=s1, seg2=s2, resid=1, pp192=p, lnw=lnw, lnf=lnf) for M in (21504, 21760) for K in (1024, 1088)
          for s1, s2 in ((768, 1536), (256, 512)) for p in (0, 1) for lnw, lnf in ((0, 0), (1, 1), (1, 0), (0, 1))]
    # ... both sides of the 0.95: costs 352 r against 256 w, over the tall tile's rounds
    c += [v(M, 1024, 1024, resid=1, bias=b) for M in range(352 * 64 - 704, 352 * 64 * 3, 352 * 16) for b in ("0.95", "0.69", "1.1")]
    # fp8: both sides of the 1.1, the knob
    c += [f(M, N) for N in (256, 1024, 3072, 4096) for M in range(256, 256 * 100, 256 * 9)]
    c += [f(21760, 1024, 768, 1536, k) for k in (-1, 0, 1, 2)] + [f(21760, 4096, 768, 1536, k) for k in (-1, 0, 1, 2)]
    # split-K: off, K against the bound, rows of one image, 199 / 200 tiles, the work-item and K-range bounds of S, the 4096-tile workspace
    c += [s(199 * 128, 199 * 128, 128, 4096), s(200 * 128, 200 * 128, 128, 4096), s(199 * 128, 199 * 128, 128, 4096, on=0),
          s(0, 9216, 256, 9216), s(-1, 9216, 256, 9216), s(9216, 9216, 256, 4032), s(9216, 9216, 256, 4096), s(9216, 9216, 256, 9216)]
    c += [s(128 * t, 128 * t, 128, K, 1, 512) for t in (1, 40, 41, 80, 81, 160, 161) for K in (960, 1024, 2047, 2048, 4095, 4096)]
    c += [s(128, 128 * t, 128, 4096) for t in (4096, 4097)] + [s(2304, 2304 * B, 256, 9216) for B in (1, 2, 8, 64, 128)]
    return list(dict.fromkeys(c))


CASES = _cases()


def case_list_digest():
    import hashlib
    return hashlib.sha256("\n".join(CASES).encode()).hexdigest()


def table():
    """(digest of the case list the answers are for, the answers in the order of CASES).  The file packs many answers to a line, an
    answer's words joined by ':' (`ok:3`, `tail:20480`)."""
    digest, answers = None, []
    for ln in open(os.path.join(GOLDEN, "tile_choice_table.txt")):
        if ln.startswith("# cases "):
            digest = ln.split()[2]
        elif ln.strip() and not ln.startswith("#"):
            answers += [w.replace(":", " ") for w in ln.split()]
    return digest, answers
