"""Plain references of the layout / element-wise kernels (csrc/elementwise.hip) and of the [hi | lo] operand split:
a few lines of torch indexing each, no arithmetic beyond what the kernel itself does.  test_layout_refs_cpu.py ties
them to oracle/depth_pro_oracle.py; test_gpu_layout.py and test_gpu_split_forms.py hold the kernels to them."""
import torch

# |hi + lo - v| of split_hi_lo, asserted by test_layout_refs_cpu.py on 10 M values so that the GPU tests may use them as constants
SPLIT_REL = {torch.float16: 2.0 ** -22, torch.bfloat16: 2.0 ** -16}   # relative to |v| (f16: where |v| >= 2^-3)
SPLIT_ABS_F16 = 2.0 ** -25                                            # f16 below 2^-3: the subnormal grid of the lo part
EPS16 = {torch.float16: 2.0 ** -11, torch.bfloat16: 2.0 ** -8}        # half an ulp, relative: one rounding


def split_hi_lo(v: torch.Tensor, T: torch.dtype):
    """Split operands (csrc/gemm_core.h store_16bit_lo): hi = T(v), lo = T(v - hi) with an overflowed hi keeping lo = 0."""
    v = v.float()
    hi = v.to(T)
    lo = torch.where(torch.isfinite(hi), v - hi.float(), torch.zeros_like(v)).to(T)
    return hi, lo


def ulp16(hi: torch.Tensor) -> torch.Tensor:
    """Spacing of the 16-bit grid at hi (f64), with the subnormal floor."""
    fi = torch.finfo(hi.dtype)
    mant = {torch.float16: 10, torch.bfloat16: 7}[hi.dtype]
    a = hi.double().abs().clamp_min(fi.smallest_normal)
    return torch.exp2(torch.floor(torch.log2(a)) - mant)


def patchify_windows(xs: torch.Tensor, grid: int) -> torch.Tensor:
    """[W][3][16 g][16 g] -> im2col rows [W * g * g][c * 256 + iy * 16 + ix] of the 16 x 16 stride-16 patch embed."""
    W, C, S, _ = xs.shape
    assert C == 3 and S == 16 * grid
    p = xs.reshape(W, 3, grid, 16, grid, 16).permute(0, 2, 4, 1, 3, 5)    # [W][py][px][c][iy][ix]
    return p.reshape(W * grid * grid, 768)


def window_origins(grid: int):
    """(level, y, x) of the 35 windows of one image in the order 25 + 9 + 1 (encoder.rs:142-156 split at overlap 1/4 and
    1/2 of a 16 g window on the 64 g, 32 g and 16 g pyramid levels)."""
    wp = 16 * grid
    out = [(0, j * (wp - wp // 4), i * (wp - wp // 4)) for j in range(5) for i in range(5)]
    out += [(1, j * (wp - wp // 2), i * (wp - wp // 2)) for j in range(3) for i in range(3)]
    return out + [(2, 0, 0)]


def windows_of(x0, x1, x2, grid: int) -> torch.Tensor:
    """The window stack [B * 35][3][16 g][16 g], image-major (b * 35 + win)."""
    wp = 16 * grid
    lv = (x0, x1, x2)
    B = x0.shape[0]
    wins = [lv[l][b:b + 1, :, y:y + wp, x:x + wp] for b in range(B) for (l, y, x) in window_origins(grid)]
    return torch.cat(wins, dim=0)


def patchify(x0, x1, x2, grid: int) -> torch.Tensor:
    """patchify_kernel: rows ((b * 35 + win) * g * g + py * g + px) of the three pyramid levels' windows."""
    return patchify_windows(windows_of(x0, x1, x2, grid), grid)


def cls_rows(tokens: torch.Tensor, cls: torch.Tensor, pos: torch.Tensor) -> torch.Tensor:
    """tokens [W][T][C]: row 0 of every window = cls + pos[0] (one f32 addition); the other rows as they were."""
    out = tokens.clone()
    out[:, 0, :] = cls + pos[0]
    return out


def merge(tok: torch.Tensor, batch: int, wpi: int, win0: int, steps: int, padding: int, grid: int) -> torch.Tensor:
    """reshape_feature + merge (encoder.rs:158-208) of windows win0 .. win0 + steps^2 - 1 of each image's wpi windows:
    tok [batch * wpi][g * g + 1][C] -> NHWC [batch][side][side][C], values untouched."""
    C = tok.shape[-1]
    t = tok.reshape(batch, wpi, grid * grid + 1, C)[:, :, 1:, :].reshape(batch, wpi, grid, grid, C)
    rows = []
    for j in range(steps):
        row = []
        for i in range(steps):
            h0 = padding if j > 0 else 0
            h1 = grid - padding if j < steps - 1 else grid
            w0 = padding if i > 0 else 0
            w1 = grid - padding if i < steps - 1 else grid
            row.append(t[:, win0 + j * steps + i, h0:h1, w0:w1, :])
        rows.append(torch.cat(row, dim=2))
    return torch.cat(rows, dim=1)


def nchw_to_nhwc(x: torch.Tensor) -> torch.Tensor:
    return x.permute(0, 2, 3, 1).contiguous()


def nhwc_to_nchw(x: torch.Tensor) -> torch.Tensor:
    return x.permute(0, 3, 1, 2).contiguous()


def into_border(canvas: torch.Tensor, x_nhwc: torch.Tensor) -> torch.Tensor:
    """x [B][H][W][C] written into the interior of canvas [B][H+2][W+2][C]; the border keeps the canvas's values."""
    out = canvas.clone()
    out[:, 1:-1, 1:-1, :] = x_nhwc
    return out


def split_pixels(v_nhwc: torch.Tensor, T: torch.dtype) -> torch.Tensor:
    """[..][C] f32 -> [..][2 C] pixels of [hi | lo]."""
    hi, lo = split_hi_lo(v_nhwc, T)
    return torch.cat([hi, lo], dim=-1)


def concat_channels(a: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
    return torch.cat([a, b], dim=-1)


def fov_add(lin: torch.Tensor, low: torch.Tensor, grid: int) -> torch.Tensor:
    """fov.rs:66-74: tokens [B][T][C] without their cls row, as a [B][g][g][C] map, + low [B][g * g][C]; one f32 addition."""
    B, _, C = lin.shape
    return (lin[:, 1:, :] + low).reshape(B, grid, grid, C)


def patch_embed_tokens(patches: torch.Tensor, w: torch.Tensor, bias: torch.Tensor, pos: torch.Tensor, cls: torch.Tensor,
                       P: int) -> torch.Tensor:
    """vit.rs:287-295 in fp64: patches [W * P][768], w [C][768], pos [P + 1][C], cls [C] -> tokens [W][P + 1][C] with
    row 0 = cls + pos[0] and row 1 + p = patches . w^T + bias + pos[1 + p]."""
    C = w.shape[0]
    y = (patches.double() @ w.double().T + bias.double()).reshape(-1, P, C) + pos.double()[1:]
    c = (cls.double() + pos.double()[0]).expand(y.shape[0], 1, C)
    return torch.cat([c, y], dim=1)
