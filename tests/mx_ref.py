"""A torch restatement of the OCP MX rule of csrc/mx_fp8.h (e4m3 elements, one e8m0 scale per 32 of them), shared by
the fp8 tests: the quantisers are compared with it code for code."""
import numpy as np
import torch

E4M3 = torch.float8_e4m3fn


def scale_bytes(blocks_amax):
    """the rule of csrc/mx_fp8.h mx_scale_byte: exponent of amax - 8, one more when the significand is >= 1.75, so
    that no scaled element exceeds e4m3's 448"""
    bits = blocks_amax.float().contiguous().view(torch.int32).to(torch.int64) & 0x7fffffff
    e = (bits + 0x200000) >> 23
    return torch.clamp(e - 8, 0, 254).to(torch.uint8)


def quantize_ref(x):
    """x [rows, K] f32 -> (e4m3 tensor [rows, K], scale bytes [rows, K/32])"""
    rows, K = x.shape
    b = x.float().reshape(rows, K // 32, 32)
    sb = scale_bytes(b.abs().amax(dim=2))
    inv = torch.where(sb == 0, torch.tensor(1.7014118e38), torch.pow(2.0, 127.0 - sb.float()))
    q = (b * inv.unsqueeze(2)).to(E4M3)
    return q.reshape(rows, K), sb


def dequant(q8, sb):
    rows, K = q8.shape
    return (q8.float().reshape(rows, K // 32, 32).double() * torch.pow(2.0, sb.double() - 127.0).unsqueeze(2)).reshape(rows, K)


def scale_positions(ctx, rows, K, weight_layout, row_list=None):
    """byte position of (row, K block) in the packed scales of an operand of `rows` rows, for the rows of row_list (all
    by default), via me_op_scale_index -> int64 [len(row_list), K/32]"""
    fn = ctx.lib.me_op_scale_index
    row_list = range(rows) if row_list is None else row_list
    return np.array([[fn(int(r), kb, rows, weight_layout) for kb in range(K // 32)] for r in row_list], np.int64).reshape(-1, K // 32)


def read_scales(ctx, packed, rows, K, weight_layout):
    """packed scale bytes (device) -> [rows, K/32] via me_op_scale_index"""
    host = packed.cpu().numpy()
    return torch.from_numpy(host[scale_positions(ctx, rows, K, weight_layout)])
