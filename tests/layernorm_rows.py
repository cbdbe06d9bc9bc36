"""The hard rows of test_gpu_ops.py test_layernorm_hard_rows and the bound they are held to, both made without a GPU.

two_pass_f32 restates csrc/elementwise.hip layernorm_kernel operation for operation in f32 -- the sum, the mean
subtracted, the sum of squares, 1 / sqrt(var + eps), (x - mean) * rstd * w + b -- with both sums taken element after
element (numpy's cumsum: the same on every machine).  The kernel sums NPL elements per lane and then across the wave, a
different order, so it is allowed HARD_ROW_FACTOR times the error this restatement has against F.layer_norm in fp64.
test_row_segments_cpu.py re-measures HARD_ROW_ERR."""
import numpy as np
import torch
import torch.nn.functional as F

HARD_DIMS = (64, 256, 512)
EPS = 1e-5
HARD_ROW_ERR = 8.3e-5       # measured: 8.2185e-05, on a mean-100 row of dim 512 (largest |two_pass_f32 - fp64| over HARD_DIMS and the rows below)
HARD_ROW_FACTOR = 4.0

N_CONST, N_MEAN, N_OUTLIER = 3, 24, 1


def hard_rows(dim):
    """(x [rows, dim] f32, w, b): N_CONST constant rows (x = 7.25: the output is the bias exactly), N_MEAN rows with mean 100
    and spread 1, one row with an outlier channel of +40"""
    g = torch.Generator().manual_seed(4000 + dim)
    const = torch.full((N_CONST, dim), 7.25)
    mean = 100.0 + torch.randn(N_MEAN, dim, generator=g)
    out = torch.randn(N_OUTLIER, dim, generator=g)
    out[:, 17] += 40.0
    w = 1 + 0.02 * torch.randn(dim, generator=g)
    b = 0.02 * torch.randn(dim, generator=g)
    return torch.cat([const, mean, out]).contiguous(), w, b


def two_pass_f32(x, w, b, eps=EPS):
    x, w, b = (t.numpy().astype(np.float32) for t in (x, w, b))
    dim = np.float32(x.shape[1])
    one = np.float32(1.0)
    mean = np.cumsum(x, axis=1, dtype=np.float32)[:, -1:] * (one / dim)
    d = x - mean
    var = np.cumsum(d * d, axis=1, dtype=np.float32)[:, -1:] * (one / dim)
    rstd = one / np.sqrt(var + np.float32(eps))
    return torch.from_numpy(d * rstd * w + b)


def reference(x, w, b, eps=EPS):
    return F.layer_norm(x.double(), (x.shape[1],), w.double(), b.double(), eps)


def measured_error():
    """largest |two_pass_f32 - fp64| over HARD_DIMS on the mean-100 and outlier rows"""
    worst = 0.0
    for dim in HARD_DIMS:
        x, w, b = hard_rows(dim)
        err = (two_pass_f32(x, w, b).double() - reference(x, w, b)).abs()[N_CONST:]
        worst = max(worst, float(err.max()))
    return worst
