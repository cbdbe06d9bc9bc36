"""CPU tests of tests/row_segments_ref.py and tests/layernorm_rows.py: the row map and the bound that
test_gpu_row_segments.py and test_gpu_ops.py hold the HIP kernels to are themselves held here, so the GPU tests do not
rest on an unchecked restatement."""
import pytest

import layernorm_rows as LR
import row_segments_ref as R


def _check_layout(lay, W1, W0, fov):
    T = lay.tokens
    assert lay.windows == W0 + W1 * (2 if fov else 1)
    assert lay.seg1 > 0 and lay.seg1 % 256 == 0 and lay.seg2 % 256 == 0 and lay.rows_total % 256 == 0
    assert (lay.seg2 > lay.seg1) if fov else (lay.seg2 == 0)
    assert (lay.win0, lay.win1) == (W1, W1 if fov else W0)
    bounds = R.segment_bounds(lay)
    assert [n for _, _, n in bounds] == ([W1, W1, W0] if fov else [W1, W0])
    assert bounds[0][0] == 0 and bounds[-1][1] == lay.rows_total
    assert all(a[1] == b[0] for a, b in zip(bounds, bounds[1:]))                    # the segments tile the row space
    rows = R.window_rows(lay)
    assert len(rows) == lay.windows
    # window w of segment s is that segment's window w - (windows before s), `tokens` rows apart from the segment's start
    win = 0
    for lo, hi, n in bounds:
        for i in range(n):
            assert rows[win] == lo + i * T and rows[win] + T <= hi, (win, lo, hi)  # inside its segment
            win += 1
        assert hi - (lo + n * T) < 256                                              # padded to 256 rows, no further
    # disjoint, and with the padding rows exactly [0, rows_total)
    used = [r for r0 in rows for r in range(r0, r0 + T)]
    assert len(set(used)) == len(used) == lay.windows * T
    pad = R.padding_rows(lay)
    assert sorted(used + pad) == list(range(lay.rows_total))
    return pad


@pytest.mark.parametrize("T", [65, 577])
@pytest.mark.parametrize("fov", [0, 1])
@pytest.mark.parametrize("B", [1, 2, 8])
def test_layout_of_the_merged_vit(B, fov, T):
    """the encoder's own layouts: 35 B windows of the patch encoder, B of each small ViT"""
    lay = R.layout(T, B, 35 * B, fov)
    _check_layout(lay, B, 35 * B, fov)
    assert lay.rows_total == (2 if fov else 1) * R.pad256(B * T) + R.pad256(35 * B * T)


def test_first_row():
    assert [R.first_row(w, 10, 0, 0, 0, 0) for w in range(3)] == [0, 10, 20]                   # no segmentation
    assert [R.first_row(w, 10, 256, 0, 2, 3) for w in range(5)] == [0, 10, 256, 266, 276]
    assert [R.first_row(w, 10, 256, 512, 2, 1) for w in range(5)] == [0, 10, 256, 512, 522]
    assert [R.first_row(w, 10, 256, 512, 0, 1) for w in range(3)] == [256, 512, 522]           # an empty first segment


def test_gpu_case_list():
    """every case of test_gpu_row_segments.py fits its row space; the list has a small segment without padding rows, one
    with, two- and three-segment layouts and the model's width"""
    no_padding = padded = 0
    for tokens, W1, W0, heads, fov in R.CASES:
        lay = R.layout(tokens, W1, W0, fov)
        pad = _check_layout(lay, W1, W0, fov)
        if W1 * tokens == lay.seg1:
            no_padding += 1
            assert not [r for r in pad if r < lay.seg1]
        else:
            padded += 1
        assert heads % 2 == 0                                                       # the fp8 output needs whole 128-column tiles
    assert no_padding >= 1 and padded >= 1
    assert {c[4] for c in R.CASES} == {0, 1} and any(c[3] == 16 for c in R.CASES)
    assert any(c[0] > 512 for c in R.CASES) and any(c[0] % 32 == 1 and c[0] < 64 for c in R.CASES) and any(c[0] == 1 for c in R.CASES)


def test_hard_row_bound_is_the_measured_one():
    """HARD_ROW_ERR is the f32 two-pass restatement's own error against fp64 (rounded up), not a number chosen to fit"""
    err = LR.measured_error()
    assert err <= LR.HARD_ROW_ERR <= 1.05 * err, err
    for dim in LR.HARD_DIMS:                                                         # a constant row gives the bias exactly
        x, w, b = LR.hard_rows(dim)
        assert bool((LR.two_pass_f32(x, w, b)[:LR.N_CONST] == b).all())
