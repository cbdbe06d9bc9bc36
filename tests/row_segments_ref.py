"""The row space of the encoder's merged ViT launches, restated in plain Python from the comment at csrc/common.h
(RowSegs) and the constructor of csrc/pipeline.hip MergedVit -- not by calling the library: test_gpu_row_segments.py
holds the kernels' window -> row map to this one, test_row_segments_cpu.py holds this one to the properties a row
space must have.

Row segments: segment 0 = rows [0, seg1), 1 = [seg1, seg2), 2 = [seg2, rows_total).  Windows are contiguous (`tokens`
rows apart) inside a segment; win0 / win1 are the numbers of windows of segments 0 and 1; the windows after them belong
to the last segment.  seg2 == 0: two segments.  seg1 == 0: no segmentation, the windows lie back to back from row 0."""
from collections import namedtuple

Layout = namedtuple("Layout", "tokens windows seg1 seg2 win0 win1 rows_total")

PAD = 256       # every segment is padded to a multiple of this many rows


def first_row(win, tokens, seg1, seg2, win0, win1):
    """the first row of window `win`"""
    if seg1 == 0 or win < win0:
        return win * tokens
    if win < win0 + win1:
        return seg1 + (win - win0) * tokens
    return seg2 + (win - win0 - win1) * tokens


def pad256(rows):
    return (rows + PAD - 1) // PAD * PAD


def layout(tokens, W1, W0, fov):
    """MergedVit's physical order, the SMALL segments first: [image | fov | patch] (without the FOV head: [image | patch]);
    W1 windows in each small segment, W0 in the patch encoder's; every segment padded to 256 rows."""
    side = pad256(W1 * tokens)
    seg1 = side
    seg2 = 2 * side if fov else 0
    rows_total = (seg2 if fov else seg1) + pad256(W0 * tokens)
    return Layout(tokens, W0 + W1 * (2 if fov else 1), seg1, seg2, W1, W1 if fov else W0, rows_total)


def unsegmented(tokens, windows):
    return Layout(tokens, windows, 0, 0, 0, 0, windows * tokens)


def window_rows(lay):
    """first row of every window, in window order"""
    return [first_row(w, lay.tokens, lay.seg1, lay.seg2, lay.win0, lay.win1) for w in range(lay.windows)]


def segment_bounds(lay):
    """[(first row, end row, windows)] of the segments"""
    if lay.seg1 == 0:
        return [(0, lay.rows_total, lay.windows)]
    if lay.seg2 == 0:
        return [(0, lay.seg1, lay.win0), (lay.seg1, lay.rows_total, lay.windows - lay.win0)]
    return [(0, lay.seg1, lay.win0), (lay.seg1, lay.seg2, lay.win1), (lay.seg2, lay.rows_total, lay.windows - lay.win0 - lay.win1)]


def padding_rows(lay):
    """the rows that belong to no window, ascending"""
    used = set()
    for r0 in window_rows(lay):
        used.update(range(r0, r0 + lay.tokens))
    return [r for r in range(lay.rows_total) if r not in used]


# (tokens, W1, W0, heads, fov): the smallest layouts that still have a ragged key tile, the single tail key, a second query
# block and all three segments
CASES = [
    (65, 1, 3, 2, 1),       # the tiny model's own
    (65, 4, 5, 2, 0),       # 260 rows padded to 512
    (128, 2, 3, 2, 1),      # small segments exactly 256 rows: no padding
    (577, 1, 2, 2, 1),      # 768-row segments, 1154 rows padded to 1280
    (577, 2, 1, 16, 0),     # the model's C = 1024
    (1, 1, 1, 2, 1),        # one token per window
    (33, 1, 2, 2, 0),       # the vector-pipe extra query
]
