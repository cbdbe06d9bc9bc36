"""The output back end's shape and edge cases, CPU side (no GPU): every case of tests/output_cases.py is ADMITTED from the C
oracle alone, so that tests/test_gpu_output_shapes.py cannot pass because its input was dull.

Mesh: a `scene` or `nan` map keeps some triangles and drops some, leaves a vertex unused away from the last row and column
    and (from 1025 quads on) one in the last row and one in the last column; `border` leaves the whole last row and column
    unused; `checker` keeps nothing; `flat` keeps everything.
Stereogram: the bounds-checked oracle returns 0 for every tall and square case and -1 for the wide maps (cols > rows), the
    evidence that the library's refusal refuses only what the reference cannot do; amplitude 0.6 gives the noise back,
    amplitude 0.0005 has pattern_width 0, and a caller's range narrower than the data takes forward references.
Clamp: no map is all NaN, every special value occurs, a NaN stands at index 0, and (min, max) of the `inner` maps are the
    data's own.
These are conditions, not measurements: a map that misses one gets another seed or planting, never a weaker condition."""
import numpy as np
import pytest

from oracle import output_oracle as OO
import output_cases as X


@pytest.mark.parametrize("name", [c.name for c in X.MESH_CASES])
def test_mesh_case_is_admitted(name):
    case = X.MESH_BY_NAME[name]
    w, h, nq = case.width, case.height, case.nquads
    assert nq == (w - 1) * (h - 1) and X.mesh_map(name).shape == (w, h)
    od, vi, nv, faces = X.mesh_oracle(name)
    raw = X.mesh_map(name)
    assert np.array_equal(od.view(np.uint32), raw.view(np.uint32))     # what was planted lies inside the clamp range
    v = vi.reshape(h, w)                                               # the mesh view
    nf = len(faces)
    if case.content in ("scene", "nan"):
        assert 0 < nf < 2 * nq
        assert (v[:h - 1, :w - 1] < 0).any()            # unused, and written by the quad whose own corner it is
        if case.border_spikes:
            assert (v[h - 1, :] < 0).any() and (v[:, w - 1] < 0).any()
            assert (v[h - 1, :] >= 0).any() and (v[:, w - 1] >= 0).any()      # ... beside used ones
        if case.content == "nan":
            nans = X.mesh_nan_positions(case)
            assert len(set((x, y) for x, y, _ in nans)) == len(nans)
            for x, y, neg in nans:
                assert np.isnan(od.reshape(h, w)[y, x]) and bool(np.signbit(od.reshape(h, w)[y, x])) == neg
                assert v[y, x] == -1
            assert int(np.isnan(od).sum()) == len(nans)
        else:
            assert not np.isnan(od).any()
    elif case.content == "border":
        assert (v[h - 1, :] == -1).all() and (v[:, w - 1] == -1).all()
        assert nf == 2 * (w - 2) * (h - 2)                  # every quad clear of the border is whole, on a strip none is
        assert nv == ((w - 1) * (h - 1) if nf else 0)
    elif case.content == "checker":
        assert nv == 0 and nf == 0 and (v == -1).all()
    else:
        assert case.content == "flat" and nv == w * h and nf == 2 * nq and (v >= 0).all()


def test_mesh_table_covers_the_workgroup_edges():
    quads = {c.shape: c.nquads for c in X.MESH_CASES}
    assert quads[(4, 342)] == 1023 and quads[(3, 513)] == 1024 and quads[(26, 42)] == 1025
    assert quads[(131, 601)] == quads[(601, 131)] == 78000 and -(-78000 // 1024) == 77 > 64
    assert {c.content for c in X.MESH_CASES} == set(X.MESH_CONTENTS)
    assert all(n in X.MESH_BY_NAME for n in X.MESH_FILE_CASES)
    assert X.mesh_oracle("5x7-checker")[2] == 0       # the zero-face file


def test_depth_generator_is_unchanged_on_square_maps():
    """_depth moved here from test_gpu_output.py and learnt (rows, cols): an n x n map is value for value what it was"""
    def old(n, seed=0, kind="scene"):
        rng = np.random.default_rng(seed)
        yy, xx = np.meshgrid(np.linspace(0, 1, n, dtype=np.float32), np.linspace(0, 1, n, dtype=np.float32),
                             indexing="ij")
        d = 0.2 + 0.15 * np.sin(3 * xx + 2 * yy) + 0.1 * yy
        if kind == "scene":
            for _ in range(6):
                x0, y0 = rng.integers(0, n - n // 4, size=2)
                w, h = rng.integers(n // 16, n // 4, size=2)
                d[y0:y0 + h, x0:x0 + w] += rng.uniform(0.2, 1.5)
            d += rng.normal(0, 0.002, size=d.shape).astype(np.float32)
        return np.ascontiguousarray(d.astype(np.float32))
    for n, seed, kind in ((16, 0, "scene"), (48, 8, "scene"), (64, 66, "smooth"), (257, 259, "scene"), (333, 334, "scene")):
        assert np.array_equal(X._depth(n, seed=seed, kind=kind), old(n, seed, kind))
        assert np.array_equal(X._depth((n, n), seed=seed, kind=kind), old(n, seed, kind))
    assert X._depth((96, 40), seed=1).shape == (96, 40) and X._depth((300, 2), seed=1).shape == (300, 2)


@pytest.mark.parametrize("name", [c.name for c in X.STEREO_CASES])
def test_stereogram_case_is_admitted(name):
    case = X.STEREO_BY_NAME[name]
    od, mn, mx = X.stereo_map(case.map)
    assert od.shape[0] >= od.shape[1] and mn < mx
    rc, out, fwd, strict = X.stereo_oracle(name)
    assert rc == 0                                   # tall and square maps are well defined at every size
    noise = X.stereo_noise(case.out_w, case.out_h)
    pw = X.pattern_width(case.out_w, case.amplitude)
    if case.amplitude == X.AMP_BIG:
        assert pw > case.out_w and np.array_equal(out, noise)
    elif case.amplitude == X.AMP_ZERO:
        assert pw == 0 and case.out_w < 500
        assert fwd == case.out_w * case.out_h and strict == 0     # every pixel refers to itself: the shift == 0 branch
    elif case.out_w == 1:
        assert pw == 0 and (fwd, strict) == (case.out_h, 0)
    else:
        assert 0 < pw <= case.out_w
        assert (fwd, strict) == (0, 0)               # the map's own range never refers forward
        if case.out_w > pw:
            assert not np.array_equal(out, noise)
    assert np.isnan(od).sum() == (1 if case.map.endswith("-nan") else 0)


@pytest.mark.parametrize("name", [c.name for c in X.NARROW_CASES])
def test_narrow_range_case_takes_forward_references(name):
    case = X.STEREO_BY_NAME[name]
    od, mn, mx = X.stereo_map(case.map)
    lo, hi = X.stereo_range(case)
    assert mn < lo < hi < mx
    rc, out, fwd, strict = X.stereo_oracle(name)
    assert rc == 0 and fwd >= 1 and strict >= 1
    # and the forward references are in the picture: the map's own range gives another one
    _, own, _, _ = OO.stereogram_counted(od, mn, mx, case.out_w, case.out_h, case.amplitude,
                                         X.stereo_noise(case.out_w, case.out_h))
    assert not np.array_equal(out, own)


def test_stereogram_table_covers_the_listed_sizes():
    for m in X.STEREO_MAPS:
        sizes = {(c.out_w, c.out_h) for c in X.STEREO_CASES if c.map == m and c.amplitude == 1.0 / 16.0}
        assert sizes == set(X.STEREO_SIZES)
        assert {c.amplitude for c in X.STEREO_CASES if c.map == m} == {1.0 / 16.0, 0.125, X.AMP_BIG, X.AMP_ZERO}
    assert len({c.name for c in X.STEREO_CASES + X.NARROW_CASES}) == len(X.STEREO_CASES) + len(X.NARROW_CASES)


@pytest.mark.parametrize("name", list(X.STEREO_WIDE))
def test_oracle_refuses_the_wide_maps(name):
    """cols > rows: the reference's data[cols * y + x] passes the end of the map once y reaches the lower rows, and panics"""
    od, mn, mx = X.stereo_map(name)
    rows, cols = od.shape
    assert cols > rows
    for out_w, out_h in ((64, 2 * cols), (257, 2 * cols), (1, 2 * cols + 1)):
        noise = X.stereo_noise(out_w, out_h)
        assert OO.stereogram_counted(od, mn, mx, out_w, out_h, 1.0 / 16.0, noise)[0] == -1
        with pytest.raises(IndexError):
            OO.stereogram(od, mn, mx, out_w, out_h, 1.0 / 16.0, noise)
    # the transposed (tall) map of the same values is fine
    t = np.ascontiguousarray(od.T)
    assert OO.stereogram_counted(t, mn, mx, 64, 2 * cols, 1.0 / 16.0, X.stereo_noise(64, 2 * cols))[0] == 0


def test_oracle_reports_the_row_index_panic_as_before():
    """the -1 the oracle already had: a range so narrow that a source index reaches out_w (output.rs:181)"""
    od, mn, mx = X.stereo_map("64x64")
    noise = X.stereo_noise(513, 2)
    assert OO.stereogram_counted(od, mn, mn + (mx - mn) / 64, 513, 2, 1.0 / 16.0, noise)[0] == -1


@pytest.mark.parametrize("content", X.CLAMP_CONTENTS)
@pytest.mark.parametrize("count", X.CLAMP_COUNTS)
def test_clamp_case_is_admitted(count, content):
    d = X.clamp_case(count, content)
    od, mn, mx = X.clamp_oracle(count, content)
    assert d.shape == (count,) and not np.isnan(d).all()
    assert np.isfinite(mn) and np.isfinite(mx) and X.LO <= mn <= mx <= X.HI
    keep = ~np.isnan(d)
    assert np.array_equal(od.view(np.uint32)[~keep], d.view(np.uint32)[~keep])      # NaNs pass with sign and payload
    assert mn == od[keep].min() and mx == od[keep].max()
    if content == "inner":
        assert np.array_equal(od.view(np.uint32), d.view(np.uint32))                # nothing is clamped
        if count >= 5:
            assert (mn, mx) == (od[count - 1], od[count - 2]) and X.LO < mn and mx < X.HI
    elif count >= 64:
        have = set(d.view(np.uint32).tolist())
        assert all(int(s) in have for s in X.CLAMP_SPECIALS.view(np.uint32))
        assert (mn, mx) == (X.LO, X.HI)


def test_clamp_table_covers_the_kernel_paths():
    assert X.CLAMP_COUNTS[-1] > 512 * 256 * 16 and X.CLAMP_COUNTS[-1] % 4 == 3        # past the grid's cap, with a tail
    assert {c % 4 for c in X.CLAMP_COUNTS} == {0, 1, 2, 3}
    assert any(np.isnan(X.clamp_case(c, k)[0]) for c in X.CLAMP_COUNTS for k in X.CLAMP_CONTENTS)
    s = X.CLAMP_SPECIALS
    assert np.isnan(s[:4]).all() and np.signbit(s[:4]).tolist() == [False, True, False, True]
    assert 0 < s[9] < np.finfo(np.float32).tiny                                     # the subnormal
    # the specials clamp as f32::clamp does: NaN kept, everything below 1/250 (zeros, negatives, -inf) to it
    od, _, _ = OO.clamp_minmax(s)
    assert np.array_equal(od[4:], np.array([X.HI, X.LO, X.LO, X.LO, X.LO, X.LO, X.LO, X.HI, X.LO,
                                            np.nextafter(X.LO, np.float32(1)), np.nextafter(X.HI, np.float32(0)), X.HI],
                                           np.float32))


@pytest.mark.parametrize("content", X.COLOUR_CONTENTS)
@pytest.mark.parametrize("shape", X.COLOUR_SHAPES)
def test_colour_case_is_admitted(shape, content):
    od, mn, mx = OO.clamp_minmax(X.colour_map(shape, content))
    rgb = OO.depthmap_rgb(od, mn, mx)
    assert rgb.shape == shape + (3,)
    if content == "flat":
        assert mn == mx and (rgb == 0).all()         # t = 0 / 0: NaN -> `as u8` 0 in every channel
    else:
        assert mn < mx and len(np.unique(rgb.reshape(-1, 3), axis=0)) >= 3
        assert int(np.isnan(od).sum()) == (3 if content == "nan" else 0)
