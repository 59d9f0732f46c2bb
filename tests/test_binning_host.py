"""The references and generators of tests/binning_cases.py, without a GPU: the pixel rule against the CPU oracle's
`orc_binning_indices_2d`, the image reference against `orc_render_accumulate`, the spectrum membership (np.histogram's counts)
against oracle/spectrum.py, and every case class present and non-empty, so that a generator cannot silently produce nothing."""
import numpy as np
import pytest

import binning_cases as bc
import oracle_bridge as ob
from oracle import spectrum as ospec

IMAGE_CASES = bc.edge_cases() + bc.count_cases() + bc.wave_cases() + [bc.hash_overflow_case(4)]


@pytest.mark.parametrize("case", IMAGE_CASES, ids=repr)
def test_pixel_rule_matches_oracle(case):
    """`pixel_index` gives the oracle's indices for every hit that stays, and drops exactly the hits the oracle drops."""
    h = case.hits
    pix = bc.pixel_index(h.x, h.y, case.Nx, case.Ny, case.extent)
    xi, yi, wm = ob.binning(h.x, h.y, np.ones(h.n, dtype=np.float32), case.Nx, case.Ny, case.extent)
    inside = wm != 0
    assert np.array_equal(inside, pix >= 0)
    assert np.array_equal(yi[inside].astype(np.int64) * case.Nx + xi[inside], pix[inside])
    assert np.all(xi[~inside] == 0) and np.all(yi[~inside] == 0)


@pytest.mark.parametrize("case", bc.edge_cases()[::7] + bc.wave_cases()[:1], ids=repr)
def test_image_reference_matches_oracle(case):
    """`reference_image` (longdouble sums, bounds) against the oracle's sequential f64 image of the same hits, with the hits of
    NaN weight left out: the oracle, like the reference, would carry the NaN into the image, the device drops such a hit."""
    h = case.hits
    keep = ~np.isnan(h.w)
    ref = bc.reference_image(h.x, h.y, h.w, h.wl, case.Nx, case.Ny, case.extent)
    with np.errstate(invalid="ignore"):
        img = ob.render(h.x[keep], h.y[keep], h.w[keep], h.wl[keep], case.extent, case.Nx, case.Ny)
    # (the oracle adds every dropped hit as 0 * observer to pixel (0, 0): NaN there from a dropped hit with a NaN wavelength)
    worst = bc.check_image(img, ref, case.mode, what=case.name)
    assert worst <= 1.0


def test_observer_terms_match_oracle():
    pool, _ = bc.wavelength_pool(np.random.default_rng(0))
    wl = np.concatenate([pool, [np.nan]]).astype(np.float32)
    val, mag = bc.observer_terms(wl)
    want = ob.observers(wl)
    assert np.array_equal(np.isnan(val), np.isnan(want))
    fin = ~np.isnan(want)
    assert np.all(np.abs(val[fin] - want[fin]) <= 3 * bc.EPS * mag[fin])
    tab = bc.observer_table()
    nodes = np.arange(471)
    assert np.array_equal(val[nodes].astype(np.float64), tab[:, 1:])  # the pool starts with the 471 nodes
    assert np.all(val[np.isin(wl, [100.0, 359.5, 830.5, 2000.0])] == 0)


def test_image_case_classes_present():
    seen = {}
    for case in IMAGE_CASES:
        got = case.hits.classes()
        for c in case.expects:
            assert got.get(c, 0) > 0, f"{case.name}: no hit of class {c}"
        for c, n in got.items():
            seen[c] = seen.get(c, 0) + n
        h = case.hits
        huge = h.cls == "huge_index"
        if huge.any():  # finite, and the scaled index of x or y is beyond int32
            x0, x1, y0, y1 = case.extent
            gx = np.floor(case.Nx / (x1 - x0) * (h.x[huge] - x0))
            gy = np.floor(case.Ny / (y1 - y0) * (h.y[huge] - y0))
            assert np.all(np.isfinite(h.x[huge]) & np.isfinite(h.y[huge]))
            assert np.all((gx > 2.0 ** 31) | (gx < -2.0 ** 31) | (gy > 2.0 ** 31) | (gy < -2.0 ** 31))
            assert np.any(gx > 2.0 ** 31) and np.any(gx < -2.0 ** 31) and np.any(gy > 2.0 ** 31) and np.any(gy < -2.0 ** 31)
        # every hit placed on a decision point carries a weight that adds
        placed = np.isin(h.cls, bc.HIT_CLASSES) & ~np.isin(h.wcls, ["w_zero", "w_neg_zero", "w_nan"])
        assert np.all(h.w[placed] != 0) and not np.any(np.isnan(h.w[placed]))
    for c in bc.HIT_CLASSES + bc.WEIGHT_CLASSES + bc.WL_CLASSES + bc.COUNT_CLASSES + bc.WAVE_CLASSES:
        assert seen.get(c, 0) > 0, f"no case holds a hit of class {c}"
    assert {(c.Nx, c.Ny) for c in bc.edge_cases()} == set(bc.SHAPES)
    assert {tuple(c.extent) for c in bc.edge_cases()} == {tuple(float(v) for v in e) for e in bc.EXTENTS.values()}


def test_edge_cases_decide_both_ways():
    """The boundary hits are decision points: in every case some of them stay and some are dropped, and the one-ulp neighbours of
    a boundary fall into different pixels somewhere."""
    for case in bc.edge_cases():
        h = case.hits
        pix = bc.pixel_index(h.x, h.y, case.Nx, case.Ny, case.extent)
        for c in ("extent_edge", "corner"):
            sel = (h.cls == c) & (h.wcls == "w_ordinary") | (h.cls == c) & (h.wcls == "w_negative") | (h.cls == c) & (h.wcls == "w_subnormal")
            assert np.any(pix[sel] >= 0) and np.any(pix[sel] < 0), (case.name, c)
        assert np.all(pix[h.cls == "nonfinite"] < 0) and np.all(pix[h.cls == "huge_index"] < 0)
        if case.Nx > 1:
            b = pix[h.cls == "boundary_x"]
            # the columns are reached from their boundaries (not each one: the rule is inexact, and a boundary with both its
            # neighbours may round into the column below it)
            assert np.unique(b[b >= 0] % case.Nx).size >= case.Nx // 2 + 1, case.name


def test_tile_occupancy_of_count_cases():
    by = {c.name: c for c in bc.count_cases()}

    def tiles(case):
        h = case.hits
        pix = bc.pixel_index(h.x, h.y, case.Nx, case.Ny, case.extent)
        pix = pix[(pix >= 0) & (h.w != 0)]
        tx = (case.Nx + 63) // 64
        return np.bincount((pix // case.Nx // 64) * tx + (pix % case.Nx) // 64, minlength=tx * ((case.Ny + 63) // 64))

    t = tiles(by["two_slabs"])
    assert t[1] > 2 * 16384 and t[7] > 0 and t[[0, 2, 3, 4, 5, 6]].sum() == 0  # chunks of the tile accumulation: 16384 hits
    t = tiles(by["empty_tiles_between"])
    assert np.array_equal(t > 0, [True, False, False, True, False, False, True, False])
    t = tiles(by["last_partial_tile"])
    assert t[7] > 0 and t[:7].sum() == 0


def test_wave_compositions():
    """What the wave cases promise, counted per 64-lane group of the list."""
    case = bc.wave_cases()[0]
    h = case.hits
    pix = np.where(h.w != 0, bc.pixel_index(h.x, h.y, case.Nx, case.Ny, case.extent), -1)
    assert h.n % 64 == 0
    seen = set()
    for g in range(h.n // 64):
        lanes, cls = pix[64 * g:64 * g + 64], h.cls[64 * g]
        ids, counts = np.unique(lanes[lanes >= 0], return_counts=True)
        big = np.sort(counts[counts >= 8])
        if cls == "one_pixel":
            assert counts.tolist() == [64]
        elif cls.startswith("share"):
            assert counts.max() == int(cls[5:]) and np.sum(counts > 1) == 1
        elif cls == "four_keys":
            assert ids.size == 4 and big.size == 4
        elif cls == "eight_by_eight":
            assert counts.tolist() == [8] * 8
        elif cls == "lane63_singleton":
            assert big.size == 2 and np.sum(lanes == lanes[63]) == 1
        elif cls == "lane63_first_key":
            first = lanes[lanes >= 0][0]
            assert lanes[63] == first and np.sum(lanes == first) >= 8 and big.size == 2
        elif cls == "invalid_interleaved":
            assert np.any(lanes < 0) and big.size >= 1
            assert np.any(h.w[64 * g:64 * g + 64] == 0) and np.any(h.x[64 * g:64 * g + 64] > case.extent[1])
        seen.add(cls)
    assert seen >= {"one_pixel", "share7", "share8", "share9", "four_keys", "eight_by_eight", "lane63_singleton",
                    "lane63_first_key", "invalid_interleaved"}
    assert bc.wave_cases()[1].hits.n % 64 == 1 and bc.wave_cases()[2].hits.n % 64 == 63
    # the hash case: nine ids, one slot, one workgroup
    case = bc.wave_cases()[3]
    pix = bc.pixel_index(case.hits.x, case.hits.y, case.Nx, case.Ny, case.extent)
    assert case.hits.n <= 1024 and np.unique(pix).size == 9 and np.unique(bc.hash_slot(np.unique(pix))).size == 1
    case = bc.hash_overflow_case(4)
    pix = bc.pixel_index(case.hits.x, case.hits.y, case.Nx, case.Ny, case.extent).reshape(4, 3072)
    assert all(np.unique(row).size > 2048 for row in pix)


def test_compact_layout():
    rng = np.random.default_rng(5)
    for n in (0, 1, 2, 5, 1023, 1024, 1030, 5000, 40050):
        fill, pos = bc.compact_layout(n, 1024, rng)
        assert fill.shape == (1024,) and int(fill.sum()) == n and np.unique(pos).size == n
        assert np.all(pos % 1024 < fill[pos // 1024])
        if n >= 1030:
            assert fill[0] == 1024 and fill[1] == 0 and fill[2] == 1 and fill[1023] > 0 and np.any(fill[3:1023] == 0)


@pytest.mark.parametrize("case", bc.spectrum_cases(), ids=repr)
def test_spectrum_membership_matches_oracle(case):
    counts = bc.spectrum_counts(case.wl, case.first, case.last, case.nbins)
    edges, sums = ospec.histogram(case.wl, np.ones(case.wl.shape[0], dtype=np.float32), case.first, case.last, case.nbins)
    assert np.array_equal(edges, case.edges)
    assert np.array_equal(sums, counts.astype(np.float64))
    got = case.classes()
    for c in bc.SPECTRUM_CLASSES:
        assert got.get(c, 0) > 0, f"{case.name}: no wavelength of class {c}"
    assert got["edge"] == case.nbins + 1
    # the wavelengths on the edges are decision points: each opens its own bin (the last edge closes the last bin)
    on_edge = case.wl[case.cls == "edge"]
    assert np.array_equal(np.sort(on_edge), case.edges)
    inside = case.wl[(case.wl >= case.first) & (case.wl <= case.last)]
    assert counts.sum() == inside.shape[0]


def test_spectrum_global_atomics_case_is_past_the_lds_limit():
    assert bc.hist_lds_bytes(1001) <= bc.HIST_LDS_LIMIT < bc.hist_lds_bytes(6001)
    assert {c.nbins for c in bc.spectrum_cases()} == set(bc.SPECTRUM_BINS)
