"""The integer layer of the host replay of the ray generator (tests/generate_replay.py), on a machine without a device: Philox
against the Random123 known answers, the keyed permutations as bijections, the lattice multiplier of the RGB choice
variable, the dither fields of every source kind, and the reciprocal fix-up of the grid row against divmod."""
import itertools

import numpy as np
import pytest

import generate_replay as gr


def _words(s):
    return [int(v, 16) for v in s.split()]


@pytest.mark.parametrize("counter, key, want", [
    ("0 0 0 0", "0 0", "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
    ("ffffffff ffffffff ffffffff ffffffff", "ffffffff ffffffff", "408f276d 41c83b0e a20bc7c6 6d5451fd"),
    ("243f6a88 85a308d3 13198a2e 03707344", "a4093822 299f31d0", "d16cfe09 94fdcceb 5001e420 24126ea1"),
])
def test_philox_known_answers(counter, key, want):
    """Philox4x32-10, kat_vectors of Random123; the generator's 7-round variant is the same function with rounds=7."""
    got = gr.philox4x32(np.array(_words(counter)), np.array(_words(key)), 10)
    assert got.dtype == np.uint32 and got.tolist() == _words(want)
    seven = gr.philox4x32(np.array(_words(counter)), np.array(_words(key)), 7)
    assert seven.tolist() != got.tolist()
    # vectorised over a leading axis: the same words row by row
    both = gr.philox4x32(np.array([_words(counter)] * 3), np.array([_words(key)] * 3), 10)
    assert both.shape == (3, 4) and all(row.tolist() == _words(want) for row in both)


KEYS = [0, 0x9E3779B9, 0xffffffff, gr.stream_key(77, 3, gr.ST_POS), gr.stream_key((5 << 32) | 9, 0, gr.ST_WL)]


def _is_bijection(l, key):
    got = gr.permute_index(np.arange(l), l, key)
    return got.shape == (l,) and np.array_equal(np.sort(got), np.arange(l, dtype=np.uint64))


def test_permute_index_is_a_bijection_small():
    for l in range(1, 4098):
        for key in KEYS[:3] if l > 700 else KEYS:
            assert _is_bijection(l, key), (l, key)


@pytest.mark.parametrize("l", [65535, 65536, 70001, 1 << 20, 1 << 21])
def test_permute_index_is_a_bijection_large(l):
    for key in KEYS[1:4]:
        assert _is_bijection(l, key), (l, key)
    # two keys give two permutations
    assert not np.array_equal(gr.permute_index(np.arange(l), l, KEYS[1]), gr.permute_index(np.arange(l), l, KEYS[3]))


def test_rgb_lattice_multiplier():
    """k -> (k * mult + c) & (n - 1) with mult = (0x9E3779B1 >> (32 - m)) | 1: odd, so a bijection of [0, 2^m)."""
    for m in range(1, 32):
        assert ((0x9E3779B1 >> (32 - m)) | 1) & 1
    for m in range(1, 21):
        n, mult = 1 << m, (0x9E3779B1 >> (32 - m)) | 1
        for c in (0, 1, 0x12345678):
            k = (np.arange(n, dtype=np.uint64) * np.uint64(mult) + np.uint64(c)) & np.uint64(n - 1)
            assert np.array_equal(np.sort(k), np.arange(n, dtype=np.uint64)), (m, c)


SHAPES = {"image_rgb": gr.SRC_IMAGE_RGB, "image_gray": gr.SRC_IMAGE_GRAY, "extended": gr.SRC_RECT, "line": gr.SRC_LINE,
          "point": gr.SRC_POINT}
DIVS = {"none": (gr.DIV_NONE, 0), "3d": (gr.DIV_ISOTROPIC, 0), "2d": (gr.DIV_TABLE, 1)}


@pytest.mark.parametrize("shape, div", list(itertools.product(SHAPES, DIVS)))
def test_slot_table(shape, div):
    """The streams one source reads occupy pairwise disjoint bit fields of the blocks it draws, and block B is read only where
    it is drawn (extended emitters and 2-D divergence)."""
    sh, (dv, d2) = SHAPES[shape], DIVS[div]
    image, has_b = sh >= gr.SRC_IMAGE_RGB, gr.needs_block_b(sh, dv, d2)
    assert has_b == ((shape in ("extended", "line")) or div == "2d")
    used = {}
    for stream, count in gr.streams_read(sh, dv, d2):
        for slot in range(gr.dither_slot(stream), gr.dither_slot(stream) + count):
            block, word, shift, bits = gr.dither_field(slot, image)
            assert bits == (16 if image and block == 0 else 32)
            assert block == 0 or has_b, f"stream {stream} reads block B, which is not drawn"
            for bit in range(shift, shift + bits):
                assert (block, word, bit) not in used, f"streams {stream} and {used[(block, word, bit)]} share a bit"
                used[(block, word, bit)] = stream
    # and the replay's context refuses a read of an undrawn block instead of inventing a value
    c = gr.Ctx(1, 0, 0, 4, has_b, image)
    if not has_b:
        with pytest.raises(RuntimeError):
            c.bits(4)


def test_enums_are_the_librarys():
    from optrace_amd import _capi
    for name in [n for n in dir(gr) if n.split("_")[0] in ("SRC", "DIV", "OR", "POL", "SPEC")]:
        assert getattr(gr, name) == getattr(_capi, name), name


@pytest.mark.parametrize("n", [2, 3, 4, 5, 8, 15, 16, 17, 1000, 4096, 1 << 15, (1 << 16) - 1])
def test_grid_row_by_reciprocal_equals_divmod(n):
    """strat_rect finds the row of stratum k as (uint32)((k + 0.5) * inv_n2) with two fix-ups; for every k of the grid that
    is divmod(k, n2).  The half keeps the product 0.5 / n2 away from every integer, far more than the rounding of inv_n2 moves
    it: the first guess is already the row, and the fix-ups never fire (dropping one changes no ray)."""
    n2, inv_n, inv_n2 = gr.range_constants(n)
    assert n2 * n2 <= n < (n2 + 1) * (n2 + 1) and inv_n == 1.0 / n and inv_n2 == 1.0 / n2
    k = np.arange(n2 * n2, dtype=np.int64)
    guess = ((k.astype(np.float64) + 0.5) * inv_n2).astype(np.int64)
    iy = guess - (guess * n2 > k)
    iy = iy + ((iy + 1) * n2 <= k)
    want_y, want_x = np.divmod(k, n2)
    assert np.array_equal(guess, want_y)
    assert np.array_equal(iy, want_y) and np.array_equal(k - iy * n2, want_x)


def test_range_ids_follow_the_stable_sort():
    ranges = [(0, 10, 5, 0.), (1, 0, 10, 0.), (2, 10, 0, 0.), (0, 15, 0, 0.), (1, 15, 3, 0.)]
    assert [r[:3] for r in gr.range_ids(ranges)] == [(1, 0, 10), (2, 10, 0), (0, 10, 5), (0, 15, 0), (1, 15, 3)]


def test_longdouble_carries_the_uniform_variable():
    """k + bits * 2^-32 needs up to 21 + 32 bits here and must be exact: the replay relies on a 64-bit mantissa."""
    assert np.finfo(np.longdouble).nmant >= 63
    c = gr.Ctx(9, 0, 0, 1 << 20, True, False)
    k = c.stratum(gr.ST_POS)
    u = c.plus(gr.dither_slot(gr.ST_POS), k)
    back = (u - k.astype(np.longdouble)) * np.longdouble(2.0 ** 32)
    assert np.array_equal(back.astype(np.uint64), c.bits(4)[0])


def test_erf_and_its_inverse_in_longdouble():
    import math
    x = np.linspace(-3, 3, 61)
    assert np.abs(gr.erf_ld(x).astype(np.float64) - np.array([math.erf(v) for v in x])).max() < 4e-16
    t = np.linspace(-0.999, 0.999, 101).astype(np.longdouble)
    assert np.abs(gr.erf_ld(gr.erfinv_ld(t)) - t).max() < 1e-18
