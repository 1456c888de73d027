"""The bucket-id arithmetic of the sort (tests/sort_reference.py restates sort_build_kernel / bucket_scatter_kernel in
numpy) on the CPU: ids inside their bit widths always give a bucket id below nb; ids beyond them ("wild") give, by
shape and kind, either an index far outside the LDS histogram and the bucket offsets or one that wraps back below nb;
`fits`, the predicate the build kernel keeps such entries out with, is false for exactly the wild entries.  This is the
evidence for the hazard the predicate closes, obtained without running a wild id through a kernel.  The host routes of
the shapes the GPU tests use (tests/test_sort_device_routes_gpu.py) are pinned as literals."""
import numpy as np
import pytest

from tests import sort_reference as R

OFF = (0, ) * 9
# (E, M, N, value_bytes, coalesce): route, key_bits, idx_bits, packed, passes, ride, tiles,
#                                   on, levels, strip, bits, bits1, kshift, shift, nb, cap
ROUTES = [
    # full words at the first E with a bucket plan; a 4-byte value rides (12-byte entries: smaller tiles and buckets)
    ((1 << 17, 300, 500, 0, 0), (2, 18, 17, 1, 3, 0, 16, 1, 1, 0, 6, 6, 0, 29, 64, 8192)),
    ((1 << 17, 300, 500, 0, 1), (2, 18, 17, 1, 3, 0, 16, 1, 1, 0, 6, 6, 0, 29, 64, 8192)),
    ((1 << 17, 300, 500, 4, 0), (2, 18, 17, 1, 3, 1, 22, 1, 1, 0, 6, 6, 0, 29, 64, 6144)),
    ((1 << 17, 300, 500, 4, 1), (2, 18, 17, 1, 3, 1, 22, 1, 1, 0, 6, 6, 0, 29, 64, 6144)),
    # strip, one level: 44 + 21 bits do not fit a word
    (((1 << 20) + 1, 1 << 22, 1 << 22, 0, 0), (2, 44, 21, 0, 6, 0, 171, 1, 1, 1, 8, 8, 36, 57, 256, 8192)),
    (((1 << 20) + 1, 1 << 22, 1 << 22, 0, 1), (2, 44, 21, 0, 6, 0, 171, 1, 1, 1, 8, 8, 36, 57, 256, 8192)),
    (((1 << 20) + 1, 1 << 22, 1 << 22, 4, 0), (2, 44, 21, 0, 6, 0, 171, 1, 1, 1, 8, 8, 36, 57, 256, 6144)),
    (((1 << 20) + 1, 1 << 22, 1 << 22, 4, 1), (2, 44, 21, 0, 6, 0, 171, 1, 1, 1, 8, 8, 36, 57, 256, 6144)),
    # the rest of the census
    (((1 << 17) + 1, 300, 500, 0, 0), (2, 18, 18, 1, 3, 0, 17, 1, 1, 0, 6, 6, 0, 30, 64, 8192)),
    ((1 << 17, 9000, 7000, 0, 0), (2, 27, 17, 1, 4, 0, 16, 1, 1, 0, 6, 6, 0, 38, 64, 8192)),
    (((1 << 17) + 1, 9000, 7000, 4, 1), (2, 27, 18, 1, 4, 1, 22, 1, 1, 0, 6, 6, 0, 39, 64, 6144)),
    ((1 << 20, 16, 16, 0, 1), (2, 8, 20, 1, 1, 0, 128, 1, 1, 0, 8, 8, 0, 20, 256, 8192)),
    ((500000, 1 << 20, 1 << 20, 0, 0), (2, 40, 19, 1, 5, 0, 62, 1, 1, 0, 7, 7, 0, 52, 128, 8192)),
    ((500000, 1 << 20, 1 << 20, 4, 1), (2, 40, 19, 1, 5, 1, 82, 1, 1, 0, 7, 7, 0, 52, 128, 6144)),
    (((1 << 17) - 1, 300, 500, 4, 1), (2, 18, 17, 1, 3, 1, 22) + OFF),
    # packed words of exactly 64 bits whose sixth digit reaches past them (8 * 6 + 17 > 64), passes only
    (((1 << 17) - 1, 1 << 24, 1 << 23, 0, 0), (2, 47, 17, 1, 6, 0, 16) + OFF),
]


@pytest.mark.parametrize('case', range(len(ROUTES)))
def test_host_routes_of_the_device_route_cases(case):
    args, want = ROUTES[case]
    got = R.route(*args)
    assert {f: got[f] for f in R.FIELDS} == dict(zip(R.FIELDS, want)), args


def test_census_agrees_with_the_host_plan():
    for c in R.census():
        for vb in (0, 4, 8):
            for co in (0, 1):
                assert R.route(c.E, c.M, c.N, vb, co)['on'] == c.on, (c, vb, co)
        assert c.E <= 1100000


def _plans(c):
    return [R.route(c.E, c.M, c.N, vb, co) for vb in (0, 4) for co in (0, 1)]


@pytest.mark.parametrize('c', [c for c in R.census() if c.on], ids=lambda c: c.name)
def test_in_range_ids_stay_below_nb(c):
    row, col = R.make_input(c)
    for rt in _plans(c):
        b = R.bucket_ids(row, col, c.E, rt)
        assert b.min() >= 0 and b.max() < rt['nb']
        assert np.array_equal(b, R.bucket_ids(row, col, c.E, rt, 'scatter'))  # both kernels: the same id
        assert R.fits(row, col, rt).all()


@pytest.mark.parametrize('c', [c for c in R.census() if c.on and c.M & (c.M - 1)], ids=lambda c: c.name)
def test_out_of_range_ids_inside_the_bit_width_stay_below_nb(c):
    """Row M .. 2^row_bits - 1 and col N .. 2^col_bits - 1 (300 .. 511 of 300): not wild, an ordinary bucket id."""
    row, col = R.make_input(c)
    rng = np.random.default_rng(3)
    at = rng.permutation(c.E)[:c.E // 50]
    row[at[::2]] = rng.integers(c.M, 1 << R.bits_for(c.M), at[::2].size)
    col[at[1::2]] = rng.integers(c.N, 1 << R.bits_for(c.N), at[1::2].size)
    row[0], col[c.E - 1] = c.M, (1 << R.bits_for(c.N)) - 1
    for rt in _plans(c):
        assert R.fits(row, col, rt).all()
        b = R.bucket_ids(row, col, c.E, rt)
        assert b.max() < rt['nb'] and np.array_equal(b, R.bucket_ids(row, col, c.E, rt, 'scatter'))


@pytest.mark.parametrize('shape', R.WILD_SHAPES, ids=lambda c: c.name)
@pytest.mark.parametrize('where', R.WHERE)
def test_wild_ids_leave_the_histogram_and_fits_names_exactly_them(shape, where):
    """The hazard, on the CPU: the id the kernels compute without `fits` for every wild kind.  R.HAZARD records, by shape
    and kind, whether it lies outside [0, nb) -- the row ids beyond the width (where the word still holds them) and every
    negative id do, by up to 2^32; a col bit that lands in the key's row bits, or bits shifted out of the 64-bit word,
    wrap to an ordinary id.  `fits` is false for exactly the planted entries in every case, and the entries it accepts
    have ids below nb."""
    row0, col0 = R.make_input(shape)
    at = R.wild_positions(shape.E, where)
    planted = np.zeros(shape.E, dtype=bool)
    planted[at] = True
    for name, which, bad in R.wild_kinds(shape.M, shape.N):
        row, col = row0.copy(), col0.copy()
        (row if which == 'row' else col)[at] = bad
        for rt in _plans(shape):
            f = R.fits(row, col, rt)
            assert np.array_equal(~f, planted), (name, 'fits must reject the wild entries and nothing else')
            b = R.bucket_ids(row, col, shape.E, rt)
            assert b[f].max() < rt['nb']
            assert np.array_equal(b[f], R.bucket_ids(row, col, shape.E, rt, 'scatter')[f])
            outside = b[planted] >= rt['nb']
            assert outside.all() == outside.any() == R.HAZARD[(shape.name, name)], (shape.name, name, b[planted][:4])
    # the kinds the contract is about leave the histogram on both shapes
    for s in R.WILD_SHAPES:
        for name in ('row_pow2', 'row_-1', 'col_-5'):
            assert R.HAZARD[(s.name, name)]


def test_a_share_of_every_wild_kind_at_once():
    """1 % of the entries wild, all kinds mixed: the entries `fits` accepts are the untouched ones, ids below nb."""
    for shape in R.WILD_SHAPES:
        row, col = R.make_input(shape)
        at = R.wild_positions(shape.E, 'percent')
        kinds = R.wild_kinds(shape.M, shape.N)
        for j, (name, which, bad) in enumerate(kinds):
            (row if which == 'row' else col)[at[j::len(kinds)]] = bad
        planted = np.zeros(shape.E, dtype=bool)
        planted[at] = True
        for rt in _plans(shape):
            f = R.fits(row, col, rt)
            assert np.array_equal(~f, planted)
            assert R.bucket_ids(row, col, shape.E, rt)[f].max() < rt['nb']
            assert (R.bucket_ids(row, col, shape.E, rt)[planted] >= rt['nb']).any()


def test_fits_at_a_width_of_zero_bits():
    """M = 1: row_bits = 0, only row 0 fits (a shift by the full width, never by 64)."""
    rt = R.route(200000, 1, 1 << 20)
    assert rt['key_bits'] == rt['col_bits'] == 20
    row = np.array([0, 1, -1, 0, 0])
    col = np.array([5, 5, 5, 1 << 20, (1 << 20) - 1])
    assert R.fits(row, col, rt).tolist() == [True, False, False, False, True]


def test_pass_digits_come_from_the_word():
    """The one-sweep passes on any word: the build kernel histograms the bits the passes read.  For ids inside their
    widths the whole key says the same; a wild id in a 64-bit packed word whose last digit reaches past bit 64 does not
    (the evidence for taking the histogram from the word), and wherever the word holds every digit the three agree."""
    c = R.WILD_PASSES_ONLY
    rt = R.route(c.E, c.M, c.N)
    assert rt['packed'] == 1 and 8 * rt['passes'] + rt['idx_bits'] > 64
    row, col = R.make_input(c)
    assert np.array_equal(R.pass_digits(row, col, c.E, rt), R.pass_digits(row, col, c.E, rt, 'build_full_key'))
    for name, which, bad in R.wild_kinds(c.M, c.N):
        r, k = row.copy(), col.copy()
        (r if which == 'row' else k)[R.wild_positions(c.E, 'percent')] = bad
        want = R.pass_digits(r, k, c.E, rt)
        assert np.array_equal(R.pass_digits(r, k, c.E, rt, 'build'), want), name
        differs = not np.array_equal(R.pass_digits(r, k, c.E, rt, 'build_full_key'), want)
        assert differs == (name in ('row_pow2', 'row_-1', 'col_-5')), name
    for shape in R.WILD_SHAPES:   # 24 + 17 bits / pairs: every digit lies inside the word
        rt = R.route(shape.E, shape.M, shape.N)
        row, col = R.make_input(shape)
        row[::100] = -1
        want = R.pass_digits(row, col, shape.E, rt)
        assert np.array_equal(R.pass_digits(row, col, shape.E, rt, 'build'), want)
        assert np.array_equal(R.pass_digits(row, col, shape.E, rt, 'build_full_key'), want)
