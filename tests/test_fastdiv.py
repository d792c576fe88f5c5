"""The path kernel's multiply-shift divider (tmpt_internal.h FastDiv: the
frame's width and a unit's block counts as {mul, shift}), through the host's
statement of the device's expression (tm.fastdiv, no GPU): x // d for every
multiple of d below 2^31 with its two neighbours -- where a quotient steps --
and 10^6 seeded random dividends, against Python's integer division."""
import numpy as np
import pytest

import toymeshpathtracer_amd as tm

LIMIT = 1 << 31
DIVISORS = [1, 2, 3, 7, 8, 64, 1279, 1280, 1920, 3840, 65535, (1 << 16) + 1, (1 << 31) - 1]
CHUNK = 1 << 24  # dividends per call


def check(d, x):
    """x: uint32 dividends below 2^31; the expected quotients are exact integer
    division (numpy's // on unsigned integers is Python's // there)."""
    got, _ = tm.fastdiv(d, x)
    want = x // np.uint32(d)
    bad = np.nonzero(got != want)[0]
    assert bad.size == 0, f"d={d}: {bad.size} wrong, first x={x[bad[:4]]} got={got[bad[:4]]} want={want[bad[:4]]}"


@pytest.mark.parametrize("d", DIVISORS)
def test_pair_fits_and_reproduces_the_definition(d):
    _, (mul, shift) = tm.fastdiv(d, np.zeros(0, np.uint32))
    assert shift == (d - 1).bit_length() and mul == -(-(1 << (31 + shift)) // d) and mul < 1 << 32
    for x in (0, 1, d - 1, d, d + 1, LIMIT - 1):
        if 0 <= x < LIMIT:
            assert ((2 * x * mul) >> 32) >> shift == x // d  # the device's expression, in Python integers
            assert int(tm.fastdiv(d, np.array([x], np.uint32))[0][0]) == x // d


@pytest.mark.parametrize("d", DIVISORS)
def test_every_multiple_and_its_neighbours(d):
    if d <= 3:  # the multiples' neighbourhoods cover every dividend
        for lo in range(0, LIMIT, CHUNK):
            check(d, np.arange(lo, min(lo + CHUNK, LIMIT), dtype=np.uint32))
        return
    n_mult = (LIMIT - 1) // d + 1  # multiples k * d < 2^31, k = 0 ..
    per = CHUNK // 3
    for k0 in range(0, n_mult, per):
        m = np.arange(k0, min(k0 + per, n_mult), dtype=np.uint32) * np.uint32(d)  # < 2^31: no wrap
        check(d, m)
        check(d, m[1 if k0 == 0 else 0:] - np.uint32(1))
        up = m + np.uint32(1)  # only the last multiple's neighbour can reach 2^31
        check(d, up[up < LIMIT])


@pytest.mark.parametrize("d", DIVISORS)
def test_random_dividends(d):
    rng = np.random.default_rng(0xD1F + d)
    check(d, rng.integers(0, LIMIT, size=1_000_000, dtype=np.uint32))
    check(d, np.array([0, 1, LIMIT - 2, LIMIT - 1], np.uint32))


def test_domain_is_checked():
    for d in (0, 1 << 31):
        with pytest.raises(tm.TmptError, match="divisor out of range"):
            tm.fastdiv(d, np.zeros(1, np.uint32))
    with pytest.raises(tm.TmptError, match="dividend out of range"):
        tm.fastdiv(3, np.array([LIMIT], np.uint32))
