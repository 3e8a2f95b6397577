"""tests/dust_model.py against itself: the vectorised recurrence (mask) equals the literal reading of the definition (mask_brute,
every interval and every sub-interval), and the values the definition pins.  No device."""
import numpy as np
import pytest

from tests import dust_model as dm


def _cases():
    rng = np.random.default_rng(2006)
    out = []
    lengths = list(range(1, 131)) + [int(x) for x in rng.integers(1, 131, size=90)]
    for j, n in enumerate(lengths):
        k = j % 10
        if k == 0:
            s = dm.iid(rng, n)
        elif k == 1:
            s = dm.biased(rng, n)
        elif k <= 4:
            s = dm.periodic(rng, n, 1 + (j // 10) % 7)
        elif k == 5:
            s = dm.mixed(rng, n, n_share=0.03)
        elif k == 6:
            s = dm.mixed(rng, n, lower_share=0.5)
        elif k == 7:
            s = dm.mixed(rng, n, flank=4, longest=30)
        elif k == 8:
            s = dm.mixed(rng, n, n_share=0.02, lower_share=0.3)
        else:
            s = dm.homopolymer(rng, n)
        out.append(s)
    return out


def test_recurrence_equals_the_definition():
    cases = _cases()
    assert len(cases) == 220 and {len(s) for s in cases} >= set(range(1, 131))
    masked = 0
    for s in cases:
        a, b = dm.mask_bool(s), dm.mask_brute_bool(s)
        assert np.array_equal(a, b), s
        masked += int(a.sum())
    total = sum(len(s) for s in cases)
    assert 0.2 * total < masked < 0.95 * total  # (neither all clear nor all masked: the comparison shows something)


A6, A7 = b"A" * 6, b"A" * 7


@pytest.mark.parametrize("f", [dm.mask, dm.mask_brute])
def test_pinned_values(f):
    assert f(A6) == A6
    assert f(A7) == b"N" * 7
    assert f(b"AC" * 6) == b"N" * 12
    assert f(b"ACGT" * 20) == b"N" * 80
    assert f(b"a" * 7) == b"N" * 7 and f(b"aAaAaAa") == b"N" * 7          # case carries no meaning
    assert f(A6 + b"N" + A6) == A6 + b"N" + A6                             # an N in the middle of A x 12: two runs of 6
    assert f(A6 + b"-" + A7) == A6 + b"-" + b"N" * 7                       # any other byte ends a run and stays
    assert f(b"") == b"" and f(b"A") == b"A" and f(b"NNN") == b"NNN"


def test_records_are_masked_apart():
    """AAAA ending one record and AAAA starting the next: nothing masked, though AAAAAAAA in one record is"""
    a, b = b"CGTCAGTAAAA", b"AAAATGCAGTC"
    assert dm.mask(a) == a and dm.mask(b) == b
    joined = dm.mask(a + b)
    assert joined[7:15] == b"N" * 8 and dm.masked_count(a + b) == 8


def test_iid_masks_little():
    rng = np.random.default_rng(3)
    s = dm.iid(rng, 200_000)
    share = dm.masked_count(s) / len(s)
    assert 0.0002 < share < 0.005, share


def test_generators():
    rng = np.random.default_rng(4)
    assert len(dm.mixed(rng, 777, n_share=0.05, lower_share=0.5)) == 777
    s, where = dm.plant(rng, dm.iid(rng, 5000), range(5, 60))
    assert len(s) == 5000 and len(where) > 30
    for period in range(2, 8):
        p = dm.periodic(rng, 50, period)
        assert p[:50 - period] == p[period:]
