"""Host: tests/rows_order.py, the numpy restatement of the device's two-stage row sums, is a sum - exact where float64 is exact, and
within the bound of any float64 summation order elsewhere (N 2^-53 sum |t|) of the correctly rounded sum."""
import math

import numpy as np
import pytest

import rows_order as ro

FORMS = {"workgroup": ro.sum_workgroup, "wave": ro.sum_wave}


def _sizes(P):
    c = ro.chunk(P)
    return [1, 3, c - 1, c + 1, 2 * c + 3, 257 * c + 5]


@pytest.mark.parametrize("P", [2, 4])
@pytest.mark.parametrize("form", sorted(FORMS))
def test_integer_terms_sum_exactly(form, P):
    for N in _sizes(P):
        t = np.random.RandomState(N % 1000 + P).randint(-1000, 1001, size=(2, N)).astype(np.float64)      # |sum| < 2^31: exact in any order
        got = FORMS[form](t, P)
        assert got.shape == (2,) and np.array_equal(got, t.astype(np.int64).sum(1).astype(np.float64)), N


@pytest.mark.parametrize("P", [2, 4])
@pytest.mark.parametrize("form", sorted(FORMS))
def test_random_terms_within_the_bound_of_a_float64_sum(form, P):
    for N in _sizes(P):
        t = np.random.RandomState(7 * P + N % 1000).randn(2, N) * np.exp(np.random.RandomState(N % 999).randn(2, N))
        got = FORMS[form](t, P)
        for s in range(2):
            err, bound = abs(got[s] - math.fsum(t[s])), N * 2.0 ** -53 * math.fsum(np.abs(t[s]))
            assert err <= bound, (N, s, err, bound)


def test_every_element_is_counted_once_by_the_thread_that_owns_it():
    """A single 1.0 at any position sums to 1.0, and the chunk it lands in is e // CHUNK."""
    for P in (2, 4):
        c = ro.chunk(P)
        N = 2 * c + 3
        for e in (0, 3, 4, 1023, 1024, c - 1, c, 2 * c - 1, 2 * c, N - 1):
            t = np.zeros((1, N))
            t[0, e] = 1.0
            parts = ro.chunk_sums(t, P)
            assert parts.shape == (1, 3) and parts[0, e // c] == 1.0 and parts.sum() == 1.0, (P, e)
