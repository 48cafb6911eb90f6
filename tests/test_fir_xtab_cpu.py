"""The identity behind eav_eegnet_fir_wgrad_fft_xtab and the layout of its tables, in float64 numpy (tests/fir_xtab_ref.py):
the train-mode firstConv weight gradient, whose dy holds y1 = firstConv(x), equals a combination of the eval-mode sum over
the raw gradient and two per-trial functions of x alone.

Shapes, each small enough for the direct K x K x C x S sums: K odd, K even, S < K, K = S (the padded row is then twice the
record), and a batch drawn from a larger data set with repeated and permuted indices."""
import numpy as np
import pytest

from tests import fir_xtab_ref as R

# (N, C, S, K, idx)
CASES = [(2, 3, 40, 7, None), (2, 3, 40, 8, None), (2, 2, 5, 9, None), (1, 2, 300, 300, None),
         (5, 3, 33, 6, (4, 1, 1, 0, 4, 2))]


def case(N, C, S, K, idx):
    rng = np.random.default_rng(1000 * K + S)
    x = rng.standard_normal((N, C, S)).astype(np.float32)
    w = rng.uniform(-0.1, 0.1, (8, K)).astype(np.float32)
    B = N if idx is None else len(idx)
    g = rng.standard_normal((B, 8, C, S)).astype(np.float32)
    mean, m1, m2 = (rng.uniform(-0.2, 0.2, 8) for _ in range(3))
    invstd, scale = rng.uniform(0.5, 2.0, 8), rng.uniform(0.5, 1.5, 8)
    return x, w, g, (mean, invstd, scale, m1, m2)


@pytest.mark.parametrize("N,C,S,K,idx", CASES)
def test_weight_gradient_from_tables_equals_the_direct_form(N, C, S, K, idx):
    x, w, g, bn = case(N, C, S, K, idx)
    xb = x if idx is None else x[list(idx)]
    ref = R.wgrad_direct(xb, R.conv_same(xb, w), g, *bn, K)
    A, X1 = R.tables_direct(x, K)
    got = R.wgrad_from_tables(x, w, g, *bn, A, X1, idx)
    assert np.abs(got - ref).max() <= 1e-12 * np.abs(ref).max()


@pytest.mark.parametrize("N,C,S,K,idx", CASES)
def test_autocorrelation_plus_edges_equals_the_direct_tables(N, C, S, K, idx):
    x = case(N, C, S, K, idx)[0]
    A, X1 = R.tables_direct(x, K)
    A2, X12 = R.tables_autocorr(x, K)
    assert np.abs(A2 - A).max() <= 1e-12 * np.abs(A).max()
    assert np.abs(X12 - X1).max() <= 1e-12 * max(np.abs(X1).max(), 1.0)
    assert (A2 == A2.transpose(0, 2, 1)).all()


def test_table_layout():
    x = case(2, 3, 40, 7, None)[0]
    A, X1 = R.tables_direct(x, 7)
    tab = R.flat_tables(A, X1)
    assert tab.shape == (2, 7 * 7 + 7)
    assert tab[1, 3 * 7 + 5] == A[1, 3, 5] and tab[1, 49 + 2] == X1[1, 2]
    # A_b[j,k] = sum over the electrodes and the S window positions of xp[t+j] xp[t+k]
    xp = R.padded(x, 7)
    assert abs(A[0, 2, 6] - sum(xp[0, c, t + 2] * xp[0, c, t + 6] for c in range(3) for t in range(40))) < 1e-9
    assert abs(X1[0, 4] - sum(xp[0, c, t + 4] for c in range(3) for t in range(40))) < 1e-9
