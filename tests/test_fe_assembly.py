"""The host Fe assembly exists once: ``_assemble_fe`` is the one-draw form
of ``_assemble_fe_draws`` and ``_null_max_host`` builds M from the same
moments.  Bitwise guards against the copies growing back."""

import numpy as np
import pytest

from fastfp_amd import festat
from fastfp_amd.festat import (
    _assemble_fe,
    _assemble_fe_draws,
    _null_max_host,
)


def _inputs(P, D, F, seed=11):
    """Positive-definite per-pulsar blocks, random data products and one
    random sky row."""
    rng = np.random.default_rng(seed)
    prods = np.empty((P, D, 5, F))
    prods[:, :, 0:2] = rng.uniform(1.0, 2.0, (P, D, 2, F))
    prods[:, :, 2] = 0.1 * rng.normal(size=(P, D, F))
    prods[:, :, 3:] = rng.normal(size=(P, D, 2, F))
    return prods, rng.normal(size=P), rng.normal(size=P)


SHAPES = [(3, 1, 1), (5, 3, 7), (248, 2, 33)]


@pytest.mark.parametrize("P,D,F", SHAPES)
def test_one_draw_form_is_the_batched_assembly(P, D, F):
    prods, fplus, fcross = _inputs(P, D, F)
    fe = _assemble_fe_draws(prods, fplus, fcross)
    fe2, amps = _assemble_fe_draws(prods, fplus, fcross, amplitudes=True)
    assert fe.shape == (D, F) and amps.shape == (D, F, 4)
    np.testing.assert_array_equal(fe, fe2)
    for d in range(D):
        one = _assemble_fe(prods[:, d], fplus, fcross)
        one2, a = _assemble_fe(prods[:, d], fplus, fcross, amplitudes=True)
        assert one.shape == (F,) and a.shape == (F, 4)
        np.testing.assert_array_equal(one, fe[d])
        np.testing.assert_array_equal(one2, fe[d])
        np.testing.assert_array_equal(a, amps[d])


@pytest.mark.parametrize("P,D,F", SHAPES)
def test_null_reference_uses_the_assembly_moments(P, D, F, monkeypatch):
    """Both callers take M from ``festat._moments``, and what the null
    reference gets is, bit for bit, what the assembly gets and what the
    written-out sums over pulsars give."""
    prods, fplus, fcross = _inputs(P, D, F)
    seen = []
    inner = festat._moments

    def spy(*args):
        seen.append(inner(*args))
        return seen[-1]

    monkeypatch.setattr(festat, "_moments", spy)
    _assemble_fe_draws(prods, fplus, fcross)
    assert len(seen) == 1
    ant = np.stack([fplus, fcross], axis=1)[None]  # (1, P, 2)
    z = np.random.default_rng(5).standard_normal((D, F, P, 2, 3))
    _null_max_host(prods, ant, z)
    assert len(seen) == 2
    ss, cc, sc = prods[:, :, 0], prods[:, :, 1], prods[:, :, 2]
    fp2, fx2, fpx = fplus**2, fcross**2, fplus * fcross
    want = [(fp2, ss), (fp2, sc), (fpx, ss), (fpx, sc), (fp2, cc), (fpx, sc),
            (fpx, cc), (fx2, ss), (fx2, sc), (fx2, cc)]
    assert len(seen[0]) == len(seen[1]) == 10
    for a, b, (coeff, q) in zip(seen[0], seen[1], want):
        assert a.shape == (D, F)
        np.testing.assert_array_equal(a, b)
        np.testing.assert_array_equal(a, np.einsum("p,pdf->df", coeff, q))
