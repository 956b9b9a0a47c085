"""Shape edges of the frequency-precompute kernels (sigdots, sbgemm,
sigdots_block) against the longdouble oracle (tests/hpref.py).

Same tolerance rule as tests/test_solve_templates.py: normwise per
plane, within ``16 * max(base, 64 eps)``, ``base`` being the error of a
numpy fp64 evaluation of the same formula against the oracle.  The
fp64 evaluation rounds the argument 2 pi f t as the kernels do, so a
large argument raises ``base`` and the bound together; the oracle
reduces the argument exactly."""

import numpy as np
import pytest
import torch

import hpref

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def _ext():
    from fastfp_amd import ops

    ops.require_hip()
    from fastfp_amd.ops import _fastfp_hip

    return _fastfp_hip


def _t(a, dtype=np.float64):
    return torch.tensor(np.asarray(a, dtype=dtype), device=DEV)


def _np(t):
    return t.detach().cpu().numpy()


def _check(label, got, ref, base64):
    err, tol = hpref.report(label, hpref.nerr(got, ref),
                            hpref.nerr(base64, ref))
    assert err <= tol, f"{label}: {err:.3e} > tol {tol:.3e}"


def _check_dots(tag, got, ref, base):
    names = (["s.Ns", "c.Nc", "s.Nc"], ["s.Nr", "c.Nr"])
    for k in range(2):
        g = _np(got[k])
        assert g.shape == ref[k].shape
        for i, name in enumerate(names[k]):
            _check(f"{tag} {name}", g[i], ref[k][i], base[k][i])


# ----------------------------------------------------------------------
# sigdots
# ----------------------------------------------------------------------
def _check_sigdots(ntoa, F, offset=0.0):
    ext = _ext()
    rng = np.random.default_rng([1, ntoa, F])
    toas, ninv, nr, freqs = hpref.gen_trig(rng, ntoa, F, offset)
    got = ext.sigdots(_t(toas), _t(ninv), _t(nr), _t(freqs))
    ref = hpref.trig_dots(toas, ninv, nr, freqs)
    base = hpref.trig_dots(toas, ninv, nr, freqs, np.float64)
    _check_dots(f"sigdots ntoa={ntoa} F={F} off={offset:g}", got, ref, base)


@pytest.mark.parametrize("F", [1, 5])
@pytest.mark.parametrize("ntoa", [1, 63, 256, 257, 1000])
def test_sigdots_shapes(ntoa, F):
    """One TOA, less than a wave, exactly and one past the 256-thread
    block, and several strides."""
    _check_sigdots(ntoa, F)


def test_sigdots_present_day_toas():
    """TOAs offset by 4.6e9 s (a present-day MJD in seconds):
    |2 pi f t| ~ 1.5e3, against arguments below 130 everywhere else."""
    _check_sigdots(1000, 5, offset=4.6e9)


# ----------------------------------------------------------------------
# sbgemm through ops.freq_precompute
# ----------------------------------------------------------------------
def _check_rhs(tag, RHS, m, F, TNr, ref, base):
    RHS = _np(RHS)
    mp = max(16, (m + 15) // 16 * 16)
    assert RHS.shape == (mp, 2 * F + 1)
    _check(f"{tag} sin", RHS[:m, 0:-1:2], ref[:, 0::2], base[:, 0::2])
    _check(f"{tag} cos", RHS[:m, 1:-1:2], ref[:, 1::2], base[:, 1::2])
    assert (RHS[m:] == 0).all(), f"{tag}: pad rows"
    assert (RHS[:m, -1] == TNr).all(), f"{tag}: u column"


@pytest.mark.parametrize("F,ntoa,m", [
    (1, 5, 1), (32, 16, 16), (33, 17, 64), (5, 257, 65), (5, 300, 128),
    (5, 300, 129), (40, 1793, 37)])
def test_freq_precompute_shapes(F, ntoa, m):
    """ntoa below one K panel; the 64-column tile edge at F = 32 / 33;
    a partly filled second row half (mp = 80); a second M tile of 16
    rows (mp = 144); ksplit 1, 2 and 8 with K chunks that are no
    multiple of 16."""
    from fastfp_amd import ops

    rng = np.random.default_rng([2, F, ntoa, m])
    toas, ninv, nr, freqs = hpref.gen_trig(rng, ntoa, F)
    nvec = 1.0 / ninv
    ninv = 1.0 / nvec  # what the op forms on the device from Nvec
    r = rng.normal(0, 1e-6, ntoa)
    T = rng.normal(size=(ntoa, m))
    TNr = rng.normal(size=m)
    RHS, sNs, sNr = ops.freq_precompute(_t(toas), _t(nvec), _t(r), _t(T),
                                        _t(TNr), _t(freqs))
    tag = f"sbgemm F={F} ntoa={ntoa} m={m}"
    _check_rhs(tag, RHS, m, F, TNr,
               hpref.basis_rhs(T, ninv, toas, freqs),
               hpref.basis_rhs(T, ninv, toas, freqs, np.float64))
    nrv = r / nvec
    _check_dots(tag, (sNs, sNr), hpref.trig_dots(toas, ninv, nrv, freqs),
                hpref.trig_dots(toas, ninv, nrv, freqs, np.float64))


# ----------------------------------------------------------------------
# sigdots_block, directly and through ops.freq_precompute_block
# ----------------------------------------------------------------------
SIZES = [1, 1, 2, 40, 300] + [1, 2, 3] * 100


def _block_inputs(sizes, F, seed):
    rng = np.random.default_rng([3, seed])
    uvec, beta, offsets, sizes = hpref.gen_blocks(rng, sizes)
    toas, _, nr, freqs = hpref.gen_trig(rng, int(sizes.sum()), F)
    return toas, uvec, nr, freqs, beta, offsets, sizes


def _check_sigdots_block():
    ext = _ext()
    args = _block_inputs(SIZES, 3, 0)
    toas, uvec, nr, freqs, beta, offsets, sizes = args
    assert len(sizes) == 305 and sizes.max() == 300
    assert (beta[sizes == 1] == 0).all() and (beta[sizes > 1] > 0).all()
    got = ext.sigdots_block(_t(toas), _t(uvec), _t(nr), _t(freqs), _t(beta),
                            _t(offsets, np.int64), _t(sizes, np.int64))
    _check_dots("sigdots_block", got, hpref.block_dots(*args),
                hpref.block_dots(*args, np.float64))


def test_sigdots_block_direct():
    """305 blocks (more than blockDim), one of 300 TOAs (longer than
    blockDim), beta = 0 on the singletons, F = 3."""
    _check_sigdots_block()


class _Blocks:
    """The part of BlockNoise that ops.freq_precompute_block reads."""

    def __init__(self, uvec, beta, offsets, sizes):
        self._t = dict(uvec=_t(uvec), beta=_t(beta),
                       offsets=_t(offsets, np.int64),
                       sizes=_t(sizes, np.int64))

    def tensors(self, device):
        return self._t


def test_freq_precompute_block_unit_weights():
    """The ECORR entry point: sbgemm with V in place of T and unit
    weights (m = 129: two M tiles), sigdots_block for the dots."""
    from fastfp_amd import ops

    F, m = 5, 129
    args = _block_inputs([1, 2, 3] * 50, F, 1)
    toas, uvec, nr, freqs, beta, offsets, sizes = args
    ntoa = len(toas)
    rng = np.random.default_rng(4)
    V = rng.normal(size=(ntoa, m)) * 1e12
    TNr = rng.normal(size=m)
    RHS, sNs, sNr = ops.freq_precompute_block(
        _t(toas), _Blocks(uvec, beta, offsets, sizes), _t(nr), _t(V),
        _t(TNr), _t(freqs))
    ones = np.ones(ntoa)
    _check_rhs("sbgemm unit-weight", RHS, m, F, TNr,
               hpref.basis_rhs(V, ones, toas, freqs),
               hpref.basis_rhs(V, ones, toas, freqs, np.float64))
    _check_dots("sigdots_block via op", (sNs, sNr), hpref.block_dots(*args),
                hpref.block_dots(*args, np.float64))


# ----------------------------------------------------------------------
# host side: empty launches return
# ----------------------------------------------------------------------
def _empty(*shape):
    return torch.empty(shape, dtype=torch.float64, device=DEV)


def test_empty_frequencies_or_toas_launch_nothing():
    """F = 0 or ntoa = 0: correctly shaped (empty, or empty-sum zero)
    outputs, no launch, no error left behind, and the next valid call
    passes its oracle check."""
    from fastfp_amd import ops

    ext = _ext()
    toas, ninv, nr, _ = hpref.gen_trig(np.random.default_rng(9), 20, 1)
    f0 = _empty(0)

    sNs, sNr = ext.sigdots(_t(toas), _t(ninv), _t(nr), f0)
    assert sNs.shape == (3, 0) and sNr.shape == (2, 0)
    sNs, sNr = ext.sigdots(f0, f0, f0, _t([3e-9, 4e-9]))
    assert sNs.shape == (3, 2) and sNr.shape == (2, 2)
    assert (sNs == 0).all() and (sNr == 0).all()
    torch.cuda.synchronize()
    _check_sigdots(63, 1)

    i0 = torch.empty(0, dtype=torch.int64, device=DEV)
    one = _t([1.0] * 20)
    off, siz = _t([0], np.int64), _t([20], np.int64)
    sNs, sNr = ext.sigdots_block(_t(toas), _t(ninv), _t(nr), f0, one[:1],
                                 off, siz)
    assert sNs.shape == (3, 0) and sNr.shape == (2, 0)
    sNs, sNr = ext.sigdots_block(f0, f0, f0, _t([3e-9]), f0, i0, i0)
    assert sNs.shape == (3, 1) and (sNs == 0).all() and (sNr == 0).all()
    torch.cuda.synchronize()
    _check_sigdots_block()

    # sbgemm with no frequencies: RHS is just the u column
    T = np.random.default_rng(10).normal(size=(20, 3))
    TNr = np.array([1.0, 2.0, 3.0])
    RHS, sNs, sNr = ops.freq_precompute(_t(toas), _t(1.0 / ninv), _t(nr),
                                        _t(T), _t(TNr), f0)
    assert RHS.shape == (16, 1) and sNs.shape == (3, 0)
    assert (_np(RHS)[:3, 0] == TNr).all() and (_np(RHS)[3:] == 0).all()
    torch.cuda.synchronize()
    test_freq_precompute_shapes(1, 5, 1)
