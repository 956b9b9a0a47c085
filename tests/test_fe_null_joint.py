"""Joint null of the Fe sky maximum across frequencies
(docs/DESIGN.md section 14): ``FpEngine.null_data``, the ``data`` form of
the sky layer, ``null_max(joint=True)``, ``global_false_alarm`` and the
``--null_joint`` CLI flag, on the CPU engine.

Tolerances.  ``null_data`` is compared with dense linear algebra on ``C =
diag(N) + T diag(phi) T^T``.  A backward-stable dense solve carries a
relative error of order ``cond(C) eps``; the engine forms the same
quantities as differences ``white - B^T Sigma^-1 (...)`` of operands no
larger than the un-cancelled ``S^T N^-1 S`` (or ``S^T N^-1 r``).  Every
bound below is therefore

    FACTOR * cond(C) * eps * max|un-cancelled operand|,   FACTOR = 50,

computed in the test from the dense matrices alone.  The priors are
chosen so that every basis column contributes to a TOA about as much
variance as the white noise does (``phi_k = a_k ntoa mean(N) /
|T_k|^2``, ``a_k`` in [0.5, 20]): ``cond(C)`` is then of order 1e3 (the
covariance test asserts it stays below 1e4).
"""

import json
import re

import numpy as np
import pytest
import torch

from fastfp_amd import (
    FastFe,
    FpEngine,
    NMFe,
    false_alarm_probability,
    global_false_alarm,
    initialize_pta,
    make_synthetic_pta,
)
from fastfp_amd.cli.run_fe import fibonacci_sky
from fastfp_amd.festat import _antenna_table, _null_max_host
from fastfp_amd.model import get_mats_fp, get_mats_nmfp

EPS = np.finfo(np.float64).eps
FACTOR = 50.0
F = 3
FREQS = np.linspace(5e-9, 4e-8, F)


def _noise(psrs):
    noise = {"gw_gamma": 13.0 / 3.0, "gw_log10_A": float(np.log10(2e-15))}
    for p in psrs:
        noise[f"{p.name}_red_noise_gamma"] = 4.0
        noise[f"{p.name}_red_noise_log10_A"] = -14.5
    return noise


def _array(npsr=2, seed=3):
    """``npsr`` pulsars of up to 40 TOAs, m = 4 + 2 * 4 = 12 basis columns."""
    psrs = make_synthetic_pta(npsr=npsr, ntoa=40, ntm=4, seed=seed)
    noise = _noise(psrs)
    pta = initialize_pta(psrs, noise, inc_cp=True, rn_comps=4, gwb_comps=4)
    _, Nvecs, Ts = get_mats_nmfp(pta, noise)
    Nvecs = [np.asarray(n, dtype=np.float64) for n in Nvecs]
    Ts = [np.asarray(T, dtype=np.float64) for T in Ts]
    assert all(T.shape[1] == 12 for T in Ts)
    return psrs, pta, noise, Nvecs, Ts


def _phi0(Nvec, T):
    """The prior at which a basis column adds mean(N) / ntoa per TOA."""
    return Nvec.mean() / (T * T).sum(axis=0)


def _priors(Nvecs, Ts, seed=5):
    rng = np.random.default_rng(seed)
    return [rng.uniform(0.5, 20.0, T.shape[1]) * T.shape[0] * _phi0(n, T)
            for n, T in zip(Nvecs, Ts)]


def _S(toas):
    """(ntoa, 2F), columns 2f = sin, 2f + 1 = cos: the rows of n."""
    arg = 2.0 * np.pi * FREQS[None, :] * np.asarray(toas)[:, None]
    S = np.empty((len(toas), 2 * F))
    S[:, 0::2], S[:, 1::2] = np.sin(arg), np.cos(arg)
    return S


def _engine(psrs, Nvecs, Ts):
    eng = FpEngine(psrs, Nvecs, Ts, device="cpu")
    eng.precompute(FREQS)
    return eng


def _identity_normals(Ts):
    """w = [I_ntoa | 0], u = [0 | I_m | 0], zero-padded to the common R =
    max ntoa + m: column j of n is the response to the j-th unit normal,
    so A A^T is the covariance of n."""
    R = max(T.shape[0] for T in Ts) + Ts[0].shape[1]
    w, u = [], []
    for T in Ts:
        ntoa, m = T.shape
        wp = torch.zeros((ntoa, R), dtype=torch.float64)
        wp[:, :ntoa] = torch.eye(ntoa, dtype=torch.float64)
        up = torch.zeros((m, R), dtype=torch.float64)
        up[:, ntoa:ntoa + m] = torch.eye(m, dtype=torch.float64)
        w.append(wp)
        u.append(up)
    return w, u, R


# ----------------------------------------------------------------------
# 1. the covariance of n is S^T C^-1 S, cross-frequency blocks included
# ----------------------------------------------------------------------
def test_null_data_covariance():
    psrs, pta, noise, Nvecs, Ts = _array()
    phis = _priors(Nvecs, Ts)
    phiinvs = [torch.as_tensor(1.0 / p) for p in phis]
    eng = _engine(psrs, Nvecs, Ts)
    w, u, R = _identity_normals(Ts)
    n = eng.null_data(phiinvs, R, w=w, u=u)
    assert n.shape == (1, F, 2, 2, R) and n.dtype == torch.float64
    prods = eng.sweep_products(phiinvs=phiinvs).numpy()  # (P, 5, F)
    for p, psr in enumerate(psrs):
        S = _S(psr.toas)
        C = np.diag(Nvecs[p]) + (Ts[p] * phis[p]) @ Ts[p].T
        cond = np.linalg.cond(C)
        G = S.T @ np.linalg.solve(C, S)
        scale = np.abs(S.T @ (S / Nvecs[p][:, None])).max()
        tol = FACTOR * cond * EPS * scale
        A = n[0, :, p].reshape(2 * F, R).numpy()
        got = A @ A.T
        err = np.abs(got - G).max()
        off = np.abs(G - np.kron(np.eye(F), np.ones((2, 2))) * G).max()
        print(f"pulsar {p}: cond(C) {cond:.3e}, |A A^T - S^T C^-1 S| "
              f"{err:.3e} (tol {tol:.3e}, scale {scale:.3e}), largest "
              f"cross-frequency entry {off:.3e}")
        assert cond < 1e4
        assert err <= tol
        # independent draws per frequency would make these blocks zero
        assert off > 1e3 * tol
        j = 2 * np.arange(F)
        for k, (a, b) in enumerate(((j, j), (j + 1, j + 1), (j, j + 1))):
            assert np.abs(got[a, b] - prods[p, k]).max() <= tol


# ----------------------------------------------------------------------
# 2. improper prior: phi^-1 = 0 on two timing-model columns
# ----------------------------------------------------------------------
def test_null_data_improper_prior():
    """Two columns with ``phi^-1 = 0`` against the dense ``C`` with ``phi
    = 1e12 ntoa phi0`` there.  ``cond`` of that ``C`` is ~1e14, so it is
    inverted through the Woodbury identity on those two columns alone, as
    tests/test_fe_null.py does: ``C = Cr + U diag(phi_u) U^T``, ``K =
    diag(1 / phi_u) + U^T Cr^-1 U``, with the dense ``Cr`` of the other
    ten columns solved directly.  The finite ``phi_u`` differs from the
    projection limit by ``K^-1 - K0^-1``, relative size at most ``|diag(1
    / phi_u)|_2 |K0^-1|_2`` to first order; the tolerance is the
    ``cond(Cr)`` bound of the module docstring plus twice that, both
    computed from the dense matrices."""
    psrs, pta, noise, Nvecs, Ts = _array()
    phis = _priors(Nvecs, Ts)
    eng = _engine(psrs, Nvecs, Ts)
    imp = np.zeros(12, dtype=bool)
    imp[[0, 2]] = True
    phiinvs = []
    for p in phis:
        pi = 1.0 / p
        pi[imp] = 0.0
        phiinvs.append(torch.as_tensor(pi))
    w, u, R = _identity_normals(Ts)
    n = eng.null_data(phiinvs, R, w=w, u=u)
    assert torch.isfinite(n).all()
    # the improper columns' normals reach nothing
    for p, T in enumerate(Ts):
        assert (n[:, :, p][..., T.shape[0] + np.flatnonzero(imp)] == 0).all()
    for p, psr in enumerate(psrs):
        S = _S(psr.toas)
        T = Ts[p]
        phi_u = 1e12 * T.shape[0] * _phi0(Nvecs[p], T)[imp]
        U = T[:, imp]
        Cr = np.diag(Nvecs[p]) + (T[:, ~imp] * phis[p][~imp]) @ T[:, ~imp].T
        cond = np.linalg.cond(Cr)
        X = np.linalg.solve(Cr, np.concatenate([S, U], axis=1))
        CS, CU = X[:, :2 * F], X[:, 2 * F:]
        K0 = U.T @ CU
        K = np.diag(1.0 / phi_u) + K0
        G = S.T @ CS - (S.T @ CU) @ np.linalg.solve(K, CU.T @ S)
        scale = np.abs(S.T @ (S / Nvecs[p][:, None])).max()
        limit = np.linalg.norm(np.diag(1.0 / phi_u), 2) \
            * np.linalg.norm(np.linalg.inv(K0), 2)
        tol = (FACTOR * cond * EPS + 2.0 * limit) * scale
        A = n[0, :, p].reshape(2 * F, R).numpy()
        err = np.abs(A @ A.T - G).max()
        print(f"pulsar {p}: cond(Cr) {cond:.3e}, limit term {limit:.3e}, "
              f"err {err:.3e} (tol {tol:.3e})")
        assert err <= tol


# ----------------------------------------------------------------------
# 3. one realisation through the existing data path
# ----------------------------------------------------------------------
def test_null_data_is_the_engine_data_path():
    psrs, pta, noise, Nvecs, Ts = _array()
    phis = _priors(Nvecs, Ts)
    phiinvs = [torch.as_tensor(1.0 / p) for p in phis]
    rng = np.random.default_rng(11)
    w = [rng.standard_normal((T.shape[0], 1)) for T in Ts]
    u = [rng.standard_normal((12, 1)) for _ in psrs]
    n = _engine(psrs, Nvecs, Ts).null_data(
        phiinvs, 1, w=[torch.as_tensor(x) for x in w],
        u=[torch.as_tensor(x) for x in u]).numpy()
    sim = make_synthetic_pta(npsr=2, ntoa=40, ntm=4, seed=3)
    for p, psr in enumerate(sim):
        assert np.array_equal(psr.toas, psrs[p].toas)
        psr.residuals = (np.sqrt(Nvecs[p]) * w[p][:, 0]
                         + Ts[p] @ (np.sqrt(phis[p]) * u[p][:, 0]))
    prods = _engine(sim, Nvecs, Ts).sweep_products(phiinvs=phiinvs).numpy()
    for p, psr in enumerate(sim):
        S = _S(psr.toas)
        C = np.diag(Nvecs[p]) + (Ts[p] * phis[p]) @ Ts[p].T
        scale = np.abs(S.T @ (psr.residuals / Nvecs[p])).max()
        tol = FACTOR * np.linalg.cond(C) * EPS * scale
        err = max(np.abs(prods[p, 3] - n[0, :, p, 0, 0]).max(),
                  np.abs(prods[p, 4] - n[0, :, p, 1, 0]).max())
        print(f"pulsar {p}: |(sr, cr) - n| {err:.3e} (tol {tol:.3e})")
        assert err <= tol


# ----------------------------------------------------------------------
# 4. the sky layer: chunking, joint=False, NMFe
# ----------------------------------------------------------------------
def _fixed(npsr=3):
    psrs, pta, noise, _, _ = _array(npsr=npsr, seed=7)
    Nvecs, Ts, sigmas = get_mats_fp(pta, noise)
    return psrs, pta, Nvecs, Ts, sigmas, _engine(psrs, Nvecs, Ts)


def _normals(psrs, nreal, seed=13):
    g = torch.Generator().manual_seed(seed)
    w = [torch.randn((len(p.toas), nreal), generator=g, dtype=torch.float64)
         for p in psrs]
    u = [torch.randn((12, nreal), generator=g, dtype=torch.float64)
         for _ in psrs]
    return w, u


def test_joint_null_max_chunk_independent():
    psrs, pta, Nvecs, Ts, sigmas, eng = _fixed()
    sky = fibonacci_sky(12)
    fe = FastFe(psrs, pta)
    w, u = _normals(psrs, 23)
    args = (FREQS, sky, Nvecs, Ts, sigmas, 23)
    a = fe.null_max(*args, engine=eng, joint=True, w=w, u=u, real_chunk=5)
    b = fe.null_max(*args, engine=eng, joint=True, w=w, u=u, real_chunk=17)
    assert a.shape == (23, F) and np.isfinite(a).all() and (a > 0).all()
    np.testing.assert_array_equal(a, b)
    # what it returns: the host reference on the engine's own n
    from fastfp_amd.festat import _phiinvs_from_sigmas

    n = eng.null_data(_phiinvs_from_sigmas(eng, sigmas, improper=True), 23,
                      w=w, u=u)
    prods = eng.sweep_products(sigmas=sigmas).numpy()[:, None]
    want, _ = _null_max_host(prods, _antenna_table(fe.pos, sky), n=n.numpy())
    np.testing.assert_array_equal(a, want[:, 0])
    # the generator: reproducible per (seed, real_chunk)
    c = fe.null_max(*args, seed=4, engine=eng, joint=True, real_chunk=8)
    np.testing.assert_array_equal(
        c, fe.null_max(*args, seed=4, engine=eng, joint=True, real_chunk=8))
    assert (c != fe.null_max(*args, seed=5, engine=eng, joint=True,
                             real_chunk=8)).all()
    with pytest.raises(ValueError, match="joint=True"):
        fe.null_max(*args, engine=eng, w=w, u=u)
    with pytest.raises(ValueError, match="not z="):
        fe.null_max(*args, engine=eng, joint=True,
                    z=torch.zeros((1, F, 3, 2, 23), dtype=torch.float64))


def test_joint_false_is_unchanged():
    """``joint=False`` against the parent's loop, written out: one randn
    call per chunk, ``_null_max_host`` on the engine's products."""
    psrs, pta, Nvecs, Ts, sigmas, eng = _fixed()
    sky = fibonacci_sky(12)
    fe = FastFe(psrs, pta)
    got = fe.null_max(FREQS, sky, Nvecs, Ts, sigmas, 20, seed=6, engine=eng,
                      real_chunk=8)
    prods = eng.sweep_products(sigmas=sigmas).numpy()[:, None]
    ant = _antenna_table(fe.pos, sky)
    gen = torch.Generator(device="cpu")
    gen.manual_seed(6)
    want = np.concatenate([
        _null_max_host(prods, ant, torch.randn(
            (1, F, 3, 2, c), generator=gen, dtype=torch.float64).numpy())[0]
        for c in (8, 8, 4)])
    np.testing.assert_array_equal(got, want[:, 0])
    femax, argmax, pfa = fe.false_alarm(FREQS, sky, Nvecs, Ts, sigmas, 20,
                                        seed=6, engine=eng, real_chunk=8)
    np.testing.assert_array_equal(pfa, false_alarm_probability(femax, got))


def test_false_alarm_joint():
    psrs, pta, Nvecs, Ts, sigmas, eng = _fixed()
    sky = fibonacci_sky(12)
    fe = FastFe(psrs, pta)
    args = (FREQS, sky, Nvecs, Ts, sigmas, 19)
    out = fe.false_alarm(*args, seed=2, engine=eng, joint=True, real_chunk=8)
    assert len(out) == 6
    femax, argmax, pfa, fg, fi, pg = out
    null = fe.null_max(*args, seed=2, engine=eng, joint=True, real_chunk=8)
    np.testing.assert_array_equal(pfa, false_alarm_probability(femax, null))
    assert fg == femax.max() and fi == femax.argmax()
    assert pg == (1 + (null.max(axis=1) >= fg).sum()) / 20.0
    assert pg >= pfa[fi]  # more trials never lower the probability


def test_nmfe_joint_null_max():
    psrs, pta, noise, Nvecs, Ts = _array(npsr=3, seed=7)
    rng = np.random.default_rng(17)
    samples = {k: (rng.uniform(2, 6, 5) if k.endswith("gamma")
                   else rng.uniform(-16, -14, 5)) for k in pta.params}
    sky = fibonacci_sky(12)
    nm = NMFe(psrs, pta.rn_containers)
    w, u = _normals(psrs, 9)
    args = (FREQS, sky, samples, Nvecs, Ts, 9)
    a = nm.null_max(*args, device="cpu", joint=True, w=w, u=u, draw_chunk=2,
                    real_chunk=4)
    assert a.shape == (9, 5, F) and np.isfinite(a).all()
    # neither chunk size is part of the result
    b = nm.null_max(*args, device="cpu", joint=True, w=w, u=u, draw_chunk=5,
                    real_chunk=9)
    np.testing.assert_array_equal(a, b)
    # the generator does not depend on draw_chunk: common random numbers
    c = nm.null_max(*args, seed=1, device="cpu", joint=True, draw_chunk=2,
                    real_chunk=4)
    d = nm.null_max(*args, seed=1, device="cpu", joint=True, draw_chunk=3,
                    real_chunk=4)
    np.testing.assert_array_equal(c, d)


# ----------------------------------------------------------------------
# 5. global_false_alarm on hand-made arrays
# ----------------------------------------------------------------------
def test_global_false_alarm():
    femax = np.array([1.0, 5.0, 5.0, 2.0])
    null = np.array([[0.0, 1.0, 2.0, 3.0],   # max 3
                     [5.0, 0.0, 0.0, 0.0],   # max 5: a tie counts
                     [0.0, 0.0, 0.0, 7.0],   # max 7
                     [4.9, 4.9, 4.9, 4.9]])  # max 4.9
    fg, fi, pg = global_false_alarm(femax, null)
    assert fg == 5.0 and fi == 1 and pg == 3.0 / 5.0
    # never zero
    fg, fi, pg = global_false_alarm(femax + 100.0, null)
    assert pg == 1.0 / 5.0
    # leading axes (draws) pass through
    fg, fi, pg = global_false_alarm(np.stack([femax, femax[::-1]]),
                                    np.stack([null, null], axis=1))
    assert fg.shape == fi.shape == pg.shape == (2,)
    assert list(fi) == [1, 1] and list(pg) == [0.6, 0.6]
    # the per-frequency probability never exceeds the global one
    assert (false_alarm_probability(femax, null)[1] <= 0.6)
    with pytest.raises(ValueError, match="null must be"):
        global_false_alarm(femax, null[:, :3])


# ----------------------------------------------------------------------
# 6. block-diagonal white noise is refused by name
# ----------------------------------------------------------------------
def test_block_noise_raises():
    from fastfp_amd.blocknoise import BlockNoise

    psrs, pta, noise, Nvecs, Ts = _array()
    for b in np.unique(psrs[1].backend_flags):
        noise[f"{psrs[1].name}_basis_ecorr_{b}_log10_ecorr"] = -6.3
    eng = _engine(psrs, [Nvecs[0], BlockNoise(psrs[1], noise)], Ts)
    phiinvs = [torch.as_tensor(1.0 / p) for p in _priors(Nvecs, Ts)]
    with pytest.raises(NotImplementedError, match=re.escape(psrs[1].name)):
        eng.null_data(phiinvs, 4)


# ----------------------------------------------------------------------
# 7. CLI
# ----------------------------------------------------------------------
def test_run_fe_null_joint_cli(tmp_path):
    from fastfp_amd.cli import run_fe
    from fastfp_amd.data import save_pulsars

    psrs = make_synthetic_pta(npsr=3, ntoa=60, ntm=3, seed=0)
    psrfile = str(tmp_path / "psrs.npz")
    save_pulsars(psrs, psrfile)
    noisefile = str(tmp_path / "noise.json")
    with open(noisefile, "w") as f:
        json.dump({k: v for k, v in _noise(psrs).items()
                   if not k.startswith("gw_")}, f)
    kw = dict(nfreqs=4, nsky=6, rn_comps=3, gwb_comps=3, device="cpu",
              skymax=True, null=16)
    run_fe.main(psrfile, noisefile, str(tmp_path / "a"), null_joint=True, **kw)
    run_fe.main(psrfile, noisefile, str(tmp_path / "b"), null_joint=True, **kw)
    run_fe.main(psrfile, noisefile, str(tmp_path / "c"), **kw)
    run_fe.main(psrfile, noisefile, str(tmp_path / "d"), null_joint=False,
                **kw)
    null = np.load(tmp_path / "a.null.npy")
    pg = np.load(tmp_path / "a.pfa_global.npy")
    fmax = np.load(tmp_path / "a.max.npy")
    assert null.shape == (16, 4) and np.isfinite(null).all()
    assert pg.shape == (3,)
    assert pg[0] == fmax.max() and pg[1] == fmax.argmax()
    assert pg[2] == global_false_alarm(fmax, null)[2] and 0 < pg[2] <= 1
    np.testing.assert_array_equal(
        np.load(tmp_path / "a.pfa.npy"), false_alarm_probability(fmax, null))
    for ext in ("null", "pfa", "pfa_global", "max", "argmax"):
        assert (tmp_path / f"a.{ext}.npy").read_bytes() \
            == (tmp_path / f"b.{ext}.npy").read_bytes()
    # without the flag: the outputs of the parent, byte for byte
    assert not (tmp_path / "c.pfa_global.npy").exists()
    assert (np.load(tmp_path / "c.null.npy") != null).all()
    fe = FastFe(psrs)
    from fastfp_amd.model import get_mats_fp as mats

    with open(noisefile) as f:
        nz = json.load(f)
    nz["gw_gamma"], nz["gw_log10_A"] = 13 / 3, float(np.log10(2e-15))
    pta = initialize_pta(psrs, nz, inc_cp=True, rn_comps=3, gwb_comps=3)
    Nvecs, Ts, sigmas = mats(pta, nz)
    freqs = np.linspace(2e-9, 3e-7, 4)
    want = fe.null_max(freqs, fibonacci_sky(6), Nvecs, Ts, sigmas, 16,
                       seed=0, device="cpu")
    np.testing.assert_array_equal(np.load(tmp_path / "c.null.npy"), want)
    for ext in ("null", "pfa", "max", "argmax"):
        assert (tmp_path / f"c.{ext}.npy").read_bytes() \
            == (tmp_path / f"d.{ext}.npy").read_bytes()
    with pytest.raises(ValueError, match="null_joint needs null"):
        run_fe.main("x", "x", "x", skymax=True, null_joint=True)
