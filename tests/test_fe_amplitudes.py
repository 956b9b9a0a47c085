"""Fe maximum-likelihood amplitudes ``a = M^-1 N`` and the source
parameters at the maximum: the amplitude <-> (zeta, cos iota, psi, phi0)
maps, the coherent Earth-term injector, the host solve, the
``fe_amplitudes`` kernel, ``sweep_max(amplitudes=True)``,
``FastFe.amplitudes`` and the ``--amplitudes`` CLI flag.

Tolerances.  The maps are closed-form fp64 (a prototype of the formulas
round-tripped parameters to 3.5e-12 and amplitudes to 1.5e-13): 1e-10.
Every solve is compared at the project's Fe tolerance rtol = 1e-9
(tests/test_festat.py), with an absolute floor of 1e-9 max|a| per point
because single components cross zero.  The device inputs are those of
tests/test_fe_device.py (condition number of every 4x4 at most 85), so
an fp64 LDL^T solve sits six orders below that bound.
"""

import functools
import json
import sys

import numpy as np
import pytest
import torch

from fastfp_amd import FpEngine, initialize_pta, make_synthetic_pta
from fastfp_amd.cli.run_fe import fibonacci_sky
from fastfp_amd.festat import (
    FastFe,
    NMFe,
    _assemble_fe,
    _assemble_fe_draws,
    gw_antenna_pattern,
)
from fastfp_amd.model import get_mats_fp, get_mats_nmfp
from fastfp_amd.noise import batch_phiinv

RTOL = 1e-9
MAP_TOL = 1e-10
SEEDS = {5: 31, 9: 32}
DEV = "cuda:0"
INJ = dict(zeta=3e-7, cosi=0.3, psi=0.4, phi0=1.1)
INJ_SKY = (1.0, 2.0)


# ----------------------------------------------------------------------
# shared inputs (the recipes of tests/test_fe_device.py)
# ----------------------------------------------------------------------
def _noise(psrs):
    noise = {"gw_gamma": 13.0 / 3.0, "gw_log10_A": float(np.log10(2e-15))}
    for p in psrs:
        noise[f"{p.name}_red_noise_gamma"] = 4.0
        noise[f"{p.name}_red_noise_log10_A"] = -14.5
    return noise


def _pta(npsr, ntoa=80, seed=0, rn_comps=3):
    psrs = make_synthetic_pta(npsr=npsr, ntoa=ntoa, ntm=3, seed=seed)
    noise = _noise(psrs)
    pta = initialize_pta(psrs, noise, inc_cp=True, rn_comps=rn_comps,
                         gwb_comps=3)
    return psrs, noise, pta


def _samples(pta, D, seed):
    rng = np.random.default_rng(seed)
    return {
        n: (rng.uniform(2, 6, D) if n.endswith("gamma")
            else rng.uniform(-16, -14, D))
        for n in pta.params
    }


@functools.lru_cache(maxsize=None)
def _case(npsr, rn_comps=3, F=7, D=5):
    psrs, noise, pta = _pta(npsr, seed=SEEDS[npsr], rn_comps=rn_comps)
    _, Nvecs, Ts = get_mats_nmfp(pta, noise)
    samples = _samples(pta, D, seed=SEEDS[npsr] + 100)
    phiinvs = batch_phiinv(pta.rn_containers, samples)
    phiinvs = [p[None, :] if p.dim() == 1 else p for p in phiinvs]
    freqs = np.linspace(5e-9, 4e-8, F)
    return psrs, pta, Nvecs, Ts, samples, phiinvs, freqs


@functools.lru_cache(maxsize=None)
def _cpu_products(npsr):
    """(P, 5, 5, 7) CPU-engine products (D*F = 35: a partial wave)."""
    psrs, pta, Nvecs, Ts, samples, phiinvs, freqs = _case(npsr)
    eng = FpEngine(psrs, Nvecs, Ts, device="cpu")
    eng.precompute(freqs)
    prods = eng.sweep_products(phiinvs=phiinvs).numpy()
    assert prods.shape == (npsr, 5, 5, 7)
    return prods


@functools.lru_cache(maxsize=None)
def _ant(npsr, nsky=48):
    psrs = _case(npsr)[0]
    pos = np.stack([p.pos for p in psrs])
    sky = fibonacci_sky(48)[:nsky]
    ant = np.empty((nsky, npsr, 2))
    for k, (th, ph) in enumerate(sky):
        ant[k, :, 0], ant[k, :, 1] = gw_antenna_pattern(pos, th, ph)
    return ant


def _synthetic_products(P, D=5, F=7, nsky=20, seed=3):
    """Well-posed random inputs: positive-definite per-pulsar 2x2 blocks
    and a random antenna table."""
    rng = np.random.default_rng(seed)
    prods = np.empty((P, D, 5, F))
    prods[:, :, 0:2] = rng.uniform(1.0, 2.0, (P, D, 2, F))
    prods[:, :, 2] = 0.1 * rng.normal(size=(P, D, F))
    prods[:, :, 3:] = rng.normal(size=(P, D, 2, F))
    return prods, rng.normal(size=(nsky, P, 2))


def _dev(x):
    return torch.as_tensor(x, dtype=torch.float64).to(DEV)


def _mixed_idx(D, F, nsky):
    """A different sky row in every neighbouring lane."""
    n = np.arange(D * F)
    return ((7 * n + 3) % nsky).reshape(D, F).astype(np.int32)


def _host_at(prods, ant, idx):
    """(fe (D, F), a (D, F, 4)) of the host solve at sky row idx[d, f]:
    the reference every device result is compared against."""
    D, F = idx.shape
    fe = np.empty((D, F))
    a = np.empty((D, F, 4))
    for k in np.unique(idx):
        fk, ak = _assemble_fe_draws(prods, ant[k, :, 0], ant[k, :, 1],
                                    amplitudes=True)
        sel = idx == k
        fe[sel], a[sel] = fk[sel], ak[sel]
    return fe, a


def _assert_amps_close(got, want, what=""):
    """rtol = 1e-9 with atol = 1e-9 max|a| of each point."""
    scale = np.abs(want).max(axis=-1, keepdims=True)
    err = (np.abs(got - want) / scale).max()
    print(f"{what}: max |da| / max|a| = {err:.3e}")
    assert np.isfinite(got).all()
    assert (np.abs(got - want) <= RTOL * np.abs(want) + RTOL * scale).all(), \
        f"{what}: {err:.3e}"


def _moments(prods, fplus, fcross):
    """N (..., 4) rebuilt from the products, independent of the solve."""
    sr, cr = prods[:, ..., 3, :], prods[:, ..., 4, :]
    sub = "p,p...->..."
    return np.stack([np.einsum(sub, fplus, sr), np.einsum(sub, fplus, cr),
                     np.einsum(sub, fcross, sr), np.einsum(sub, fcross, cr)],
                    axis=-1)


# ----------------------------------------------------------------------
# 1. CPU: the amplitude <-> parameter maps
# ----------------------------------------------------------------------
def test_parameter_round_trip():
    from fastfp_amd import cw_amplitudes, cw_parameters

    rng = np.random.default_rng(0)
    n = 20000
    zeta = 10.0 ** rng.uniform(-9, -6, n)
    cosi = rng.uniform(-0.95, 0.95, n)
    psi = rng.uniform(0.0, 0.5 * np.pi, n)
    phi0 = rng.uniform(0.0, 2.0 * np.pi, n)
    a = cw_amplitudes(zeta, cosi, psi, phi0)
    assert a.shape == (n, 4)
    f = 2e-8
    par = cw_parameters(a, f=f)
    assert sorted(par) == ["cosi", "h0", "phi0", "psi", "zeta"]
    errs = {
        "zeta": np.abs(par["zeta"] / zeta - 1).max(),
        "h0": np.abs(par["h0"] / (2 * np.pi * f * zeta) - 1).max(),
        "cosi": np.abs(par["cosi"] - cosi).max(),
        "psi": np.abs(par["psi"] - psi).max(),
        "phi0": np.abs(par["phi0"] - phi0).max(),
    }
    print({k: f"{v:.2e}" for k, v in errs.items()})
    for k, v in errs.items():
        assert v < MAP_TOL, (k, v)
    assert (par["psi"] >= 0).all() and (par["psi"] < 0.5 * np.pi).all()
    assert (par["phi0"] >= 0).all() and (par["phi0"] < 2 * np.pi).all()
    assert "h0" not in cw_parameters(a)


def test_amplitude_round_trip_and_broadcast():
    from fastfp_amd import cw_amplitudes, cw_parameters

    rng = np.random.default_rng(1)
    a = rng.normal(size=(20000, 4)) * 10.0 ** rng.uniform(-9, -5, (20000, 1))
    par = cw_parameters(a)
    back = cw_amplitudes(par["zeta"], par["cosi"], par["psi"], par["phi0"])
    err = (np.abs(back - a).max(axis=1) / np.abs(a).max(axis=1)).max()
    print(f"amplitude round trip {err:.2e}")
    assert err < MAP_TOL
    assert (np.abs(par["cosi"]) <= 1.0).all()
    # leading axes broadcast: (3, 1) x (5,) -> (3, 5, 4); f per column
    b = cw_amplitudes(np.array([[1e-7], [2e-7], [3e-7]]), 0.2,
                      np.linspace(0.1, 1.0, 5), 0.3)
    assert b.shape == (3, 5, 4)
    pb = cw_parameters(b, f=np.linspace(1e-8, 2e-8, 5))
    assert pb["h0"].shape == (3, 5)
    np.testing.assert_allclose(pb["psi"], np.broadcast_to(
        np.linspace(0.1, 1.0, 5), (3, 5)), atol=MAP_TOL)
    # (psi + pi/2, phi0 + pi) is the same signal
    np.testing.assert_allclose(
        cw_amplitudes(1e-7, 0.3, 0.4 + 0.5 * np.pi, 1.1 + np.pi),
        cw_amplitudes(1e-7, 0.3, 0.4, 1.1), rtol=0, atol=1e-7 * 1e-14)


@pytest.mark.parametrize("cosi", [1.0, -1.0])
def test_circular_polarisation(cosi):
    from fastfp_amd import cw_amplitudes, cw_parameters

    zeta = 2.5e-7
    a = cw_amplitudes(zeta, cosi, 0.4, 1.1)
    par = cw_parameters(a)
    assert abs(par["zeta"] / zeta - 1) < MAP_TOL
    assert abs(par["cosi"] - cosi) < MAP_TOL
    back = cw_amplitudes(par["zeta"], par["cosi"], par["psi"], par["phi0"])
    assert np.abs(back - a).max() < MAP_TOL * np.abs(a).max()
    zero = cw_parameters(np.zeros(4))
    assert zero["zeta"] == 0.0 and np.isfinite(zero["cosi"])


# ----------------------------------------------------------------------
# 2. CPU: noiseless injection recovery
# ----------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _injected(seed, npsr):
    """Array whose residuals ARE the injected Earth term (grid point 3
    of 5 frequencies, sky INJ_SKY)."""
    from fastfp_amd import inject_earth_term_cw

    psrs = make_synthetic_pta(npsr=npsr, ntoa=120, ntm=3, toaerr=1e-7,
                              seed=seed)
    freqs = np.linspace(5e-9, 4e-8, 5)
    for p in psrs:
        p.residuals = np.zeros_like(p.residuals)
    a = inject_earth_term_cw(psrs, freqs[3], *INJ_SKY, **INJ)
    assert a.shape == (4,)
    noise = _noise(psrs)
    pta = initialize_pta(psrs, noise, inc_cp=True, rn_comps=3, gwb_comps=3)
    Nvecs, Ts, sigmas = get_mats_fp(pta, noise)
    return psrs, pta, Nvecs, Ts, sigmas, freqs, a


def _check_recovery(fe, amps, a, freqs):
    from fastfp_amd import cw_parameters

    assert fe.shape == (5,) and amps.shape == (5, 4)
    err = np.abs(amps[3] - a).max() / np.abs(a).max()
    print(f"injection recovery: max |da| / max|a| = {err:.3e}")
    assert err <= RTOL
    # noiseless: Fe = 1/2 a^T M a peaks at the injected frequency
    assert np.argmax(fe) == 3
    # amplitudes good to 1e-9 max|a|; the angles come from atan2 of
    # combinations of size zeta (1 -+ c)^2 >= 0.49 zeta against max|a|
    # <= 1.09 zeta, zeta and cos iota from sums of squares: a factor of
    # under 10 on the amplitude error
    par = cw_parameters(amps[3], f=freqs[3])
    assert abs(par["zeta"] / INJ["zeta"] - 1) < 1e-8
    assert abs(par["h0"] / (2 * np.pi * freqs[3] * INJ["zeta"]) - 1) < 1e-8
    for k in ("cosi", "psi", "phi0"):
        assert abs(par[k] - INJ[k]) < 1e-8, (k, par[k])


@pytest.mark.parametrize("seed,npsr", [(13, 6), (32, 9)])
def test_injection_recovery_cpu(seed, npsr):
    psrs, pta, Nvecs, Ts, sigmas, freqs, a = _injected(seed, npsr)
    fe, amps = FastFe(psrs, pta).amplitudes(
        freqs, *INJ_SKY, Nvecs, Ts, sigmas, device="cpu")
    _check_recovery(fe, amps, a, freqs)


def test_injector_arguments():
    from fastfp_amd import cw_amplitudes, inject_earth_term_cw

    psrs = make_synthetic_pta(npsr=2, ntoa=30, ntm=3, seed=5)
    before = [p.residuals.copy() for p in psrs]
    with pytest.raises(ValueError, match="exactly one"):
        inject_earth_term_cw(psrs, 1e-8, 1.0, 2.0)
    with pytest.raises(ValueError, match="exactly one"):
        inject_earth_term_cw(psrs, 1e-8, 1.0, 2.0, h0=1e-14, zeta=1e-7)
    f = 1e-8
    a = inject_earth_term_cw(psrs, f, 1.0, 2.0, h0=1e-14, cosi=0.5, psi=0.2,
                             phi0=0.7)
    np.testing.assert_allclose(
        a, cw_amplitudes(1e-14 / (2 * np.pi * f), 0.5, 0.2, 0.7), rtol=1e-15)
    # added to the residuals, through the antenna pattern
    p = psrs[1]
    fp, fx = gw_antenna_pattern(p.pos, 1.0, 2.0)
    s, c = np.sin(2 * np.pi * f * p.toas), np.cos(2 * np.pi * f * p.toas)
    want = before[1] + fp * (a[0] * s + a[1] * c) + fx * (a[2] * s + a[3] * c)
    np.testing.assert_allclose(p.residuals, want, rtol=0,
                               atol=1e-14 * np.abs(a).max())


# ----------------------------------------------------------------------
# 3. CPU: sweep_max(amplitudes=True)
# ----------------------------------------------------------------------
def test_fastfe_sweep_max_amplitudes_cpu():
    psrs, noise, pta = _pta(5, seed=31)
    Nvecs, Ts, sigmas = get_mats_fp(pta, noise)
    freqs = np.linspace(5e-9, 4e-8, 7)
    sky = fibonacci_sky(48)
    fe = FastFe(psrs, pta)
    eng = FpEngine(psrs, Nvecs, Ts, device="cpu")
    eng.precompute(freqs)
    femax2, argmax2 = fe.sweep_max(freqs, sky, Nvecs, Ts, sigmas, engine=eng)
    femax, argmax, amps = fe.sweep_max(freqs, sky, Nvecs, Ts, sigmas,
                                       engine=eng, amplitudes=True)
    assert amps.shape == (7, 4)
    np.testing.assert_array_equal(femax, femax2)
    np.testing.assert_array_equal(argmax, argmax2)
    prods = eng.sweep_products(sigmas=sigmas).numpy()
    for j in range(7):
        fplus, fcross = gw_antenna_pattern(fe.pos, *sky[argmax[j]])
        N = _moments(prods, fplus, fcross)[j]
        assert abs(0.5 * N @ amps[j] / femax[j] - 1) < 1e-12
    # the targeted search at that sky point gives the same numbers
    j = 2
    fe1, a1 = fe.amplitudes(freqs, *sky[argmax[j]], Nvecs, Ts, sigmas,
                            engine=eng)
    assert fe1.shape == (7,) and a1.shape == (7, 4)
    np.testing.assert_array_equal(a1[j], amps[j])
    np.testing.assert_array_equal(fe1[j], femax[j])


def test_nmfe_sweep_max_amplitudes_cpu():
    psrs, pta, Nvecs, Ts, samples, phiinvs, freqs = _case(5)
    sky = fibonacci_sky(48)
    nm = NMFe(psrs, pta.rn_containers)
    femax2, argmax2 = nm.sweep_max(freqs, sky, samples, Nvecs, Ts,
                                   device="cpu", draw_chunk=2)
    femax, argmax, amps = nm.sweep_max(freqs, sky, samples, Nvecs, Ts,
                                       device="cpu", draw_chunk=2,
                                       amplitudes=True)
    assert amps.shape == (5, 7, 4)
    np.testing.assert_array_equal(femax, femax2)
    np.testing.assert_array_equal(argmax, argmax2)
    prods, ant = _cpu_products(5), _ant(5)
    for d in range(5):
        for j in range(7):
            k = argmax[d, j]
            N = _moments(prods, ant[k, :, 0], ant[k, :, 1])[d, j]
            assert abs(0.5 * N @ amps[d, j] / femax[d, j] - 1) < 1e-12


def test_default_returns_unchanged():
    """amplitudes=False is the code that ran before: Fe alone."""
    prods, ant = _cpu_products(5), _ant(5)
    fe = _assemble_fe_draws(prods, ant[3, :, 0], ant[3, :, 1])
    fe2, a = _assemble_fe_draws(prods, ant[3, :, 0], ant[3, :, 1],
                                amplitudes=True)
    assert isinstance(fe, np.ndarray) and fe.shape == (5, 7)
    np.testing.assert_array_equal(fe, fe2)
    assert a.shape == (5, 7, 4)
    one = _assemble_fe(prods[:, 1], ant[3, :, 0], ant[3, :, 1])
    one2, a1 = _assemble_fe(prods[:, 1], ant[3, :, 0], ant[3, :, 1],
                            amplitudes=True)
    np.testing.assert_array_equal(one, one2)
    assert a1.shape == (7, 4)


# ----------------------------------------------------------------------
# 4. CLI
# ----------------------------------------------------------------------
def _cli_inputs(tmp_path):
    """3-pulsar npz + noise json + fake chain (the recipe of
    tests/test_fe_device.py)."""
    from fastfp_amd.data import save_pulsars

    psrs = make_synthetic_pta(npsr=3, ntoa=60, ntm=3, seed=0)
    psrfile = str(tmp_path / "psrs.npz")
    save_pulsars(psrs, psrfile)
    noise = {}
    for p in psrs:
        noise[f"{p.name}_red_noise_gamma"] = 4.0
        noise[f"{p.name}_red_noise_log10_A"] = -14.5
    noisefile = str(tmp_path / "noise.json")
    with open(noisefile, "w") as f:
        json.dump(noise, f)
    nparams = 2 * len(psrs) + 2
    rng = np.random.default_rng(1)
    chain = np.zeros((40, nparams + 4))
    for i in range(nparams):
        chain[:, i] = (rng.uniform(2.0, 6.0, 40) if i % 2 == 0
                       else rng.uniform(-16, -14, 40))
    chainfile = str(tmp_path / "chain.txt")
    np.savetxt(chainfile, chain)
    return psrfile, noisefile, chainfile


def _check_cwpar(cwpar, amps, freqs):
    from fastfp_amd import cw_amplitudes

    assert cwpar.shape == amps.shape
    h0, cosi, psi, phi0 = np.moveaxis(cwpar, -1, 0)
    back = cw_amplitudes(h0 / (2 * np.pi * freqs), cosi, psi, phi0)
    scale = np.abs(amps).max(axis=-1, keepdims=True)
    assert (np.abs(back - amps) <= MAP_TOL * scale).all()


def test_run_fe_amplitudes_cli(tmp_path):
    from fastfp_amd.cli import run_fe

    psrfile, noisefile, _ = _cli_inputs(tmp_path)
    kw = dict(nfreqs=4, nsky=6, rn_comps=3, gwb_comps=3, device="cpu",
              skymax=True)
    run_fe.main(psrfile, noisefile, str(tmp_path / "a"), amplitudes=True,
                **kw)
    run_fe.main(psrfile, noisefile, str(tmp_path / "b"), **kw)
    assert not (tmp_path / "b.amps.npy").exists()
    np.testing.assert_array_equal(np.load(tmp_path / "a.max.npy"),
                                  np.load(tmp_path / "b.max.npy"))
    np.testing.assert_array_equal(np.load(tmp_path / "a.argmax.npy"),
                                  np.load(tmp_path / "b.argmax.npy"))
    amps = np.load(tmp_path / "a.amps.npy")
    cwpar = np.load(tmp_path / "a.cwpar.npy")
    assert amps.shape == (4, 4) and np.isfinite(amps).all()
    with open(tmp_path / "a.json") as f:
        freqs = np.asarray(json.load(f)["freqs"])
    _check_cwpar(cwpar, amps, freqs)


def test_run_nmfe_amplitudes_cli(tmp_path):
    from fastfp_amd.cli import run_nmfe

    psrfile, noisefile, chainfile = _cli_inputs(tmp_path)
    kw = dict(inc_cp=True, nrncomps=3, ngwbcomps=3, ncwfreqs=4, nsamples=5,
              nsky=6, outdir=str(tmp_path), device="cpu", batch_size=2,
              skymax=True)
    run_nmfe.main(psrfile, noisefile, chainfile, "a", amplitudes=True, **kw)
    run_nmfe.main(psrfile, noisefile, chainfile, "b", **kw)
    assert not (tmp_path / "b.amps.npy").exists()
    np.testing.assert_array_equal(np.load(tmp_path / "a.max.npy"),
                                  np.load(tmp_path / "b.max.npy"))
    amps = np.load(tmp_path / "a.amps.npy")
    cwpar = np.load(tmp_path / "a.cwpar.npy")
    assert amps.shape == (5, 4, 4) and np.isfinite(amps).all()
    with open(tmp_path / "a.meta.json") as f:
        freqs = np.asarray(json.load(f)["freqs"])
    _check_cwpar(cwpar, amps, freqs)


@pytest.mark.parametrize("mod,npos", [("run_fe", 3), ("run_nmfe", 4)])
def test_cli_amplitudes_needs_skymax(mod, npos, monkeypatch, capsys):
    import importlib

    cli = importlib.import_module(f"fastfp_amd.cli.{mod}")
    monkeypatch.setattr(sys, "argv", [mod] + ["x"] * npos + ["--amplitudes"])
    with pytest.raises(SystemExit) as exc:
        cli.cli()
    assert exc.value.code == 2
    assert "--amplitudes requires --skymax" in capsys.readouterr().err
    with pytest.raises(ValueError, match="skymax"):
        cli.main(*["x"] * npos, amplitudes=True)


# ----------------------------------------------------------------------
# 5. CPU: singular sky
# ----------------------------------------------------------------------
def test_singular_sky_amplitudes_are_pinv():
    prods = _cpu_products(5)
    fplus = _ant(5)[7, :, 0].copy()
    fcross = np.zeros(5)
    fe, a = _assemble_fe_draws(prods, fplus, fcross, amplitudes=True)
    assert np.isfinite(a).all() and np.isfinite(fe).all()
    ss, cc, sc = prods[:, :, 0], prods[:, :, 1], prods[:, :, 2]
    w = fplus[:, None, None] ** 2
    for d in range(5):
        for j in range(7):
            M = np.zeros((4, 4))
            M[0, 0] = (w * ss).sum(0)[d, j]
            M[0, 1] = M[1, 0] = (w * sc).sum(0)[d, j]
            M[1, 1] = (w * cc).sum(0)[d, j]
            N = _moments(prods, fplus, fcross)[d, j]
            want = np.linalg.pinv(M, rcond=1e-12) @ N
            np.testing.assert_allclose(a[d, j], want, rtol=RTOL,
                                       atol=RTOL * np.abs(want).max())
    # single-draw form
    fe1, a1 = _assemble_fe(prods[:, 0], fplus, fcross, amplitudes=True)
    np.testing.assert_array_equal(a1, a[0])


# ----------------------------------------------------------------------
# 6. GPU: the kernel against the host solve
# ----------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("npsr", [5, 9])
def test_fe_amplitudes_mixed_indices(npsr):
    from fastfp_amd import ops

    prods, ant = _cpu_products(npsr), _ant(npsr)
    idx = _mixed_idx(5, 7, 48)
    assert (np.diff(idx.ravel()) != 0).all()
    fe_h, a_h = _host_at(prods, ant, idx)
    prods_d, ant_d, idx_d = _dev(prods), _dev(ant), torch.as_tensor(idx).to(DEV)
    amps, fe, status = ops.fe_amplitudes(prods_d, ant_d, idx_d, repair=False)
    assert amps.shape == (5, 7, 4) and amps.dtype == torch.float64
    assert fe.shape == (5, 7) and fe.dtype == torch.float64
    assert status.shape == (5, 7) and status.dtype == torch.int32
    assert int(status.abs().sum()) == 0
    _assert_amps_close(amps.cpu().numpy(), a_h, f"P={npsr}")
    np.testing.assert_allclose(fe.cpu().numpy(), fe_h, rtol=RTOL)
    # the sky kernel's Fe at the same index (other summation order)
    fmap = ops.fe_assemble(prods_d, ant_d, repair=False).cpu().numpy()
    at = np.take_along_axis(fmap, idx[:, None, :].astype(np.int64),
                            axis=1)[:, 0]
    print(f"fe vs fe_assemble: {np.abs(fe.cpu().numpy() / at - 1).max():.3e}")
    np.testing.assert_allclose(fe.cpu().numpy(), at, rtol=RTOL)
    again = ops.fe_amplitudes(prods_d, ant_d, idx_d, repair=False)
    for x, y in zip((amps, fe, status), again):
        assert torch.equal(x, y)
    # int64 indices (numpy argmax) are accepted by the wrapper
    a64 = ops.fe_amplitudes(prods_d, ant_d, idx_d.long(), repair=False)[0]
    assert torch.equal(a64, amps)


# ----------------------------------------------------------------------
# 7. GPU: guards
# ----------------------------------------------------------------------
@pytest.mark.gpu
def test_fe_amplitudes_index_guard():
    from fastfp_amd import ops

    prods, ant = _cpu_products(5), _ant(5)
    idx = _mixed_idx(5, 7, 48)
    prods_d, ant_d = _dev(prods), _dev(ant)
    clean = ops.fe_amplitudes(prods_d, ant_d, torch.as_tensor(idx).to(DEV),
                              repair=False)
    bad = idx.copy()
    bad[0, 0], bad[2, 3], bad[4, 6] = -1, 48, 2**31 - 1
    mask = bad != idx
    for repair in (False, True):  # repair leaves status 2 alone
        amps, fe, status = ops.fe_amplitudes(
            prods_d, ant_d, torch.as_tensor(bad).to(DEV), repair=repair)
        amps, fe, status = (t.cpu().numpy() for t in (amps, fe, status))
        assert (status[mask] == 2).all() and (status[~mask] == 0).all()
        assert np.isnan(amps[mask]).all() and np.isnan(fe[mask]).all()
        np.testing.assert_array_equal(amps[~mask],
                                      clean[0].cpu().numpy()[~mask])
        np.testing.assert_array_equal(fe[~mask],
                                      clean[1].cpu().numpy()[~mask])


@pytest.mark.gpu
def test_fe_amplitudes_singular_row_repaired():
    from fastfp_amd import ops

    prods = _cpu_products(5)
    ant = _ant(5).copy()
    row = 7
    ant[row, :, 1] = 0.0
    idx = _mixed_idx(5, 7, 48)
    idx[1, :] = row
    hit = idx == row
    assert hit.sum() >= 7 and (~hit).sum() > 0
    fe_h, a_h = _host_at(prods, ant, idx)  # row 7: the pinv branch
    assert np.isfinite(a_h).all()
    args = (_dev(prods), _dev(ant), torch.as_tensor(idx).to(DEV))
    amps, fe, status = (t.cpu().numpy()
                        for t in ops.fe_amplitudes(*args, repair=False))
    assert (status[hit] == 1).all() and (status[~hit] == 0).all()
    assert np.isnan(amps[hit]).all() and np.isnan(fe[hit]).all()
    assert np.isfinite(amps[~hit]).all()
    amps, fe, status = (t.cpu().numpy() for t in ops.fe_amplitudes(*args))
    assert (status[hit] == 1).all()
    _assert_amps_close(amps, a_h, "repaired")
    np.testing.assert_allclose(fe, fe_h, rtol=RTOL)


@pytest.mark.gpu
def test_fe_amplitudes_rejects_bad_inputs():
    from fastfp_amd import ops
    from fastfp_amd.ops import _fastfp_hip as ext

    prods, ant = _dev(_cpu_products(5)), _dev(_ant(5))
    idx = torch.zeros((5, 7), dtype=torch.int32, device=DEV)
    with pytest.raises(RuntimeError, match="int32"):
        ext.fe_amplitudes(prods, ant, idx.long())
    with pytest.raises(RuntimeError, match=r"\(D, F\)"):
        ops.fe_amplitudes(prods, ant, idx[:, :6])
    with pytest.raises(RuntimeError, match="P matching"):
        ops.fe_amplitudes(prods, ant[:, :4], idx)
    with pytest.raises(RuntimeError, match="fp64"):
        ops.fe_amplitudes(prods.float(), ant, idx)


# ----------------------------------------------------------------------
# 8. GPU: pulsar counts
# ----------------------------------------------------------------------
@pytest.mark.gpu
def test_fe_amplitudes_no_pulsar_cap():
    """P = 249 is one past the LDS tile of the sky kernels; this kernel
    has no tile."""
    from fastfp_amd import ops

    prods, ant = _synthetic_products(249)
    idx = _mixed_idx(5, 7, 20)
    fe_h, a_h = _host_at(prods, ant, idx)
    amps, fe, status = ops.fe_amplitudes(
        _dev(prods), _dev(ant), torch.as_tensor(idx).to(DEV), repair=False)
    assert int(status.abs().sum()) == 0
    _assert_amps_close(amps.cpu().numpy(), a_h, "P=249")
    np.testing.assert_allclose(fe.cpu().numpy(), fe_h, rtol=RTOL)


@pytest.mark.gpu
def test_fe_amplitudes_single_pulsar_degenerate():
    """One pulsar: M = (F+, Fx)(F+, Fx)^T x [[ss, sc], [sc, cc]] has rank
    2, every point is degenerate."""
    from fastfp_amd import ops

    prods, ant = _synthetic_products(1)
    idx = _mixed_idx(5, 7, 20)
    amps, fe, status = ops.fe_amplitudes(
        _dev(prods), _dev(ant), torch.as_tensor(idx).to(DEV), repair=False)
    assert (status.cpu().numpy() == 1).all()
    assert torch.isnan(amps).all() and torch.isnan(fe).all()


# ----------------------------------------------------------------------
# 9. GPU: end to end
# ----------------------------------------------------------------------
@pytest.mark.gpu
def test_fastfe_sweep_max_amplitudes_device():
    psrs, noise, pta = _pta(5, seed=31)
    Nvecs, Ts, sigmas = get_mats_fp(pta, noise)
    freqs = np.linspace(5e-9, 4e-8, 7)
    sky = fibonacci_sky(48)
    fe = FastFe(psrs, pta)
    wmax, warg, wamp = fe.sweep_max(freqs, sky, Nvecs, Ts, sigmas,
                                    device="cpu", amplitudes=True)
    eng = FpEngine(psrs, Nvecs, Ts, device=DEV)
    eng.precompute(freqs)
    femax, argmax, amps = fe.sweep_max(freqs, sky, Nvecs, Ts, sigmas,
                                       engine=eng, amplitudes=True)
    assert amps.shape == (7, 4) and argmax.dtype == np.int64
    np.testing.assert_allclose(femax, wmax, rtol=RTOL)
    np.testing.assert_array_equal(argmax, warg)
    _assert_amps_close(amps, wamp, "FastFe.sweep_max")
    # the two-value call is what it was
    f2, a2 = fe.sweep_max(freqs, sky, Nvecs, Ts, sigmas, engine=eng)
    np.testing.assert_array_equal(f2, femax)
    np.testing.assert_array_equal(a2, argmax)


@pytest.mark.gpu
def test_nmfe_sweep_max_amplitudes_device():
    psrs, pta, Nvecs, Ts, samples, _, freqs = _case(5)
    sky = fibonacci_sky(48)
    nm = NMFe(psrs, pta.rn_containers)
    wmax, warg, wamp = nm.sweep_max(freqs, sky, samples, Nvecs, Ts,
                                    device="cpu", draw_chunk=2,
                                    amplitudes=True)
    femax, argmax, amps = nm.sweep_max(freqs, sky, samples, Nvecs, Ts,
                                       device=DEV, draw_chunk=2,
                                       amplitudes=True)
    assert amps.shape == (5, 7, 4)
    np.testing.assert_allclose(femax, wmax, rtol=RTOL)
    np.testing.assert_array_equal(argmax, warg)
    _assert_amps_close(amps, wamp, "NMFe.sweep_max")


@pytest.mark.gpu
@pytest.mark.parametrize("seed,npsr", [(13, 6), (32, 9)])
def test_injection_recovery_device(seed, npsr):
    psrs, pta, Nvecs, Ts, sigmas, freqs, a = _injected(seed, npsr)
    fe, amps = FastFe(psrs, pta).amplitudes(
        freqs, *INJ_SKY, Nvecs, Ts, sigmas, device=DEV)
    _check_recovery(fe, amps, a, freqs)
