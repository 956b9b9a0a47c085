"""Fe on the device: products mode of the HIP solve, the sky-assembly
kernels (``fe_assemble`` / ``fe_skymax``), the sky-maximised public
entry points and their CLI flags.

Reference inputs: 5- and 9-pulsar synthetic arrays (ntoa=80, seeds 31 /
32, common process on), D=5 red-noise draws (log10_A ~ U[-16, -14],
gamma ~ U[2, 6]) and the 48-point Fibonacci sky.  On these inputs every
4x4 M is well conditioned (condition number <= 85, smallest relative
Cholesky pivot 0.18) and a straight 4x4 Cholesky assembly agrees with
the ``np.linalg.solve`` host assembly to 1.5e-15, so the GPU-vs-CPU Fe
tolerance of the project (rtol=1e-9, tests/test_festat.py) applies with
no case excluded.
"""

import functools
import json

import numpy as np
import pytest
import torch

from fastfp_amd import FpEngine, initialize_pta, make_synthetic_pta
from fastfp_amd.cli.run_fe import fibonacci_sky
from fastfp_amd.festat import (
    FastFe,
    NMFe,
    _assemble_fe_draws,
    gw_antenna_pattern,
)
from fastfp_amd.model import get_mats_fp, get_mats_nmfp
from fastfp_amd.noise import batch_phiinv

RTOL = 1e-9
SEEDS = {5: 31, 9: 32}
DEV = "cuda:0"


def _pta(npsr, ntoa=80, seed=0, rn_comps=3):
    psrs = make_synthetic_pta(npsr=npsr, ntoa=ntoa, ntm=3, seed=seed)
    noise = {"gw_gamma": 13.0 / 3.0, "gw_log10_A": float(np.log10(2e-15))}
    for p in psrs:
        noise[f"{p.name}_red_noise_gamma"] = 4.0
        noise[f"{p.name}_red_noise_log10_A"] = -14.5
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
    """(psrs, pta, Nvecs, Ts, samples, phiinvs, freqs) of one reference
    array; built once and shared (read-only) between the tests."""
    psrs, noise, pta = _pta(npsr, seed=SEEDS[npsr], rn_comps=rn_comps)
    _, Nvecs, Ts = get_mats_nmfp(pta, noise)
    samples = _samples(pta, D, seed=SEEDS[npsr] + 100)
    phiinvs = batch_phiinv(pta.rn_containers, samples)
    phiinvs = [p[None, :] if p.dim() == 1 else p for p in phiinvs]
    freqs = np.linspace(5e-9, 4e-8, F)
    return psrs, pta, Nvecs, Ts, samples, phiinvs, freqs


@functools.lru_cache(maxsize=None)
def _cpu_products(npsr):
    """(P, 5, 5, 7) products of the reference array from the CPU engine
    (D*F = 35: a partial column tile)."""
    psrs, pta, Nvecs, Ts, samples, phiinvs, freqs = _case(npsr)
    eng = FpEngine(psrs, Nvecs, Ts, device="cpu")
    eng.precompute(freqs)
    prods = eng.sweep_products(phiinvs=phiinvs).numpy()
    assert prods.shape == (npsr, 5, 5, 7)
    return prods


def _ant(npsr, nsky):
    """(nsky, P, 2) antenna table: the first ``nsky`` points of the
    48-point Fibonacci sky."""
    psrs = _case(npsr)[0]
    pos = np.stack([p.pos for p in psrs])
    sky = fibonacci_sky(48)[:nsky]
    ant = np.empty((nsky, npsr, 2))
    for k, (th, ph) in enumerate(sky):
        ant[k, :, 0], ant[k, :, 1] = gw_antenna_pattern(pos, th, ph)
    return ant


def _host_map(prods, ant):
    """(D, nsky, F) through the existing host assembly."""
    return np.stack([
        _assemble_fe_draws(prods, ant[k, :, 0], ant[k, :, 1])
        for k in range(ant.shape[0])
    ], axis=1)


def _dev(x):
    return torch.as_tensor(x, dtype=torch.float64).to(DEV)


# ----------------------------------------------------------------------
# CPU: the sky-maximised interface and the new keywords
# ----------------------------------------------------------------------
def test_fastfe_sweep_max_cpu_matches_sweep():
    psrs, noise, pta = _pta(5, seed=31)
    Nvecs, Ts, sigmas = get_mats_fp(pta, noise)
    freqs = np.linspace(5e-9, 4e-8, 7)
    sky = fibonacci_sky(48)
    fe = FastFe(psrs, pta)
    grid = fe.sweep(freqs, sky, Nvecs, Ts, sigmas, device="cpu")
    femax, argmax = fe.sweep_max(freqs, sky, Nvecs, Ts, sigmas, device="cpu")
    assert femax.shape == (7,) and argmax.shape == (7,)
    np.testing.assert_array_equal(femax, grid.max(axis=0))
    np.testing.assert_array_equal(argmax, np.argmax(grid, axis=0))


def test_nmfe_sweep_max_cpu_matches_sweep():
    psrs, pta, Nvecs, Ts, samples, _, freqs = _case(5)
    sky = fibonacci_sky(48)
    nm = NMFe(psrs, pta.rn_containers)
    cube = nm.sweep(freqs, sky, samples, Nvecs, Ts, device="cpu")
    femax, argmax = nm.sweep_max(freqs, sky, samples, Nvecs, Ts,
                                 device="cpu", draw_chunk=2)
    assert femax.shape == (5, 7) and argmax.shape == (5, 7)
    np.testing.assert_allclose(femax, cube.max(axis=1), rtol=1e-14)
    np.testing.assert_array_equal(argmax, np.argmax(cube, axis=1))
    assert argmax.min() >= 0 and argmax.max() < len(sky)


def test_assemble_device_on_cpu_raises():
    psrs, pta, Nvecs, Ts, samples, _, freqs = _case(5)
    sky = fibonacci_sky(48)[:3]
    nm = NMFe(psrs, pta.rn_containers)
    with pytest.raises(ValueError, match="assemble='device'"):
        nm.sweep(freqs, sky, samples, Nvecs, Ts, device="cpu",
                 assemble="device")
    psrs2, noise2, pta2 = _pta(5, seed=31)
    Nvecs2, Ts2, sigmas2 = get_mats_fp(pta2, noise2)
    with pytest.raises(ValueError, match="assemble='device'"):
        FastFe(psrs2, pta2).sweep(freqs, sky, Nvecs2, Ts2, sigmas2,
                                  device="cpu", assemble="device")
    # an explicit CPU engine is rejected as well, and so is a typo
    eng = FpEngine(psrs, Nvecs, Ts, device="cpu")
    eng.precompute(freqs)
    with pytest.raises(ValueError, match="assemble='device'"):
        nm.sweep(freqs, sky, samples, Nvecs, Ts, engine=eng,
                 assemble="device")
    with pytest.raises(ValueError, match="'host' or 'device'"):
        nm.sweep(freqs, sky, samples, Nvecs, Ts, device="cpu",
                 assemble="gpu")


def test_sweep_products_hip_cpu_engine_falls_back():
    """On an engine without the stacked HIP state the method IS
    ``sweep_products``."""
    psrs, pta, Nvecs, Ts, samples, phiinvs, freqs = _case(5)
    eng = FpEngine(psrs, Nvecs, Ts, device="cpu")
    eng.precompute(freqs)
    np.testing.assert_array_equal(
        eng.sweep_products_hip(phiinvs).numpy(), _cpu_products(5))


def _cli_inputs(tmp_path):
    """3-pulsar npz + noise json + fake chain (the tests/test_cli.py
    recipe)."""
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


def test_run_fe_skymax_cpu(tmp_path):
    from fastfp_amd.cli import run_fe

    psrfile, noisefile, _ = _cli_inputs(tmp_path)
    kw = dict(nfreqs=4, nsky=6, rn_comps=3, gwb_comps=3, device="cpu")
    run_fe.main(psrfile, noisefile, str(tmp_path / "mx"), skymax=True, **kw)
    femax = np.load(tmp_path / "mx.max.npy")
    argmax = np.load(tmp_path / "mx.argmax.npy")
    with open(tmp_path / "mx.json") as f:
        axes = json.load(f)
    assert sorted(axes) == ["freqs", "sky"] and len(axes["sky"]) == 6
    run_fe.main(psrfile, noisefile, str(tmp_path / "map"), **kw)
    with open(tmp_path / "map.json") as f:
        fmap = np.asarray(json.load(f)["fe"])  # (nsky, nfreqs)
    assert femax.shape == (4,) and argmax.shape == (4,)
    np.testing.assert_allclose(femax, fmap.max(axis=0), rtol=1e-12)
    np.testing.assert_array_equal(argmax, np.argmax(fmap, axis=0))


def test_run_nmfe_skymax_cpu(tmp_path):
    from fastfp_amd.cli import run_nmfe

    psrfile, noisefile, chainfile = _cli_inputs(tmp_path)
    kw = dict(inc_cp=True, nrncomps=3, ngwbcomps=3, ncwfreqs=4, nsamples=5,
              nsky=6, outdir=str(tmp_path), device="cpu", batch_size=2)
    run_nmfe.main(psrfile, noisefile, chainfile, "mx", skymax=True, **kw)
    femax = np.load(tmp_path / "mx.max.npy")
    argmax = np.load(tmp_path / "mx.argmax.npy")
    assert femax.shape == (5, 4) and np.isfinite(femax).all()
    assert argmax.shape == (5, 4)
    assert np.issubdtype(argmax.dtype, np.integer)
    assert argmax.min() >= 0 and argmax.max() < 6
    assert not (tmp_path / "mx.npy").exists()
    with open(tmp_path / "mx.meta.json") as f:
        meta = json.load(f)
    assert len(meta["freqs"]) == 4 and len(meta["sky"]) == 6
    # same seed, full cube: the maximum over its sky axis
    run_nmfe.main(psrfile, noisefile, chainfile, "cube", **kw)
    cube = np.load(tmp_path / "cube.npy")
    np.testing.assert_allclose(femax, cube.max(axis=1), rtol=1e-12)
    np.testing.assert_array_equal(argmax, np.argmax(cube, axis=1))


def test_run_nmfe_builds_engine_once(tmp_path, monkeypatch):
    """The frequency precompute does not depend on the draws: three
    batches share one engine."""
    from fastfp_amd import festat
    from fastfp_amd.cli import run_nmfe

    made = []

    class Counting(FpEngine):
        def __init__(self, *a, **k):
            made.append(1)
            super().__init__(*a, **k)

    monkeypatch.setattr(run_nmfe, "FpEngine", Counting)
    monkeypatch.setattr(festat, "FpEngine", Counting)
    psrfile, noisefile, chainfile = _cli_inputs(tmp_path)
    run_nmfe.main(psrfile, noisefile, chainfile, "once", inc_cp=True,
                  nrncomps=3, ngwbcomps=3, ncwfreqs=4, nsamples=5, nsky=3,
                  outdir=str(tmp_path), device="cpu", batch_size=2)
    assert np.load(tmp_path / "once.npy").shape == (5, 3, 4)
    assert len(made) == 1


# ----------------------------------------------------------------------
# GPU: products mode of the solve
# ----------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize(
    "rn_comps,F,D",
    [(3, 7, 5),     # m = 9  -> NBT = 1
     (8, 130, 3)],  # m = 19 -> NBT = 2; 3 frequency tiles of 63, ragged
)
def test_sweep_products_hip_matches_torch(rn_comps, F, D):
    psrs, pta, Nvecs, Ts, samples, phiinvs, freqs = _case(
        5, rn_comps=rn_comps, F=F, D=D)
    assert Ts[0].shape[1] == 3 + 2 * rn_comps
    eng = FpEngine(psrs, Nvecs, Ts, device=DEV)
    eng.precompute(freqs)
    assert eng._direct_stack is not None
    want = eng.sweep_products(phiinvs=phiinvs).cpu().numpy()
    # draw_chunk=2: full chunks plus a one-draw tail
    got_t = eng.sweep_products_hip(phiinvs, draw_chunk=2)
    assert got_t.is_cuda and got_t.shape == (5, D, 5, F)
    got = got_t.cpu().numpy()
    for i, name in enumerate(["ss", "cc", "sc", "sr", "cr"]):
        # sc / sr / cr cross zero: absolute floor from the plane's scale
        atol = 0.0 if i < 2 else RTOL * np.abs(want[:, :, i]).max()
        err = np.abs(got[:, :, i] - want[:, :, i]).max()
        print(f"{name}: max abs err {err:.3e}, "
              f"plane max {np.abs(want[:, :, i]).max():.3e}")
        np.testing.assert_allclose(got[:, :, i], want[:, :, i], rtol=RTOL,
                                   atol=atol, err_msg=name)
    # single chunk and fixed-noise (m,) forms
    np.testing.assert_array_equal(
        eng.sweep_products_hip(phiinvs, draw_chunk=32).cpu().numpy(), got)
    fixed = eng.sweep_products_hip([p[1] for p in phiinvs])
    assert fixed.shape == (5, 5, F)
    np.testing.assert_array_equal(fixed.cpu().numpy(), got[:, 1])


# ----------------------------------------------------------------------
# GPU: sky-assembly kernels
# ----------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("npsr", [5, 9])   # neither a multiple of 4
@pytest.mark.parametrize("nsky", [48, 5])  # 5: a partial sky tile
def test_fe_assemble_matches_host(npsr, nsky):
    from fastfp_amd import ops

    prods, ant = _cpu_products(npsr), _ant(npsr, nsky)
    want = _host_map(prods, ant)
    got = ops.fe_assemble(_dev(prods), _dev(ant), repair=False)
    assert got.shape == (5, nsky, 7)
    got = got.cpu().numpy()
    assert np.isfinite(got).all()
    print(f"max rel err {np.abs(got / want - 1).max():.3e}")
    np.testing.assert_allclose(got, want, rtol=RTOL)


@pytest.mark.gpu
@pytest.mark.parametrize("npsr", [5, 9])
@pytest.mark.parametrize("nsky", [48, 5])
def test_fe_skymax_matches_device_map(npsr, nsky):
    from fastfp_amd import ops

    prods, ant = _dev(_cpu_products(npsr)), _dev(_ant(npsr, nsky))
    fmap = ops.fe_assemble(prods, ant, repair=False).cpu().numpy()
    femax, argmax, nskip = ops.fe_skymax(prods, ant, repair=False)
    assert femax.dtype == torch.float64
    assert argmax.dtype == torch.int32 and nskip.dtype == torch.int32
    np.testing.assert_array_equal(femax.cpu().numpy(), fmap.max(axis=1))
    np.testing.assert_array_equal(argmax.cpu().numpy(),
                                  np.argmax(fmap, axis=1))
    assert int(nskip.abs().sum()) == 0
    again = ops.fe_skymax(prods, ant, repair=False)
    for a, b in zip((femax, argmax, nskip), again):
        assert torch.equal(a, b)


@pytest.mark.gpu
def test_fe_singular_sky_row_repaired_on_host():
    """One sky row with Fx = 0 for every pulsar: M is rank 2 there.  The
    kernel skips it; the wrappers repair through the host assembly."""
    from fastfp_amd import ops

    prods = _cpu_products(5)
    ant = _ant(5, 48).copy()
    row = 7
    ant[row, :, 1] = 0.0
    want = _host_map(prods, ant)
    assert np.isfinite(want).all()
    prods_d, ant_d = _dev(prods), _dev(ant)

    raw = ops.fe_assemble(prods_d, ant_d, repair=False).cpu().numpy()
    assert np.isnan(raw[:, row, :]).all()
    assert np.isfinite(np.delete(raw, row, axis=1)).all()
    got = ops.fe_assemble(prods_d, ant_d).cpu().numpy()
    assert np.isfinite(got).all()
    np.testing.assert_allclose(got[:, row, :], want[:, row, :], rtol=RTOL)
    np.testing.assert_allclose(got, want, rtol=RTOL)

    _, _, nskip = ops.fe_skymax(prods_d, ant_d, repair=False)
    assert int(nskip.min()) >= 1
    femax, argmax, _ = ops.fe_skymax(prods_d, ant_d)
    np.testing.assert_allclose(femax.cpu().numpy(), want.max(axis=1),
                               rtol=RTOL)
    np.testing.assert_array_equal(argmax.cpu().numpy(),
                                  np.argmax(want, axis=1))


def _synthetic_products(P, D=5, F=7, nsky=20, seed=3):
    """Well-posed random inputs for pulsar counts the synthetic-array
    cases do not reach: positive-definite per-pulsar 2x2 blocks
    [[ss, sc], [sc, cc]] and a random antenna table, so every 4x4 M is
    a sum of P >> 4 independent positive-definite terms."""
    rng = np.random.default_rng(seed)
    prods = np.empty((P, D, 5, F))
    prods[:, :, 0:2] = rng.uniform(1.0, 2.0, (P, D, 2, F))
    prods[:, :, 2] = 0.1 * rng.normal(size=(P, D, F))
    prods[:, :, 3:] = rng.normal(size=(P, D, 2, F))
    return prods, rng.normal(size=(nsky, P, 2))


@pytest.mark.gpu
@pytest.mark.parametrize(
    "P",
    [80,    # first K-padded size whose product tile exceeds 48 KB of LDS
     248],  # the largest resident tile (one block per CU)
)
def test_fe_kernels_large_pulsar_count(P):
    """The product tile lives in dynamic LDS sized by P; above 48 KB the
    launcher raises the kernel's dynamic-LDS limit first."""
    from fastfp_amd import ops

    prods, ant = _synthetic_products(P)
    want = _host_map(prods, ant)
    prods_d, ant_d = _dev(prods), _dev(ant)
    got = ops.fe_assemble(prods_d, ant_d, repair=False).cpu().numpy()
    print(f"P={P}: max rel err {np.abs(got / want - 1).max():.3e}")
    np.testing.assert_allclose(got, want, rtol=RTOL)
    femax, argmax, nskip = ops.fe_skymax(prods_d, ant_d, repair=False)
    np.testing.assert_array_equal(femax.cpu().numpy(), got.max(axis=1))
    np.testing.assert_array_equal(argmax.cpu().numpy(),
                                  np.argmax(got, axis=1))
    assert int(nskip.abs().sum()) == 0


@pytest.mark.gpu
def test_fe_kernels_reject_too_many_pulsars():
    from fastfp_amd import ops

    prods, ant = _synthetic_products(249, D=1, F=2, nsky=2)
    with pytest.raises(RuntimeError, match="248"):
        ops.fe_assemble(_dev(prods), _dev(ant))
    with pytest.raises(RuntimeError, match="248"):
        ops.fe_skymax(_dev(prods), _dev(ant))


@pytest.mark.gpu
def test_trsm_prods_rejects_large_mp():
    from fastfp_amd.ops import _fastfp_hip as ext

    D, F, mp = 1, 2, 144
    z = lambda *s: torch.zeros(s, dtype=torch.float64, device=DEV)  # noqa: E731
    with pytest.raises(RuntimeError, match="mp <= 128"):
        ext.trsm_prods(z(D, mp, mp), z(D, mp // 16, 16, 16), z(mp, 2 * F + 1),
                       z(3, F), z(2, F), z(D, 5, F), 1.0)


# ----------------------------------------------------------------------
# GPU: end to end
# ----------------------------------------------------------------------
@pytest.mark.gpu
def test_nmfe_device_paths_match_cpu():
    psrs, pta, Nvecs, Ts, samples, _, freqs = _case(5)
    sky = fibonacci_sky(48)
    nm = NMFe(psrs, pta.rn_containers)
    want = nm.sweep(freqs, sky, samples, Nvecs, Ts, device="cpu")
    got = nm.sweep(freqs, sky, samples, Nvecs, Ts, device=DEV,
                   assemble="device", draw_chunk=2)
    assert got.shape == (5, 48, 7)
    print(f"map max rel err {np.abs(got / want - 1).max():.3e}")
    np.testing.assert_allclose(got, want, rtol=RTOL)
    femax, argmax = nm.sweep_max(freqs, sky, samples, Nvecs, Ts, device=DEV,
                                 draw_chunk=2)
    assert femax.shape == (5, 7) and argmax.shape == (5, 7)
    np.testing.assert_allclose(femax, want.max(axis=1), rtol=RTOL)
    np.testing.assert_array_equal(argmax, np.argmax(want, axis=1))


@pytest.mark.gpu
def test_fastfe_device_paths_match_cpu():
    psrs, noise, pta = _pta(5, seed=31)
    Nvecs, Ts, sigmas = get_mats_fp(pta, noise)
    freqs = np.linspace(5e-9, 4e-8, 7)
    sky = fibonacci_sky(48)
    fe = FastFe(psrs, pta)
    want = fe.sweep(freqs, sky, Nvecs, Ts, sigmas, device="cpu")
    got = fe.sweep(freqs, sky, Nvecs, Ts, sigmas, device=DEV,
                   assemble="device")
    np.testing.assert_allclose(got, want, rtol=RTOL)
    femax, argmax = fe.sweep_max(freqs, sky, Nvecs, Ts, sigmas, device=DEV)
    np.testing.assert_allclose(femax, want.max(axis=0), rtol=RTOL)
    np.testing.assert_array_equal(argmax, np.argmax(want, axis=0))
