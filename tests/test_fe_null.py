"""Monte-Carlo null distribution of the Fe sky maximum: the host
reference ``_null_max_host``, the covariance identity behind it,
``FastFe.null_max`` / ``FastFe.false_alarm`` / ``NMFe.null_max``, the
``--null`` CLI flag and the ``fe_null_skymax`` kernel.

Tolerances.  Every Fe value is compared at the project's Fe tolerance
rtol = 1e-9 (tests/test_festat.py).  The device inputs are the synthetic
products of tests/test_fe_device.py (positive-definite 2x2 blocks, every
4x4 M a sum of independent positive-definite terms), so an fp64 LDL^T
sits orders below that bound; the realisations n = L z enter Fe through a
well-conditioned solve, and the one rounding by which the kernel's fused
n_c differs from the host's is far below it too.  A device argmax that
differs from the host's passes only if the HOST Fe at the device's index
is within rtol of the host maximum (a near-tie); no share of points is
exempt otherwise.
"""

import functools
import json
import sys

import numpy as np
import pytest
import torch

from fastfp_amd import (
    FastFe,
    FpEngine,
    NMFe,
    false_alarm_probability,
    initialize_pta,
    inject_earth_term_cw,
    make_synthetic_pta,
)
from fastfp_amd.cli.run_fe import fibonacci_sky
from fastfp_amd.festat import (
    _assemble_fe_draws,
    _null_draws,
    _null_max_host,
)
from fastfp_amd.model import get_mats_fp, get_mats_nmfp
from fastfp_amd.noise import batch_phiinv

RTOL = 1e-9
SEEDS = {5: 31, 9: 32}
DEV = "cuda:0"
INJ = dict(zeta=3e-7, cosi=0.3, psi=0.4, phi0=1.1)
INJ_SKY = (1.0, 2.0)
INJ_SCALE = 3.0


# ----------------------------------------------------------------------
# shared inputs (the recipes of tests/test_fe_amplitudes.py)
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


def _synthetic_products(P, D=5, F=7, nsky=20, seed=3):
    """Well-posed random inputs: positive-definite per-pulsar 2x2 blocks
    and a random antenna table."""
    rng = np.random.default_rng(seed)
    prods = np.empty((P, D, 5, F))
    prods[:, :, 0:2] = rng.uniform(1.0, 2.0, (P, D, 2, F))
    prods[:, :, 2] = 0.1 * rng.normal(size=(P, D, F))
    prods[:, :, 3:] = rng.normal(size=(P, D, 2, F))
    return prods, rng.normal(size=(nsky, P, 2))


def _normals(P, D, F, R, seed=7):
    return np.random.default_rng(seed).standard_normal((D, F, P, 2, R))


def _dev(x):
    return torch.as_tensor(x, dtype=torch.float64).to(DEV)


def _substituted(prods, z):
    """(R, P, D, 5, F): ``prods`` with realisation r of ``n = L z`` in the
    planes sr, cr."""
    ns, nc = _null_draws(prods, z)  # (P, D, F, R)
    out = np.repeat(prods[None], z.shape[-1], axis=0)
    out[:, :, :, 3] = np.moveaxis(ns, 3, 0)
    out[:, :, :, 4] = np.moveaxis(nc, 3, 0)
    return out


def _loop_max(prods, ant, z):
    """The obvious loop: per realisation and sky point one
    ``_assemble_fe_draws`` call, then nanmax / nanargmax."""
    sub = _substituted(prods, z)
    fm, am = [], []
    for r in range(z.shape[-1]):
        grid = np.stack([_assemble_fe_draws(sub[r], ant[k, :, 0], ant[k, :, 1])
                         for k in range(ant.shape[0])])
        fm.append(np.nanmax(grid, axis=0))
        am.append(np.nanargmax(grid, axis=0))
    return np.stack(fm), np.stack(am)


# ----------------------------------------------------------------------
# 1. CPU: statistics of the host reference
# ----------------------------------------------------------------------
def test_host_null_statistics():
    """One sky point: 2 Fe ~ chi2(4) in both columns (measured: means
    3.985 / 4.034, KS p = 0.91 / 0.78).  Twenty sky points: the mean of
    the maximum rises (measured 9.11), the trials factor."""
    from scipy import stats

    prods, ant = _synthetic_products(5, D=1, F=2, nsky=1)
    z = _normals(5, 1, 2, 4000)
    femax, argmax = _null_max_host(prods, ant, z)
    assert femax.shape == (4000, 1, 2) and argmax.shape == (4000, 1, 2)
    assert (argmax == 0).all()
    single = []
    for f in range(2):
        x = 2.0 * femax[:, 0, f]
        p = stats.kstest(x, "chi2", args=(4,)).pvalue
        print(f"column (0, {f}): mean {x.mean():.3f} var {x.var():.2f} "
              f"KS p {p:.3f}")
        assert p > 0.01
        single.append(x.mean())
    prods, ant = _synthetic_products(9, D=1, F=2, nsky=20)
    femax, _ = _null_max_host(prods, ant, _normals(9, 1, 2, 4000))
    many = (2.0 * femax).mean(axis=0)[0]
    print(f"mean of 2 femax over 20 sky points: {many}")
    assert (many > max(single)).all()


# ----------------------------------------------------------------------
# 2. CPU: the host reference against the obvious loop
# ----------------------------------------------------------------------
def test_host_matches_loop():
    prods, ant = _synthetic_products(9, D=2, F=3, nsky=20)
    z = _normals(9, 2, 3, 33, seed=11)
    femax, argmax = _null_max_host(prods, ant, z)
    want, warg = _loop_max(prods, ant, z)
    assert femax.shape == (33, 2, 3)
    print(f"host vs loop: {np.abs(femax / want - 1).max():.3e}")
    np.testing.assert_allclose(femax, want, rtol=RTOL)
    np.testing.assert_array_equal(argmax, warg)


def test_host_degenerate_sky_is_pinv():
    """A sky row with Fx = 2 F+ in every pulsar: M is singular, the host
    reference takes the pseudo-inverse there as ``_assemble_fe_draws``
    does; duplicate rows resolve to the lower index."""
    prods, ant = _synthetic_products(9, D=2, F=3, nsky=6)
    ant[2, :, 1] = 2.0 * ant[2, :, 0]
    ant[5] = ant[1]
    z = _normals(9, 2, 3, 8, seed=12)
    femax, argmax = _null_max_host(prods, ant, z)
    want, warg = _loop_max(prods, ant, z)
    assert np.isfinite(femax).all()
    np.testing.assert_allclose(femax, want, rtol=RTOL)
    np.testing.assert_array_equal(argmax, warg)
    assert (argmax != 5).all()
    only, _ = _null_max_host(prods, ant[2:3], z)
    sub = _substituted(prods, z)
    for r in range(8):
        np.testing.assert_allclose(
            only[r], _assemble_fe_draws(sub[r], ant[2, :, 0], ant[2, :, 1]),
            rtol=RTOL)


# ----------------------------------------------------------------------
# 3. CPU: the products ARE the covariance of (sr, cr)
# ----------------------------------------------------------------------
def test_products_are_the_covariance():
    """``S^T C^-1 S = [[ss, sc], [sc, cc]]`` with the dense ``C = diag(N)
    + T diag(phi) T^T`` of tests/oracle.py, on the 5-pulsar case, every
    draw and frequency.

    The timing-model columns carry the production prior phi = 1e40, at
    which a direct fp64 solve of the dense C returns nothing
    (``oracle.dense_xCy`` on this case: relative error 1.0 in every
    entry, cond(C) ~ 1e52 — the restriction tests/test_festat.py notes).
    The SAME C is therefore inverted through the Woodbury identity on its
    timing-model block alone: ``C = Cr + U diag(phi_tm) U^T`` with the
    dense ``Cr = diag(N) + Fb diag(phi_rn) Fb^T`` (condition number ~5)
    solved directly.  Measured against the CPU engine: 2.5e-13."""
    psrs, pta, Nvecs, Ts, samples, phiinvs, freqs = _case(5)
    eng = FpEngine(psrs, Nvecs, Ts, device="cpu")
    eng.precompute(freqs)
    prods = eng.sweep_products(phiinvs=phiinvs).numpy()  # (P, D, 5, F)
    F = len(freqs)
    worst = 0.0
    for p, psr in enumerate(psrs):
        T, N = np.asarray(Ts[p]), np.asarray(Nvecs[p])
        arg = 2.0 * np.pi * freqs[None, :] * np.asarray(psr.toas)[:, None]
        S = np.concatenate([np.sin(arg), np.cos(arg)], axis=1)
        for d in range(prods.shape[1]):
            phi = 1.0 / phiinvs[p][d].numpy()
            tm = phi > 1e30
            assert tm.sum() == 3
            U, Fb = T[:, tm], T[:, ~tm]
            Cr = np.diag(N) + Fb @ np.diag(phi[~tm]) @ Fb.T
            X = np.linalg.solve(Cr, np.concatenate([S, U], axis=1))
            CS, CU = X[:, :2 * F], X[:, 2 * F:]
            K = np.diag(1.0 / phi[tm]) + U.T @ CU
            B = S.T @ CS - (S.T @ CU) @ np.linalg.solve(K, CU.T @ S)
            j = np.arange(F)
            got = np.stack([B[j, j], B[F + j, F + j], B[j, F + j]])
            worst = max(worst, np.abs(got / prods[p, d, :3] - 1).max())
            np.testing.assert_allclose(got, prods[p, d, :3], rtol=RTOL)
            np.testing.assert_allclose(B, B.T, rtol=0,
                                       atol=1e-12 * np.abs(B).max())
    print(f"S^T C^-1 S vs engine products: {worst:.3e}")


# ----------------------------------------------------------------------
# 4. CPU: FastFe.null_max / NMFe.null_max
# ----------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _fixed_noise(inject):
    """5-pulsar array, 7 frequencies, CPU engine; ``inject``: the INJ
    signal scaled by INJ_SCALE at grid point 3."""
    psrs = make_synthetic_pta(npsr=5, ntoa=80, ntm=3, seed=31)
    freqs = np.linspace(5e-9, 4e-8, 7)
    if inject:
        inject_earth_term_cw(psrs, freqs[3], *INJ_SKY,
                             **dict(INJ, zeta=INJ_SCALE * INJ["zeta"]))
    noise = _noise(psrs)
    pta = initialize_pta(psrs, noise, inc_cp=True, rn_comps=3, gwb_comps=3)
    Nvecs, Ts, sigmas = get_mats_fp(pta, noise)
    eng = FpEngine(psrs, Nvecs, Ts, device="cpu")
    eng.precompute(freqs)
    return psrs, pta, Nvecs, Ts, sigmas, freqs, eng


def test_fastfe_null_max_cpu():
    psrs, pta, Nvecs, Ts, sigmas, freqs, eng = _fixed_noise(False)
    sky = fibonacci_sky(20)
    fe = FastFe(psrs, pta)
    args = (freqs, sky, Nvecs, Ts, sigmas)
    a = fe.null_max(*args, 40, seed=5, engine=eng)
    assert a.shape == (40, 7) and a.dtype == np.float64
    assert np.isfinite(a).all() and (a > 0).all()
    np.testing.assert_array_equal(a, fe.null_max(*args, 40, seed=5,
                                                 engine=eng))
    # an engine built inside gives the same numbers
    np.testing.assert_array_equal(a, fe.null_max(*args, 40, seed=5,
                                                 device="cpu"))
    b = fe.null_max(*args, 40, seed=6, engine=eng)
    assert (a != b).all()
    # real_chunk is part of the stream: one randn call per chunk
    c = fe.null_max(*args, 40, seed=5, engine=eng, real_chunk=16)
    assert not np.array_equal(a, c)
    # explicit normals: bitwise independent of real_chunk
    z = torch.as_tensor(_normals(5, 1, 7, 40, seed=9))
    e = fe.null_max(*args, 40, engine=eng, z=z)
    for chunk in (1, 16, 17, 64):
        np.testing.assert_array_equal(
            e, fe.null_max(*args, 40, engine=eng, z=z, real_chunk=chunk))
    with pytest.raises(ValueError, match="z must be"):
        fe.null_max(*args, 39, engine=eng, z=z)
    # the host reference on the engine's products is what it returns
    prods = eng.sweep_products(sigmas=sigmas).numpy()[:, None]
    from fastfp_amd.festat import _antenna_table

    want, _ = _null_max_host(prods, _antenna_table(fe.pos, sky), z.numpy())
    np.testing.assert_array_equal(e, want[:, 0])


def test_nmfe_null_max_cpu():
    psrs, pta, Nvecs, Ts, samples, phiinvs, freqs = _case(5)
    sky = fibonacci_sky(12)
    nm = NMFe(psrs, pta.rn_containers)
    a = nm.null_max(freqs, sky, samples, Nvecs, Ts, 10, seed=3, device="cpu",
                    draw_chunk=2, real_chunk=4)
    assert a.shape == (10, 5, 7) and np.isfinite(a).all()
    b = nm.null_max(freqs, sky, samples, Nvecs, Ts, 10, seed=3, device="cpu",
                    draw_chunk=2, real_chunk=4)
    np.testing.assert_array_equal(a, b)
    c = nm.null_max(freqs, sky, samples, Nvecs, Ts, 10, seed=4, device="cpu",
                    draw_chunk=2, real_chunk=4)
    assert (a != c).all()
    # the first draw chunk sees the generator's first normals: that slice
    # is FastFe-style reproducible from the same products
    eng = FpEngine(psrs, Nvecs, Ts, device="cpu")
    eng.precompute(freqs)
    prods = eng.sweep_products(phiinvs=[p[:2] for p in phiinvs]).numpy()
    gen = torch.Generator(device="cpu")
    gen.manual_seed(3)
    z = torch.cat([torch.randn((2, 7, 5, 2, n), generator=gen,
                               dtype=torch.float64) for n in (4, 4, 2)],
                  dim=-1)
    from fastfp_amd.festat import _antenna_table

    want, _ = _null_max_host(prods, _antenna_table(nm.fe.pos, sky), z.numpy())
    np.testing.assert_array_equal(a[:, :2], want)


# ----------------------------------------------------------------------
# 5. CPU: FastFe.false_alarm
# ----------------------------------------------------------------------
def test_false_alarm_cpu():
    """INJ scaled by INJ_SCALE = 3.0 at grid point 3: measured on the CPU
    (seed 0, 199 realisations, 20 sky points) the observed femax there is
    20.7 against a largest null value of 9.43, so pfa = 1/200.  Without
    the injection the smallest pfa over the 7 frequencies is 5/200 for
    this seed (a fixed-seed fact, not a statistical guarantee)."""
    sky = fibonacci_sky(20)
    psrs, pta, Nvecs, Ts, sigmas, freqs, eng = _fixed_noise(True)
    fe = FastFe(psrs, pta)
    args = (freqs, sky, Nvecs, Ts, sigmas)
    femax, argmax, pfa = fe.false_alarm(*args, 199, seed=0, engine=eng)
    assert femax.shape == argmax.shape == pfa.shape == (7,)
    wmax, warg = fe.sweep_max(*args, engine=eng)
    np.testing.assert_array_equal(femax, wmax)
    np.testing.assert_array_equal(argmax, warg)
    null = fe.null_max(*args, 199, seed=0, engine=eng)
    print(f"femax {femax}\nnull max {null.max(axis=0)}\npfa*200 {pfa * 200}")
    assert femax[3] > null[:, 3].max()
    assert pfa[3] == 1.0 / 200.0
    want = (1.0 + (null >= femax[None]).sum(axis=0)) / 200.0
    np.testing.assert_array_equal(pfa, want)
    np.testing.assert_array_equal(pfa, false_alarm_probability(femax, null))

    psrs, pta, Nvecs, Ts, sigmas, freqs, eng = _fixed_noise(False)
    fe = FastFe(psrs, pta)
    _, _, pfa0 = fe.false_alarm(freqs, sky, Nvecs, Ts, sigmas, 199, seed=0,
                                engine=eng)
    print(f"noise only: pfa*200 {pfa0 * 200}")
    assert (pfa0 >= 2.0 / 200.0).all() and (pfa0 <= 1.0).all()


# ----------------------------------------------------------------------
# 6. CPU: blocks that are no covariance
# ----------------------------------------------------------------------
def test_not_positive_definite_raises():
    prods, ant = _synthetic_products(5, D=2, F=3, nsky=4)
    z = _normals(5, 2, 3, 4)
    _null_max_host(prods, ant, z)
    bad = prods.copy()
    bad[3, 1, 1, 2] = 0.5 * bad[3, 1, 2, 2] ** 2 / bad[3, 1, 0, 2]
    with pytest.raises(ValueError,
                       match=r"pulsar 3, draw 1, frequency 2.*positive"):
        _null_max_host(bad, ant, z)
    bad = prods.copy()
    bad[4, 0, 0, 1] = -1.0
    bad[4, 1, 0, 1] = np.nan  # the first offender is named
    with pytest.raises(ValueError, match="pulsar 4, draw 0, frequency 1"):
        _null_max_host(bad, ant, z)
    bad = prods.copy()
    bad[0, 0, 1, 0] = np.inf
    with pytest.raises(ValueError, match="pulsar 0, draw 0, frequency 0"):
        _null_max_host(bad, ant, z)


# ----------------------------------------------------------------------
# 7. CLI
# ----------------------------------------------------------------------
def _cli_inputs(tmp_path):
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
    return psrfile, noisefile


CLI_KW = dict(nfreqs=4, nsky=6, rn_comps=3, gwb_comps=3, device="cpu",
              skymax=True)


def test_run_fe_null_cli(tmp_path):
    from fastfp_amd.cli import run_fe

    psrfile, noisefile = _cli_inputs(tmp_path)
    run_fe.main(psrfile, noisefile, str(tmp_path / "a"), null=16, **CLI_KW)
    run_fe.main(psrfile, noisefile, str(tmp_path / "b"), **CLI_KW)
    assert not (tmp_path / "b.null.npy").exists()
    assert not (tmp_path / "b.pfa.npy").exists()
    np.testing.assert_array_equal(np.load(tmp_path / "a.max.npy"),
                                  np.load(tmp_path / "b.max.npy"))
    null = np.load(tmp_path / "a.null.npy")
    pfa = np.load(tmp_path / "a.pfa.npy")
    assert null.shape == (16, 4) and np.isfinite(null).all()
    assert pfa.shape == (4,) and (pfa > 0).all() and (pfa <= 1).all()
    np.testing.assert_array_equal(
        pfa, false_alarm_probability(np.load(tmp_path / "a.max.npy"), null))
    run_fe.main(psrfile, noisefile, str(tmp_path / "c"), null=16,
                null_seed=1, **CLI_KW)
    assert (np.load(tmp_path / "c.null.npy") != null).all()


def test_cli_null_needs_skymax(monkeypatch, capsys):
    from fastfp_amd.cli import run_fe

    monkeypatch.setattr(sys, "argv", ["run_fe", "x", "x", "x", "--null", "16"])
    with pytest.raises(SystemExit) as exc:
        run_fe.cli()
    assert exc.value.code == 2
    assert "--null requires --skymax" in capsys.readouterr().err
    with pytest.raises(ValueError, match="skymax"):
        run_fe.main("x", "x", "x", null=16)


# ----------------------------------------------------------------------
# GPU: ops.fe_null_skymax against _null_max_host on the same z
# ----------------------------------------------------------------------
def _assert_matches_host(got_max, got_arg, prods, ant, z, what=""):
    """femax at rtol; argmax equal or a near-tie on the host."""
    want, warg = _null_max_host(prods, ant, z)
    got_max, got_arg = got_max.cpu().numpy(), got_arg.cpu().numpy()
    assert got_max.shape == want.shape and got_arg.shape == warg.shape
    err = np.abs(got_max / want - 1).max()
    diff = np.argwhere(got_arg != warg)
    print(f"{what}: max rel err {err:.3e}, {len(diff)} argmax differences")
    np.testing.assert_allclose(got_max, want, rtol=RTOL)
    for r, d, f in diff:
        k = int(got_arg[r, d, f])
        assert 0 <= k < ant.shape[0]
        at, _ = _null_max_host(prods[:, d:d + 1, :, f:f + 1], ant[k:k + 1],
                               z[d:d + 1, f:f + 1, :, :, r:r + 1])
        assert abs(at[0, 0, 0] / want[r, d, f] - 1) <= RTOL, (r, d, f, k)


SHAPES = [  # (P, R, nsky): every value of every axis
    (1, 1, 1), (1, 16, 17), (5, 17, 70), (5, 70, 1), (5, 16, 1),
    (9, 1, 17), (9, 16, 70), (9, 70, 17), (67, 17, 1), (67, 1, 70),
    (67, 16, 17), (67, 70, 70),
]


@pytest.mark.gpu
@pytest.mark.parametrize("P,R,nsky", SHAPES)
def test_fe_null_skymax_shapes(P, R, nsky):
    from fastfp_amd import ops

    prods, ant = _synthetic_products(P, nsky=nsky)
    z = _normals(P, 5, 7, R)
    femax, argmax, nskip = ops.fe_null_skymax(_dev(prods), _dev(ant), _dev(z))
    assert femax.shape == (R, 5, 7) and femax.dtype == torch.float64
    assert argmax.shape == (R, 5, 7) and argmax.dtype == torch.int32
    assert nskip.shape == (5, 7) and nskip.dtype == torch.int32
    # one pulsar: M has rank 2, every point is degenerate and repaired
    assert (nskip.cpu().numpy() == (nsky if P == 1 else 0)).all()
    _assert_matches_host(femax, argmax, prods, ant, z, f"P={P} R={R} "
                                                       f"nsky={nsky}")


@pytest.mark.gpu
@pytest.mark.parametrize("P", [9, 67])
def test_fe_null_skymax_matches_fe_skymax(P):
    """The route of the existing kernel: products replicated per
    realisation with n in the planes sr, cr."""
    from fastfp_amd import ops

    R, nsky = 17, 20
    prods, ant = _synthetic_products(P, nsky=nsky)
    ant[4, :, 1] = 2.0 * ant[4, :, 0]  # one skipped row in every column
    z = _normals(P, 5, 7, R)
    sub = _substituted(prods, z)  # (R, P, D, 5, F)
    rep = np.ascontiguousarray(
        np.moveaxis(sub, 0, 2).reshape(P, 5 * R, 5, 7))  # draw d * R + r
    wmax, warg, wskip = ops.fe_skymax(_dev(rep), _dev(ant), repair=False)
    femax, argmax, nskip = ops.fe_null_skymax(_dev(prods), _dev(ant), _dev(z),
                                              repair=False)
    wmax = wmax.reshape(5, R, 7).permute(1, 0, 2).cpu().numpy()
    warg = warg.reshape(5, R, 7).permute(1, 0, 2).cpu().numpy()
    wskip = wskip.reshape(5, R, 7).cpu().numpy()
    got = femax.cpu().numpy()
    print(f"P={P}: vs fe_skymax {np.abs(got / wmax - 1).max():.3e}")
    np.testing.assert_allclose(got, wmax, rtol=RTOL)
    assert (wskip == 1).all()
    np.testing.assert_array_equal(
        wskip, np.broadcast_to(nskip.cpu().numpy()[:, None, :], wskip.shape))
    # argmax: equal, or a near-tie in the existing kernel's own map
    garg = argmax.cpu().numpy()
    diff = np.argwhere(garg != warg)
    if len(diff):
        fmap = ops.fe_assemble(_dev(rep), _dev(ant), repair=False)
        fmap = fmap.reshape(5, R, nsky, 7).cpu().numpy()
        for r, d, f in diff:
            assert abs(fmap[d, r, garg[r, d, f], f] / wmax[r, d, f] - 1) \
                <= RTOL


@pytest.mark.gpu
def test_fe_null_skymax_degenerate_skies():
    from fastfp_amd import ops

    P, R, nsky = 9, 17, 20
    prods, ant = _synthetic_products(P, nsky=nsky)
    for row in (3, 11, 18):
        ant[row, :, 1] = 2.0 * ant[row, :, 0]
    ant[9] = ant[6]  # duplicates: the lower index wins
    ant[16] = ant[6]
    z = _normals(P, 5, 7, R)
    args = (_dev(prods), _dev(ant), _dev(z))
    _, _, wskip = ops.fe_skymax(args[0], args[1], repair=False)
    raw_max, raw_arg, nskip = ops.fe_null_skymax(*args, repair=False)
    assert torch.equal(nskip, wskip) and int(nskip.min()) == 3 \
        and int(nskip.max()) == 3
    raw_arg = raw_arg.cpu().numpy()
    assert not np.isin(raw_arg, (3, 11, 18, 9, 16)).any()
    # without repair: the maximum over the points that were kept
    keep = np.delete(np.arange(nsky), (3, 11, 18))
    want, warg = _null_max_host(prods, ant[keep], z)
    np.testing.assert_allclose(raw_max.cpu().numpy(), want, rtol=RTOL)
    # with repair: the host pseudo-inverse route over ALL sky points
    femax, argmax, nskip2 = ops.fe_null_skymax(*args)
    assert torch.equal(nskip2, nskip)
    _assert_matches_host(femax, argmax, prods, ant, z, "repaired")
    loop_max, loop_arg = _loop_max(prods, ant, z)
    np.testing.assert_allclose(femax.cpu().numpy(), loop_max, rtol=RTOL)
    assert not np.isin(argmax.cpu().numpy(), (9, 16)).any()
    # every row degenerate
    allbad = ant.copy()
    allbad[:, :, 1] = 2.0 * allbad[:, :, 0]
    femax, argmax, nskip = ops.fe_null_skymax(args[0], _dev(allbad), args[2],
                                              repair=False)
    assert (nskip.cpu().numpy() == nsky).all()
    assert torch.isinf(femax).all() and (femax < 0).all()
    assert (argmax == -1).all()


@pytest.mark.gpu
def test_fe_null_skymax_bitwise():
    """A realisation's result does not depend on the tile, the block or
    the tiles per block it lands in."""
    from fastfp_amd import ops

    P, nsky = 9, 70
    prods, ant = _synthetic_products(P, nsky=nsky)
    z = _dev(_normals(P, 5, 7, 70))
    prods_d, ant_d = _dev(prods), _dev(ant)
    a = ops.fe_null_skymax(prods_d, ant_d, z, repair=False)
    b = ops.fe_null_skymax(prods_d, ant_d, z, repair=False)
    for x, y in zip(a, b):
        assert torch.equal(x, y)
    parts = [ops.fe_null_skymax(prods_d, ant_d, z[..., lo:hi].contiguous(),
                                repair=False)
             for lo, hi in ((0, 16), (16, 33), (33, 70))]
    assert torch.equal(a[0], torch.cat([p[0] for p in parts], dim=0))
    assert torch.equal(a[1], torch.cat([p[1] for p in parts], dim=0))
    for p in parts:
        assert torch.equal(p[2], a[2])
    for rtiles in (1, 2, 4):
        c = ops.fe_null_skymax(prods_d, ant_d, z, repair=False, rtiles=rtiles)
        for x, y in zip(a, c):
            assert torch.equal(x, y)


@pytest.mark.gpu
def test_fe_null_skymax_rejects_bad_inputs():
    from fastfp_amd import ops

    cap = ops.fe_max_pulsars()
    prods, ant = _synthetic_products(cap + 1, D=1, F=2, nsky=2)
    z = _normals(cap + 1, 1, 2, 3)
    with pytest.raises(RuntimeError, match=str(cap)):
        ops.fe_null_skymax(_dev(prods), _dev(ant), _dev(z))
    prods, ant = _synthetic_products(5, nsky=4)
    prods_d, ant_d = _dev(prods), _dev(ant)
    z = _dev(_normals(5, 5, 7, 6))
    ops.fe_null_skymax(prods_d, ant_d, z)
    with pytest.raises(RuntimeError, match="contiguous"):
        ops.fe_null_skymax(prods_d, ant_d, z[..., ::2])
    with pytest.raises(RuntimeError, match=r"\(D, F, P, 2, R\)"):
        ops.fe_null_skymax(prods_d, ant_d, z[..., 0].contiguous())
    with pytest.raises(RuntimeError, match=r"\(D, F, P, 2, R\)"):
        ops.fe_null_skymax(prods_d, ant_d, z[:, :6].contiguous())
    with pytest.raises(RuntimeError, match="GPU"):
        ops.fe_null_skymax(prods_d, ant_d, z.cpu())
    with pytest.raises(RuntimeError, match="fp64"):
        ops.fe_null_skymax(prods_d, ant_d, z.float())
    with pytest.raises(RuntimeError, match="P matching"):
        ops.fe_null_skymax(prods_d, ant_d[:, :4].contiguous(), z)
    bad = prods.copy()
    bad[3, 1, 1, 2] = 0.5 * bad[3, 1, 2, 2] ** 2 / bad[3, 1, 0, 2]
    with pytest.raises(ValueError, match="pulsar 3, draw 1, frequency 2"):
        ops.fe_null_skymax(_dev(bad), ant_d, z)


# ----------------------------------------------------------------------
# GPU: end to end
# ----------------------------------------------------------------------
@pytest.mark.gpu
def test_fastfe_null_max_device():
    psrs, pta, Nvecs, Ts, sigmas, freqs, eng_cpu = _fixed_noise(False)
    sky = fibonacci_sky(20)
    fe = FastFe(psrs, pta)
    z = torch.as_tensor(_normals(5, 1, 7, 33, seed=9))
    want = fe.null_max(freqs, sky, Nvecs, Ts, sigmas, 33, engine=eng_cpu, z=z)
    eng = FpEngine(psrs, Nvecs, Ts, device=DEV)
    eng.precompute(freqs)
    got = fe.null_max(freqs, sky, Nvecs, Ts, sigmas, 33, engine=eng, z=z,
                      real_chunk=16)
    assert got.shape == (33, 7)
    print(f"null_max device vs cpu: {np.abs(got / want - 1).max():.3e}")
    np.testing.assert_allclose(got, want, rtol=RTOL)
    # the device stream: reproducible, and its own
    a = fe.null_max(freqs, sky, Nvecs, Ts, sigmas, 33, seed=2, engine=eng)
    b = fe.null_max(freqs, sky, Nvecs, Ts, sigmas, 33, seed=2, engine=eng)
    np.testing.assert_array_equal(a, b)
    femax, argmax, pfa = fe.false_alarm(freqs, sky, Nvecs, Ts, sigmas, 33,
                                        seed=2, engine=eng)
    wmax, warg = fe.sweep_max(freqs, sky, Nvecs, Ts, sigmas, engine=eng)
    np.testing.assert_array_equal(femax, wmax)
    np.testing.assert_array_equal(argmax, warg)
    np.testing.assert_array_equal(pfa, false_alarm_probability(femax, a))


@pytest.mark.gpu
def test_nmfe_null_max_device():
    psrs, pta, Nvecs, Ts, samples, phiinvs, freqs = _case(5)
    sky = fibonacci_sky(12)
    nm = NMFe(psrs, pta.rn_containers)
    a = nm.null_max(freqs, sky, samples, Nvecs, Ts, 10, seed=3, device=DEV,
                    draw_chunk=2, real_chunk=4)
    assert a.shape == (10, 5, 7) and np.isfinite(a).all() and (a > 0).all()
    b = nm.null_max(freqs, sky, samples, Nvecs, Ts, 10, seed=3, device=DEV,
                    draw_chunk=2, real_chunk=4)
    np.testing.assert_array_equal(a, b)
