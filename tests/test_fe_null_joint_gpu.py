"""Joint null across frequencies on the GPU (docs/DESIGN.md section 14):
the ``fe_null_data`` kernel, the ``data`` mode of ``ops.fe_null_skymax``
and ``null_max(joint=True)`` on a HIP engine against a CPU engine.

Tolerances.  ``fe_null_data`` is one length-``mp`` fp64 dot product per
entry on top of the white term, bounded elementwise by the forward error
bound ``4 mp eps (|white| + |B|^T |X|)`` (factor 4: FMA and ordering
slack).  Fe values are compared at rtol = 1e-9, the tolerance of
tests/test_fe_null.py for the ``z`` mode and for its CPU/GPU comparison.
"""

import numpy as np
import pytest
import torch

from fastfp_amd import (
    FastFe,
    FpEngine,
    NMFe,
    initialize_pta,
    make_synthetic_pta,
)
from fastfp_amd.cli.run_fe import fibonacci_sky
from fastfp_amd.festat import _null_draws, _null_max_host
from fastfp_amd.model import get_mats_fp, get_mats_nmfp

pytestmark = pytest.mark.gpu

RTOL = 1e-9
EPS = np.finfo(np.float64).eps
DEV = "cuda:0"


def _dev(x):
    return torch.as_tensor(x, dtype=torch.float64).to(DEV)


# ----------------------------------------------------------------------
# the kernel
# ----------------------------------------------------------------------
@pytest.mark.parametrize("P,D,F,m,mp,R", [(3, 2, 3, 20, 32, 17),
                                          (2, 1, 9, 130, 144, 33)])
def test_fe_null_data_kernel(P, D, F, m, mp, R):
    from fastfp_amd import ops

    rng = np.random.default_rng(100 + mp)
    Rp = ops.pad16(R)
    # what must not be read is NaN: the last column of rhs, the last
    # column and the padding rows of white
    white = np.full((P, Rp, 2 * F + 1), np.nan)
    white[:, :R, :2 * F] = rng.normal(size=(P, R, 2 * F))
    rhs = np.full((P, mp, 2 * F + 1), np.nan)
    rhs[:, :, :2 * F] = rng.normal(size=(P, mp, 2 * F))
    X = np.zeros((P, D, mp, R))
    X[:, :, :m] = rng.normal(size=(P, D, m, R))
    B = rhs[:, :, :2 * F]
    want = (white[:, :R, :2 * F].transpose(0, 2, 1)[:, None]
            - np.einsum("pkj,pdkr->pdjr", B, X))  # (P, D, 2F, R)
    want = want.reshape(P, D, F, 2, R).transpose(1, 2, 0, 3, 4)
    bound = 4.0 * mp * EPS * (
        np.abs(white[:, :R, :2 * F]).transpose(0, 2, 1)[:, None]
        + np.einsum("pkj,pdkr->pdjr", np.abs(B), np.abs(X)))
    bound = bound.reshape(P, D, F, 2, R).transpose(1, 2, 0, 3, 4)

    args = (_dev(white), _dev(rhs), _dev(X))
    numel, guard = D * F * P * 2 * R, 4096
    buf = torch.full((numel + 2 * guard,), float("nan"), dtype=torch.float64,
                     device=DEV)
    out = buf[guard:guard + numel].view(D, F, P, 2, R)
    got = ops.fe_null_data(*args, out=out)
    assert got.data_ptr() == out.data_ptr()
    assert torch.isnan(buf[:guard]).all() and torch.isnan(buf[-guard:]).all()
    got_h = got.cpu().numpy()
    assert np.isfinite(got_h).all()
    ratio = (np.abs(got_h - want) / bound).max()
    print(f"mp={mp}: largest |err| / bound {ratio:.3e}")
    assert (np.abs(got_h - want) <= bound).all()
    again = ops.fe_null_data(*args)
    assert again.shape == (D, F, P, 2, R) and again.is_contiguous()
    assert torch.equal(again, got)
    # the torch arm computes the same array
    alt = ops.fe_null_data_torch(*args).cpu().numpy()
    assert (np.abs(alt - want) <= bound).all()


def test_fe_null_data_rejects_bad_inputs():
    from fastfp_amd import ops

    white, rhs = torch.zeros((2, 16, 7)), torch.zeros((2, 16, 7))
    X = torch.zeros((2, 1, 16, 5))
    args = [_dev(white), _dev(rhs), _dev(X)]
    ops.fe_null_data(*args)
    with pytest.raises(RuntimeError, match="multiple of 16"):
        ops.fe_null_data(args[0], _dev(torch.zeros((2, 20, 7))),
                         _dev(torch.zeros((2, 1, 20, 5))))
    with pytest.raises(RuntimeError, match="multiple of 16"):
        ops.fe_null_data(args[0], _dev(torch.zeros((2, 272, 7))),
                         _dev(torch.zeros((2, 1, 272, 5))))
    with pytest.raises(RuntimeError, match="2F\\+1"):
        ops.fe_null_data(args[0], _dev(torch.zeros((2, 16, 6))), args[2])
    with pytest.raises(RuntimeError, match="white must be"):
        ops.fe_null_data(_dev(torch.zeros((2, 4, 7))), args[1], args[2])
    with pytest.raises(RuntimeError, match="X must be"):
        ops.fe_null_data(args[0], args[1], _dev(torch.zeros((3, 1, 16, 5))))
    with pytest.raises(RuntimeError, match="out must be"):
        ops.fe_null_data(*args, out=_dev(torch.zeros((1, 3, 2, 2, 4))))
    with pytest.raises(RuntimeError, match="fp64"):
        ops.fe_null_data(args[0].float(), args[1], args[2])


# ----------------------------------------------------------------------
# the data mode of the sky kernel
# ----------------------------------------------------------------------
def _synthetic_products(P, D=2, F=5, nsky=20, seed=3):
    """The recipe of tests/test_fe_null.py."""
    rng = np.random.default_rng(seed)
    prods = np.empty((P, D, 5, F))
    prods[:, :, 0:2] = rng.uniform(1.0, 2.0, (P, D, 2, F))
    prods[:, :, 2] = 0.1 * rng.normal(size=(P, D, F))
    prods[:, :, 3:] = rng.normal(size=(P, D, 2, F))
    return prods, rng.normal(size=(nsky, P, 2))


def _assert_matches(got_max, got_arg, want, warg, prods, ant, n):
    """femax at rtol; argmax equal or a near-tie on the host."""
    got_max, got_arg = got_max.cpu().numpy(), got_arg.cpu().numpy()
    diff = np.argwhere(got_arg != warg)
    print(f"max rel err {np.abs(got_max / want - 1).max():.3e}, "
          f"{len(diff)} argmax differences")
    np.testing.assert_allclose(got_max, want, rtol=RTOL)
    for r, d, f in diff:
        k = int(got_arg[r, d, f])
        at, _ = _null_max_host(prods[:, d:d + 1, :, f:f + 1], ant[k:k + 1],
                               n=n[d:d + 1, f:f + 1, :, :, r:r + 1])
        assert abs(at[0, 0, 0] / want[r, d, f] - 1) <= RTOL


def test_fe_null_skymax_data_mode():
    from fastfp_amd import ops

    P, R = 9, 33
    prods, ant = _synthetic_products(P)
    rng = np.random.default_rng(8)
    n = 3.0 * rng.standard_normal((2, 5, P, 2, R))
    want, warg = _null_max_host(prods, ant, n=n)
    femax, argmax, nskip = ops.fe_null_skymax(_dev(prods), _dev(ant), _dev(n),
                                              data=True)
    assert femax.shape == (R, 2, 5) and (nskip == 0).all()
    _assert_matches(femax, argmax, want, warg, prods, ant, n)
    # one degenerate sky row: every column goes through the host repair
    deg = ant.copy()
    deg[4, :, 1] = 2.0 * deg[4, :, 0]
    want, warg = _null_max_host(prods, deg, n=n)
    femax, argmax, nskip = ops.fe_null_skymax(_dev(prods), _dev(deg), _dev(n),
                                              data=True)
    assert (nskip == 1).all()
    _assert_matches(femax, argmax, want, warg, prods, deg, n)
    # n = L z formed on the host: the z mode's own numbers
    z = rng.standard_normal((2, 5, P, 2, R))
    ns, nc = _null_draws(prods, z)  # (P, D, F, R)
    nz = np.ascontiguousarray(
        np.stack([ns, nc], axis=3).transpose(1, 2, 0, 3, 4))
    a = ops.fe_null_skymax(_dev(prods), _dev(ant), _dev(z))
    b = ops.fe_null_skymax(_dev(prods), _dev(ant), _dev(nz), data=True)
    assert torch.equal(a[1], b[1]) and torch.equal(a[2], b[2])
    np.testing.assert_allclose(b[0].cpu().numpy(), a[0].cpu().numpy(),
                               rtol=RTOL)
    # the data mode does not ask for positive-definite blocks
    bad = prods.copy()
    bad[3, 1, 0, 2] = -1.0
    with pytest.raises(ValueError, match="pulsar 3, draw 1, frequency 2"):
        ops.fe_null_skymax(_dev(bad), _dev(ant), _dev(z))
    c = ops.fe_null_skymax(_dev(bad), _dev(ant), _dev(nz), data=True)
    assert c[0].shape == (R, 2, 5)


# ----------------------------------------------------------------------
# end to end: HIP engine against CPU engine on the same normals
# ----------------------------------------------------------------------
def _pta(npsr=3):
    psrs = make_synthetic_pta(npsr=npsr, ntoa=80, ntm=3, seed=21)
    noise = {"gw_gamma": 13.0 / 3.0, "gw_log10_A": float(np.log10(2e-15))}
    for p in psrs:
        noise[f"{p.name}_red_noise_gamma"] = 4.0
        noise[f"{p.name}_red_noise_log10_A"] = -14.5
    pta = initialize_pta(psrs, noise, inc_cp=True, rn_comps=3, gwb_comps=3)
    return psrs, noise, pta


def _normals(psrs, Ts, nreal, seed=13):
    g = torch.Generator().manual_seed(seed)
    w = [torch.randn((len(p.toas), nreal), generator=g, dtype=torch.float64)
         for p in psrs]
    u = [torch.randn((np.asarray(T).shape[1], nreal), generator=g,
                     dtype=torch.float64) for T in Ts]
    return w, u


def _engines(psrs, Nvecs, Ts, freqs):
    out = []
    for dev in ("cpu", DEV):
        eng = FpEngine(psrs, Nvecs, Ts, device=dev)
        eng.precompute(freqs)
        out.append(eng)
    assert out[1]._null_kernel_path() and not out[0]._null_kernel_path()
    return out


def test_fastfe_joint_null_max_device():
    psrs, noise, pta = _pta()
    Nvecs, Ts, sigmas = get_mats_fp(pta, noise)
    freqs = np.linspace(5e-9, 4e-8, 4)
    sky = fibonacci_sky(12)
    cpu, hip = _engines(psrs, Nvecs, Ts, freqs)
    w, u = _normals(psrs, Ts, 20)
    fe = FastFe(psrs, pta)
    args = (freqs, sky, Nvecs, Ts, sigmas, 20)
    want = fe.null_max(*args, engine=cpu, joint=True, w=w, u=u)
    got = fe.null_max(*args, engine=hip, joint=True, w=w, u=u, real_chunk=16)
    assert got.shape == (20, 4)
    print(f"joint null_max device vs cpu: {np.abs(got / want - 1).max():.3e}")
    np.testing.assert_allclose(got, want, rtol=RTOL)
    # the device stream: reproducible
    a = fe.null_max(*args, seed=2, engine=hip, joint=True)
    np.testing.assert_array_equal(
        a, fe.null_max(*args, seed=2, engine=hip, joint=True))
    out = fe.false_alarm(*args, seed=2, engine=hip, joint=True)
    assert len(out) == 6 and 0 < out[5] <= 1 and out[3] == out[0].max()


def test_nmfe_joint_null_max_device():
    psrs, noise, pta = _pta()
    _, Nvecs, Ts = get_mats_nmfp(pta, noise)
    rng = np.random.default_rng(17)
    samples = {k: (rng.uniform(2, 6, 3) if k.endswith("gamma")
                   else rng.uniform(-16, -14, 3)) for k in pta.params}
    freqs = np.linspace(5e-9, 4e-8, 4)
    sky = fibonacci_sky(12)
    cpu, hip = _engines(psrs, Nvecs, Ts, freqs)
    w, u = _normals(psrs, Ts, 10)
    nm = NMFe(psrs, pta.rn_containers)
    args = (freqs, sky, samples, Nvecs, Ts, 10)
    want = nm.null_max(*args, engine=cpu, joint=True, w=w, u=u)
    got = nm.null_max(*args, engine=hip, joint=True, w=w, u=u, draw_chunk=2,
                      real_chunk=4)
    assert got.shape == (10, 3, 4)
    print(f"NMFe joint device vs cpu: {np.abs(got / want - 1).max():.3e}")
    np.testing.assert_allclose(got, want, rtol=RTOL)
