"""Fe products on the Schur-compressed system: the ``compressed`` keyword
of ``FpEngine.sweep_products`` / ``sweep_products_hip``, ``compress`` of
``NMFe.sweep`` / ``NMFe.sweep_max`` and ``--compress`` of ``run_nmfe``.

Two arrays, both from the ``_pta`` / ``_samples`` recipes of
tests/test_fe_device.py with ``freqs = linspace(5e-9, 4e-8, F)``:

  A: 5 or 9 pulsars, 80 TOAs, m = 9, m_v = 6 -> mp = 16, lead = 10
     (SKIP = 2), PTA seeds 31 / 32, F = 7, D = 5;
  B: 3 pulsars, 300 TOAs, m = 70, m_v = 60 -> mp = 64, lead = 4
     (SKIP = 1), PTA seed 7, F = 70 (tiles of 63 + 7), D = 20.

Measured on the CPU: every pulsar keeps compression (probe errors at
most 1.3e-13 on A, 2.9e-9 on B), the per-draw margin is at least 2000,
compressed-vs-direct products differ by at most 5.2e-13 (A) and 1.8e-8
(B) of a plane's largest magnitude, and the 48-point Fe map by at most
2.1e-13 relative (A) and 3.3e-9 of its maximum (B).

Tolerances: 1e-6 of a plane's or map's maximum where the compressed
system of array B is involved — the bound the project uses for the
compressed path (the probe tolerance of ``_probe_compression``, the
GPU-vs-CPU bound of test_engine_stacked_sweep_uses_draw_loop) — and
``RTOL = 1e-9``, the project's GPU-vs-CPU Fe tolerance, on array A."""

import functools
import json
import sys
import types

import numpy as np
import pytest
import torch

from fastfp_amd import FpEngine, initialize_pta, make_synthetic_pta
from fastfp_amd.cli.run_fe import fibonacci_sky
from fastfp_amd.festat import NMFe
from fastfp_amd.model import get_mats_nmfp
from fastfp_amd.noise import batch_phiinv

RTOL = 1e-9
CTOL = 1e-6
DEV = "cuda:0"
# name -> (npsr, ntoa, ntm, comps, PTA seed, F, D)
ARRAYS = {
    "A5": (5, 80, 3, 3, 31, 7, 5),
    "A9": (9, 80, 3, 3, 32, 7, 5),
    "B": (3, 300, 10, 30, 7, 70, 20),
}


def _pta(npsr, ntoa, ntm, comps, seed):
    psrs = make_synthetic_pta(npsr=npsr, ntoa=ntoa, ntm=ntm, seed=seed)
    noise = {"gw_gamma": 13.0 / 3.0, "gw_log10_A": float(np.log10(2e-15))}
    for p in psrs:
        noise[f"{p.name}_red_noise_gamma"] = 4.0
        noise[f"{p.name}_red_noise_log10_A"] = -14.5
    pta = initialize_pta(psrs, noise, inc_cp=True, rn_comps=comps,
                         gwb_comps=comps)
    return psrs, noise, pta


def _samples(pta, D, seed):
    rng = np.random.default_rng(seed)
    return {
        n: (rng.uniform(2, 6, D) if n.endswith("gamma")
            else rng.uniform(-16, -14, D))
        for n in pta.params
    }


def _phiinvs(pta, samples):
    phiinvs = batch_phiinv(pta.rn_containers, samples)
    return [p[None, :] if p.dim() == 1 else p for p in phiinvs]


class _Array(types.SimpleNamespace):
    def engine(self, device, compress=True):
        eng = FpEngine(self.psrs, self.Nvecs, self.Ts, device=device)
        eng.precompute(self.freqs)
        if compress:
            eng.enable_draw_compression(
                [c.var_slice for c in self.pta.rn_containers],
                [c.get_phiinv(self.noise) for c in self.pta.rn_containers])
        return eng


@functools.lru_cache(maxsize=None)
def _array(name):
    """One reference array; built once and shared (read-only)."""
    npsr, ntoa, ntm, comps, seed, F, D = ARRAYS[name]
    psrs, noise, pta = _pta(npsr, ntoa, ntm, comps, seed)
    _, Nvecs, Ts = get_mats_nmfp(pta, noise)
    samples = _samples(pta, D, seed + 100)
    return _Array(psrs=psrs, noise=noise, pta=pta, Nvecs=Nvecs, Ts=Ts,
                  samples=samples, phiinvs=_phiinvs(pta, samples),
                  freqs=np.linspace(5e-9, 4e-8, F), npsr=npsr, F=F, D=D,
                  mv=2 * comps)


@functools.lru_cache(maxsize=None)
def _cpu(name):
    """(CPU engine with compression, its direct and its compressed
    products as numpy (P, D, 5, F)); computed once, never modified."""
    a = _array(name)
    eng = a.engine("cpu")
    assert all(b.comp is not None for b in eng.blocks), \
        [getattr(b, "probe_err", None) for b in eng.blocks]
    assert float(eng.compression_margin_per_draw(a.phiinvs).min()) >= 2000
    direct = eng.sweep_products(phiinvs=a.phiinvs).numpy()
    comp = eng.sweep_products(phiinvs=a.phiinvs, compressed=True).numpy()
    return eng, direct, comp


def _plane_err(got, want):
    """max over (pulsar, product) planes of max|got - want| / max|want|,
    a plane being the (D, F) values of one product of one pulsar."""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, (got.shape, want.shape)
    assert np.isfinite(got).all()
    num = np.abs(got - want).max(axis=(1, 3))
    return float((num / np.abs(want).max(axis=(1, 3))).max())


def _map_err(got, want):
    assert got.shape == want.shape and np.isfinite(got).all()
    return float(np.abs(got - want).max() / np.abs(want).max())


def _hybrid_samples(a, D=8):
    """D draws of the recipe with every log10_A overwritten by -10.0 at
    draws 2 and 5: their phi^-1 falls below the reference prior."""
    samples = _samples(a.pta, D, 1000)
    for n, v in samples.items():
        if n.endswith("log10_A"):
            v[[2, 5]] = -10.0
    return samples


def _assert_hybrid_precondition(eng, a, samples):
    margins = eng.compression_margin_per_draw(_phiinvs(a.pta, samples))
    bad = torch.nonzero(margins < 1.5).reshape(-1).tolist()
    assert bad == [2, 5], margins


# ----------------------------------------------------------------------
# CPU
# ----------------------------------------------------------------------
@pytest.mark.parametrize("name,tol", [("A5", RTOL), ("A9", RTOL),
                                      ("B", CTOL)])
def test_sweep_products_compressed_cpu(name, tol):
    a = _array(name)
    eng, direct, comp = _cpu(name)
    assert comp.shape == (a.npsr, a.D, 5, a.F)
    err = _plane_err(comp, direct)
    print(f"array {name}: compressed vs direct products, of plane max: {err}")
    assert err <= tol
    # the fixed-noise form is draw 0 of the batch
    one = eng.sweep_products(phiinvs=[p[0] for p in a.phiinvs],
                             compressed=True).numpy()
    assert one.shape == (a.npsr, 5, a.F)
    np.testing.assert_allclose(one, comp[:, 0], rtol=1e-12)


def test_sweep_products_compressed_rejects_sigmas():
    a = _array("A5")
    eng = _cpu("A5")[0]
    sigmas = [b.TNT + torch.diag(p[0]) for b, p in zip(eng.blocks, a.phiinvs)]
    with pytest.raises(ValueError):
        eng.sweep_products(sigmas=sigmas, compressed=True)
    with pytest.raises(ValueError):
        eng.sweep_products(sigmas, a.phiinvs, compressed=True)


def test_sweep_products_compressed_without_compression_is_direct():
    a = _array("A5")
    eng = a.engine("cpu")
    eng.disable_draw_compression()
    np.testing.assert_array_equal(
        eng.sweep_products(phiinvs=a.phiinvs, compressed=True).numpy(),
        eng.sweep_products(phiinvs=a.phiinvs).numpy())
    np.testing.assert_array_equal(
        eng.sweep_products_hip(a.phiinvs, compressed=True).numpy(),
        eng.sweep_products(phiinvs=a.phiinvs).numpy())


def test_nmfe_compress_cpu():
    a = _array("A5")
    sky = fibonacci_sky(48)
    nm = NMFe(a.psrs, a.pta.rn_containers)
    args = (a.freqs, sky, a.samples, a.Nvecs, a.Ts)
    want = nm.sweep(*args, device="cpu")
    got = nm.sweep(*args, device="cpu", compress=True)
    assert got.shape == (a.D, 48, a.F)
    print("NMFe.sweep compress vs direct, relative:",
          np.abs(got / want - 1).max())
    np.testing.assert_allclose(got, want, rtol=RTOL)
    np.testing.assert_array_equal(np.argmax(got, axis=1),
                                  np.argmax(want, axis=1))
    fm0, am0 = nm.sweep_max(*args, device="cpu")
    fm, am = nm.sweep_max(*args, device="cpu", compress=True, draw_chunk=2)
    np.testing.assert_allclose(fm, fm0, rtol=RTOL)
    np.testing.assert_array_equal(am, am0)
    np.testing.assert_array_equal(am, np.argmax(want, axis=1))


def test_nmfe_compress_hybrid_guard_cpu():
    a = _array("A5")
    samples = _hybrid_samples(a)
    eng = _cpu("A5")[0]
    _assert_hybrid_precondition(eng, a, samples)
    sky = fibonacci_sky(48)
    nm = NMFe(a.psrs, a.pta.rn_containers)
    args = (a.freqs, sky, samples, a.Nvecs, a.Ts)
    want = nm.sweep(*args, engine=eng)
    got = nm.sweep(*args, engine=eng, compress=True)
    assert np.isfinite(got).all()
    np.testing.assert_allclose(got[[2, 5]], want[[2, 5]], rtol=1e-12)
    rest = [0, 1, 3, 4, 6, 7]
    np.testing.assert_allclose(got[rest], want[rest], rtol=RTOL)
    # an engine built inside the call compresses around draw 0
    got2 = nm.sweep(*args, device="cpu", compress=True)
    assert np.isfinite(got2).all()
    np.testing.assert_allclose(got2[[2, 5]], want[[2, 5]], rtol=1e-12)
    np.testing.assert_allclose(got2[rest], want[rest], rtol=RTOL)


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


def test_run_nmfe_compress_cpu(tmp_path, monkeypatch):
    from fastfp_amd.cli import run_nmfe

    psrfile, noisefile, chainfile = _cli_inputs(tmp_path)
    kw = dict(inc_cp=True, nrncomps=3, ngwbcomps=3, ncwfreqs=4, nsamples=5,
              nsky=6, outdir=str(tmp_path), device="cpu", batch_size=2)
    run_nmfe.main(psrfile, noisefile, chainfile, "cube", **kw)
    run_nmfe.main(psrfile, noisefile, chainfile, "cubec", compress=True, **kw)
    want, got = np.load(tmp_path / "cube.npy"), np.load(tmp_path / "cubec.npy")
    assert got.shape == want.shape == (5, 6, 4)
    np.testing.assert_allclose(got, want, rtol=RTOL)
    run_nmfe.main(psrfile, noisefile, chainfile, "mx", skymax=True, **kw)
    run_nmfe.main(psrfile, noisefile, chainfile, "mxc", skymax=True,
                  compress=True, **kw)
    np.testing.assert_allclose(np.load(tmp_path / "mxc.max.npy"),
                               np.load(tmp_path / "mx.max.npy"), rtol=RTOL)
    np.testing.assert_array_equal(np.load(tmp_path / "mxc.argmax.npy"),
                                  np.load(tmp_path / "mx.argmax.npy"))

    # the parser accepts --compress and hands it to main
    seen = {}
    monkeypatch.setattr(run_nmfe, "main", lambda **k: seen.update(k))
    monkeypatch.setattr(sys, "argv", ["run_nmfe", "p", "n", "c", "s",
                                      "--compress"])
    run_nmfe.cli()
    assert seen["compress"] is True
    monkeypatch.setattr(sys, "argv", ["run_nmfe", "p", "n", "c", "s"])
    run_nmfe.cli()
    assert seen["compress"] is False


# ----------------------------------------------------------------------
# GPU
# ----------------------------------------------------------------------
def _counting(eng):
    """Wrap the engine's extension so the solve calls are counted."""
    calls = {"store": 0, "prods": 0}
    real = eng._ext

    def counted(name, fn):
        def f(*a, **k):
            calls[name] += 1
            return fn(*a, **k)
        return f

    eng._ext = types.SimpleNamespace(
        chol_batch=real.chol_batch,
        trsm_prods_store=counted("store", real.trsm_prods_store),
        trsm_prods=counted("prods", real.trsm_prods))
    return calls


@pytest.mark.gpu
def test_stacked_compressed_products_gpu():
    """Array B (mp = 64, lead = 4): every chunk of 32 goes through
    trsm_prods_store; chunks of 16 and 4 take one trsm_prods_store and
    one trsm_prods call and change no bit."""
    a = _array("B")
    _, direct, want = _cpu("B")
    eng = a.engine(DEV)
    st = eng._comp_stack
    assert st is not None and st.A.shape[-1] == 64 and st.lead == 4
    calls = _counting(eng)
    got = eng.sweep_products_hip(a.phiinvs, draw_chunk=32, compressed=True)
    assert calls == {"store": 1, "prods": 0}, calls
    assert got.is_cuda and got.shape == (3, 20, 5, 70)
    err = _plane_err(got.cpu().numpy(), want)
    print("array B: GPU compressed vs CPU compressed, of plane max:", err)
    print("array B: GPU compressed vs CPU direct, of plane max:",
          _plane_err(got.cpu().numpy(), direct))
    assert err <= CTOL
    two = eng.sweep_products_hip(a.phiinvs, draw_chunk=16, compressed=True)
    assert calls == {"store": 2, "prods": 1}, calls
    assert torch.equal(two, got)
    again = eng.sweep_products_hip(a.phiinvs, draw_chunk=16, compressed=True)
    assert torch.equal(again, two)
    one = eng.sweep_products_hip([p[1] for p in a.phiinvs], compressed=True)
    assert one.shape == (3, 5, 70)
    assert torch.equal(one, got[:, 1])


@pytest.mark.gpu
def test_stacked_compressed_products_skip2_gpu():
    """Array A, 9 pulsars (mp = 16, lead = 10 -> SKIP = 2) with the draw
    loop eligible from one draw."""
    a = _array("A9")
    _, direct, _ = _cpu("A9")
    eng = a.engine(DEV)
    st = eng._comp_stack
    assert st is not None and st.A.shape[-1] == 16 and st.lead == 10
    eng.DRAW_LOOP_MIN_DRAWS = 1
    calls = _counting(eng)
    got = eng.sweep_products_hip(a.phiinvs, compressed=True)
    assert calls == {"store": 1, "prods": 0}, calls
    err = _plane_err(got.cpu().numpy(), direct)
    print("array A9: GPU compressed vs CPU direct, of plane max:", err)
    assert err <= RTOL


@pytest.mark.gpu
def test_ragged_compressed_products_gpu():
    """Array B with compression dropped on pulsar 1: no stack forms, the
    products come per pulsar and pulsar 1's are the direct ones."""
    a = _array("B")
    cpu = a.engine("cpu")
    cpu.blocks[1].comp = None
    want = cpu.sweep_products(phiinvs=a.phiinvs, compressed=True).numpy()
    eng = a.engine(DEV)
    eng.blocks[1].comp = None
    eng._stack_compression()
    assert eng._comp_stack is None
    got = eng.sweep_products_hip(a.phiinvs, compressed=True)
    assert got.is_cuda and got.shape == (3, 20, 5, 70)
    err = _plane_err(got.cpu().numpy(), want)
    print("array B ragged: GPU vs CPU, of plane max:", err)
    assert err <= CTOL
    plain = eng.sweep_products_hip(a.phiinvs)
    assert torch.equal(got[1], plain[1])
    assert not torch.equal(got[0], plain[0])


@pytest.mark.gpu
def test_ragged_compressed_products_chunked_gpu():
    """The per-pulsar products across a chunk boundary: array B with
    compression dropped on pulsar 1, draws in chunks of 16 and 4.  The
    two compressed pulsars (mp = 64) take trsm_prods_store on the 16 and
    trsm_prods on the 4, the direct pulsar (mp = 80) trsm_prods on both,
    and no bit differs from the single chunk."""
    a = _array("B")
    eng = a.engine(DEV)
    eng.blocks[1].comp = None
    eng._stack_compression()
    assert eng._comp_stack is None
    assert [b.comp is not None for b in eng.blocks] == [True, False, True]
    want = eng.sweep_products_hip(a.phiinvs, draw_chunk=32, compressed=True)
    calls = _counting(eng)
    got = eng.sweep_products_hip(a.phiinvs, draw_chunk=16, compressed=True)
    assert calls == {"store": 2, "prods": 4}, calls
    assert got.shape == (3, 20, 5, 70)
    assert torch.equal(got, want)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["A5", "A9"])
def test_nmfe_compress_device_matches_cpu(name):
    a = _array(name)
    sky = fibonacci_sky(48)
    nm = NMFe(a.psrs, a.pta.rn_containers)
    args = (a.freqs, sky, a.samples, a.Nvecs, a.Ts)
    want = nm.sweep(*args, device="cpu")
    got = nm.sweep(*args, device=DEV, assemble="device", compress=True)
    print(f"array {name}: device compressed Fe vs CPU direct, relative:",
          np.abs(got / want - 1).max())
    np.testing.assert_allclose(got, want, rtol=RTOL)
    np.testing.assert_array_equal(np.argmax(got, axis=1),
                                  np.argmax(want, axis=1))
    fm, am = nm.sweep_max(*args, device=DEV, compress=True)
    np.testing.assert_allclose(fm, want.max(axis=1), rtol=RTOL)
    np.testing.assert_array_equal(am, np.argmax(want, axis=1))


@pytest.mark.gpu
def test_nmfe_compress_hybrid_guard_device():
    a = _array("A5")
    samples = _hybrid_samples(a)
    eng = a.engine(DEV)
    _assert_hybrid_precondition(eng, a, samples)
    sky = fibonacci_sky(48)
    nm = NMFe(a.psrs, a.pta.rn_containers)
    args = (a.freqs, sky, samples, a.Nvecs, a.Ts)
    plain = nm.sweep(*args, engine=eng, assemble="device")
    got = nm.sweep(*args, engine=eng, assemble="device", compress=True)
    assert np.isfinite(got).all()
    np.testing.assert_array_equal(got[[2, 5]], plain[[2, 5]])
    rest = [0, 1, 3, 4, 6, 7]
    np.testing.assert_allclose(got[rest], plain[rest], rtol=RTOL)
    fm0, am0 = nm.sweep_max(*args, engine=eng)
    fm, am = nm.sweep_max(*args, engine=eng, compress=True)
    np.testing.assert_array_equal(fm[[2, 5]], fm0[[2, 5]])
    np.testing.assert_array_equal(am[[2, 5]], am0[[2, 5]])
    np.testing.assert_allclose(fm, fm0, rtol=RTOL)


@pytest.mark.gpu
def test_products_hip_defaults_ignore_compression():
    a = _array("B")
    with_comp = a.engine(DEV)
    assert with_comp._comp_stack is not None
    without = a.engine(DEV, compress=False)
    assert torch.equal(with_comp.sweep_products_hip(a.phiinvs),
                       without.sweep_products_hip(a.phiinvs))
    assert torch.equal(without.sweep_products_hip(a.phiinvs, compressed=True),
                       without.sweep_products_hip(a.phiinvs))
