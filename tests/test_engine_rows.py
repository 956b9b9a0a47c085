"""``FpEngine.sweep`` fed with ``batch_phiinv``'s views of one (P, D, m)
device tensor — the factor then reads the prior rows in place
(``chol_rows_into``) — against the same sweep fed with cloned rows, which
takes the gathered copy and ``SolveSystem.diag``.  Three pulsars,
m_v = 60 (mp = 64, lead = 4), D = 20 draws, F = 70 frequencies; the
results must be ``torch.equal``."""

import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
D, F = 20, 70


class _Counting:
    """The engine's extension with its factor entries counted."""

    def __init__(self, real):
        self._real = real
        self.calls = {"chol_rows_into": 0, "chol_batch_into": 0,
                      "chol_batch": 0}

    def __getattr__(self, name):
        fn = getattr(self._real, name)
        if name not in self.calls:
            return fn

        def counted(*a, **k):
            self.calls[name] += 1
            return fn(*a, **k)
        return counted


@functools.lru_cache(maxsize=None)
def _setup():
    """(engine, batch_phiinv's views); built once, shared, read-only."""
    from fastfp_amd import FpEngine, get_mats_nmfp, initialize_pta, \
        make_synthetic_pta
    from fastfp_amd.noise import batch_phiinv

    psrs = make_synthetic_pta(npsr=3, ntoa=300, ntm=10, seed=7)
    noise = {"gw_gamma": 13.0 / 3.0, "gw_log10_A": float(np.log10(2e-15))}
    for p in psrs:
        noise[f"{p.name}_red_noise_gamma"] = 4.0
        noise[f"{p.name}_red_noise_log10_A"] = -14.5
    pta = initialize_pta(psrs, noise, inc_cp=True, rn_comps=30, gwb_comps=30)
    _, Nvecs, Ts = get_mats_nmfp(pta, noise)
    eng = FpEngine(psrs, Nvecs, Ts, device=DEV)
    eng.precompute(np.linspace(5e-9, 4e-8, F))
    eng.enable_draw_compression(
        [c.var_slice for c in pta.rn_containers],
        [c.get_phiinv(noise) for c in pta.rn_containers])
    st = eng._comp_stack
    assert st is not None and st.A.shape[-1] == 64 and st.lead == 4
    assert eng._direct_stack is not None
    for c in pta.rn_containers:
        c.to(DEV)
    rng = np.random.default_rng(107)
    samples = {
        n: torch.as_tensor(rng.uniform(2, 6, D) if n.endswith("gamma")
                           else rng.uniform(-16, -14, D), device=DEV)
        for n in pta.params
    }
    views = batch_phiinv(pta.rn_containers, samples)
    assert float(eng.compression_margin_per_draw(views).min()) >= 1.5
    return eng, views


@pytest.mark.parametrize("force_direct", [False, True],
                         ids=["compressed", "direct"])
@pytest.mark.parametrize("chunk", [16, 4])
def test_sweep_on_views_equals_sweep_on_clones(chunk, force_direct):
    """Chunks of 16: two chunks through the factor/solve pipeline, the
    first on the draw-looping solve.  Chunks of 4: five chunks on the
    one-draw solve."""
    eng, views = _setup()
    clones = [v.clone() for v in views]
    st = eng._direct_stack if force_direct else eng._comp_stack
    assert eng._rows_in_place(st, views) is not None
    assert eng._rows_in_place(st, clones) is None
    nchunk = -(-D // chunk)
    real = eng._ext
    try:
        eng._ext = ext = _Counting(real)
        new = eng.sweep(phiinvs=views, draw_chunk=chunk,
                        force_direct=force_direct)
        assert ext.calls == {"chol_rows_into": nchunk, "chol_batch_into": 0,
                             "chol_batch": 0}, ext.calls
        eng._ext = ext = _Counting(real)
        old = eng.sweep(phiinvs=clones, draw_chunk=chunk,
                        force_direct=force_direct)
        assert ext.calls == {"chol_rows_into": 0, "chol_batch_into": nchunk,
                             "chol_batch": 0}, ext.calls
    finally:
        eng._ext = real
    assert new.shape == (D, F) and torch.isfinite(new).all()
    assert torch.equal(new, old)


def test_single_chunk_allocates_its_factor():
    """One chunk (no pipeline): the in-place rows factor into tensors of
    their own, with the same result."""
    eng, views = _setup()
    clones = [v.clone() for v in views]
    real = eng._ext
    try:
        eng._ext = ext = _Counting(real)
        new = eng.sweep(phiinvs=views, draw_chunk=32)
        assert ext.calls["chol_rows_into"] == 1, ext.calls
    finally:
        eng._ext = real
    assert torch.equal(new, eng.sweep(phiinvs=clones, draw_chunk=32))
