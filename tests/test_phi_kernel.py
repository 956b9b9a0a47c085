"""``noise.batch_phiinv`` on the device: the one HIP kernel
(``ops.phi_inv_batch``) against the torch chain it replaces
(``noise._batch_phiinv_torch``) run on the same device.

The kernel repeats the chain's operations one rounding at a time, with
the device library's ``pow``, so the two are compared with
``torch.equal`` (docs/VALIDATION.md records that this holds)."""

import itertools
import types

import numpy as np
import pytest
import torch

from fastfp_amd import noise
from fastfp_amd.bases import create_freqarray
from fastfp_amd.noise import CURNContainer, RNContainer, batch_phiinv

DEV = "cuda:0"
TSPAN = 15.0 * 365.25 * 86400.0
# the benchmark's prior box and its corners
GAM, LGA = (1.0, 6.5), (-16.0, -13.5)
CORNERS = list(itertools.product(GAM, LGA))


def _containers(P, rn_comps, common, ntm, device):
    """P homogeneous red-noise containers; ``common``: None, "fewer" (the
    common process on fewer bins than the red noise) or "equal"."""
    curn = None
    if common is not None:
        nc = rn_comps if common == "equal" else max(1, rn_comps // 2)
        curn = CURNContainer(create_freqarray(TSPAN, nc), device=device)
    return [
        RNContainer(types.SimpleNamespace(name=f"J{i:04d}", Tspan=TSPAN,
                                          ntm=ntm),
                    ncomps=rn_comps, add_curn=curn is not None,
                    curn_container=curn, device=device)
        for i in range(P)
    ]


def _pars(conts, D, seed, device):
    """Parameters over the prior box, the first entries of every vector on
    its corners; ``D`` None: 0-d (scalar) parameters."""
    rng = np.random.default_rng(seed)
    names = [(c.rn_gam_name, c.rn_A_name) for c in conts]
    if conts[0].add_curn:
        cc = conts[0].curn_container
        names.append((cc.rn_gam_name, cc.rn_A_name))
    pars = {}
    for k, (gn, an) in enumerate(names):
        n = 1 if D is None else D
        g, a = rng.uniform(*GAM, n), rng.uniform(*LGA, n)
        for j in range(min(n, 4)):
            g[j], a[j] = CORNERS[(j + k) % 4]
        if D is None:
            g, a = g[0], a[0]
        pars[gn] = torch.as_tensor(g, dtype=torch.float64, device=device)
        pars[an] = torch.as_tensor(a, dtype=torch.float64, device=device)
    return pars


def _chain(conts, pars):
    """The torch chain's (P, D, m) on the containers' device."""
    dev = conts[0].Ffreqs.device
    gam = torch.stack([noise._as_tensor(pars[c.rn_gam_name], dev).reshape(-1)
                       for c in conts])
    lgA = torch.stack([noise._as_tensor(pars[c.rn_A_name], dev).reshape(-1)
                       for c in conts])
    return noise._batch_phiinv_torch(conts[0], gam, lgA, pars)


def _compare(got, want, label):
    rel = ((got - want).abs() / want.abs()).max().item()
    print(f"{label}: max |kernel - chain| / |chain| = {rel:.3e}, "
          f"equal = {torch.equal(got, want)}")
    assert torch.isfinite(got).all()
    assert torch.equal(got, want), f"{label}: max rel diff {rel:.3e}"


@pytest.mark.gpu
@pytest.mark.parametrize("ntm", [1, 2])
@pytest.mark.parametrize("common", [None, "fewer", "equal"])
@pytest.mark.parametrize("rn_comps", [2, 7, 30])
@pytest.mark.parametrize("D", [None, 1, 5, 67], ids=lambda d: f"D{d}")
@pytest.mark.parametrize("P", [1, 3])
def test_kernel_equals_torch_chain(P, D, rn_comps, common, ntm):
    conts = _containers(P, rn_comps, common, ntm, DEV)
    pars = _pars(conts, D, [P, D or 0, rn_comps, ntm], DEV)
    views = batch_phiinv(conts, pars, homogeneous=True)
    want = _chain(conts, pars)
    nd = 1 if D is None else D
    assert want.shape == (P, nd, ntm + 2 * rn_comps)
    assert len(views) == P and all(v.shape == want.shape[1:] for v in views)
    # the views of one (P, D, m) tensor, as the engine's factor reads them
    base = views[0].untyped_storage().data_ptr()
    assert all(v.untyped_storage().data_ptr() == base and v.is_contiguous()
               for v in views)
    _compare(torch.stack(views), want, f"P={P} D={D} comps={rn_comps} "
             f"common={common} ntm={ntm}")


@pytest.mark.gpu
def test_device_call_runs_the_kernel(monkeypatch):
    """On the device batch_phiinv goes through ops.phi_inv_batch and not
    through the torch chain."""
    from fastfp_amd import ops

    ops.require_hip()
    conts = _containers(3, 7, "fewer", 2, DEV)
    pars = _pars(conts, 5, 11, DEV)
    want = _chain(conts, pars)

    def no_chain(*a, **k):
        raise AssertionError("the torch chain ran on the device")

    monkeypatch.setattr(noise, "_batch_phiinv_torch", no_chain)
    _compare(torch.stack(batch_phiinv(conts, pars)), want, "kernel only")


@pytest.mark.gpu
def test_graph_replay_follows_new_inputs():
    """The call captures into a graph; a replay after the inputs changed
    in place gives the new inputs' phi^-1."""
    conts = _containers(3, 7, "fewer", 2, DEV)
    pars = _pars(conts, 5, 21, DEV)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        batch_phiinv(conts, pars, homogeneous=True)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        views = batch_phiinv(conts, pars, homogeneous=True)
    graph.replay()
    _compare(torch.stack(views), _chain(conts, pars), "replay, first inputs")
    first = torch.stack(views).clone()
    fresh = _pars(conts, 5, 22, DEV)
    for k, v in pars.items():
        v.copy_(fresh[k].flip(0))
    graph.replay()
    got = torch.stack(views)
    assert not torch.equal(got, first)
    _compare(got, _chain(conts, pars), "replay, new inputs")


@pytest.mark.parametrize("D", [None, 5], ids=lambda d: f"D{d}")
def test_cpu_path_is_the_torch_chain(D):
    """On the CPU batch_phiinv returns the torch chain's values, and
    those are the per-container phi^-1 within the bound of
    tests/test_property.py for the same phi by another op chain."""
    conts = _containers(3, 7, "fewer", 2, "cpu")
    pars = _pars(conts, D, 31, "cpu")
    views = batch_phiinv(conts, pars)
    want = _chain(conts, pars)
    assert torch.equal(torch.stack(views), want)
    for c, v in zip(conts, views):
        each = c.get_phiinv(pars)
        np.testing.assert_allclose(v.reshape(each.shape).numpy(),
                                   each.numpy(), rtol=1e-14, atol=0)
