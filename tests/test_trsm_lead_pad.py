"""The leading pad of the stacked compressed solve.

``trsm_fp_store(..., lead=k)`` (trsm_fp_draws_kernel<NBT, SKIP = k/4>)
leaves out the MFMAs whose operand is the zero top of W when the system
starts with a k x k identity block over k zero RHS rows.  The kernel
tests embed a real system of size mp - lead under such a block, factor
it on the device at m = mp and check that the skip changes no bit and
that the result is the unpadded system's, against the longdouble oracle
under the 16x rule of tests/hpref.py (base: numpy's fp64 factor and
scipy's fp64 substitution of the unpadded system).  The engine tests
check that the compressed stack presents such a system and hands its
``lead`` to every solve."""

import types

import numpy as np
import pytest
import torch

import hpref

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
P, D, DPB = 2, 5, 2  # slices of 2, 2 and 1 draws: both LDS buffers, a tail


def _ext():
    from fastfp_amd import ops

    ops.require_hip()
    from fastfp_amd.ops import _fastfp_hip

    return _fastfp_hip


def _t(a):
    return torch.tensor(np.asarray(a, dtype=np.float64), device=DEV)


_CASES = {}


def _case(nbt, lead):
    """Inputs of one padded system and the references of the unpadded
    one; built once per (nbt, lead), shared, never modified."""
    key = (nbt, lead)
    if key in _CASES:
        return _CASES[key]
    F = int(_ext().trsm_fp_store_tile_freqs()) + 1
    mp = 16 * nbt
    mv = mp - lead
    rng = np.random.default_rng([7, nbt, lead])
    A = np.zeros((P, mp, mp))
    diag = np.zeros((P, D, mp))
    RHS = np.zeros((P, mp, 2 * F + 1))
    S, R = np.empty((P, 3, F)), np.empty((P, 2, F))
    W = np.empty((P, D, mv, 2 * F + 1), dtype=hpref.LD)
    W64 = np.empty((P, D, mv, 2 * F + 1))
    for p in range(P):
        TNT, phiinv = hpref.gen_sigma(rng, mv, D)
        A[p, :lead, :lead] = np.eye(lead)
        A[p, lead:, lead:] = TNT
        diag[p, :, lead:] = phiinv
        B = hpref.gen_rhs(rng, mv, mv, F)
        RHS[p, lead:] = B
        for d in range(D):
            Sig = hpref.sigma_of(TNT, phiinv[d])
            W[p, d] = hpref.fsub(hpref.chol(Sig), B)
            W64[p, d] = hpref._cpu_fsub64(np.linalg.cholesky(Sig), B)
        S[p], R[p] = hpref.gen_closure(hpref.gram(W[p, 0]))
    case = hpref.Case(P=P, D=D, F=F, mp=mp, A=A, diag=diag, RHS=RHS, S=S, R=R,
                      W=W, W64=W64)
    _CASES[key] = case
    return case


@pytest.mark.parametrize("gsign", [1.0, -1.0], ids=["direct", "compressed"])
@pytest.mark.parametrize("lead", [4, 8, 12])
@pytest.mark.parametrize("nbt", range(1, 5))
def test_skip_neutral_and_unpadded_result(nbt, lead, gsign):
    """P = 2, D = 5 in slices of 2, F = T + 1 (a full tile and a
    one-frequency tile): lead = k equals lead = 0 bit for bit, and both
    are the Fp of the unpadded system."""
    ext = _ext()
    case = _case(nbt, lead)
    L, invd = ext.chol_batch(_t(case.A), _t(case.diag), case.mp)
    args = (L, invd, _t(case.RHS), _t(case.S), _t(case.R))
    shape = (P, D, case.F)
    full = torch.full(shape, float("nan"), dtype=torch.float64, device=DEV)
    skip = torch.full(shape, float("nan"), dtype=torch.float64, device=DEV)
    ext.trsm_fp_store(*args, full, gsign, DPB, lead=0)
    ext.trsm_fp_store(*args, skip, gsign, DPB, lead=lead)
    got = skip.cpu().numpy()
    assert np.isfinite(got).all(), "entries left unwritten"
    _, _, fr, fb = hpref.solve_refs(case, gsign)
    for p in range(P):
        for d in range(D):
            label = f"lead={lead} NBT={nbt} g={gsign:+.0f} p={p} d={d} fp"
            err, tol = hpref.report(label, hpref.nerr(got[p, d], fr[p, d]),
                                    hpref.nerr(fb[p, d], fr[p, d]))
            assert err <= tol, f"{label}: {err:.3e} > tol {tol:.3e}"
    assert torch.equal(skip, full), "lead changes bits against lead = 0"


def test_lead_out_of_range_raises():
    """A lead that is negative, above 12 or no multiple of 4 raises
    before any launch and leaves no error behind."""
    ext = _ext()
    case = _case(2, 4)
    L, invd = ext.chol_batch(_t(case.A), _t(case.diag), case.mp)
    args = (L, invd, _t(case.RHS), _t(case.S), _t(case.R))
    out = torch.full((P, D, case.F), 7.0, dtype=torch.float64, device=DEV)
    for bad in (-4, 2, 5, 13, 16):
        with pytest.raises(RuntimeError):
            ext.trsm_fp_store(*args, out, -1.0, DPB, lead=bad)
    torch.cuda.synchronize()
    assert bool((out == 7.0).all()), "a rejected call wrote to out"
    ref = torch.empty_like(out)
    ext.trsm_fp_store(*args, ref, -1.0, DPB, lead=0)
    ext.trsm_fp_store(*args, out, -1.0, DPB, lead=4)
    torch.cuda.synchronize()
    assert torch.equal(out, ref)


@pytest.mark.parametrize("comps,lead", [(10, 12), (30, 4)],
                         ids=["mv20-lead12", "mv60-lead4"])
def test_engine_stack_leads_with_the_pad(comps, lead):
    """Three pulsars, 13 frequencies, D = 5 draws in chunks of 2 with
    the draw loop eligible for every chunk: mv = 20 (mp = 32) and
    mv = 60 (mp = 64, the flagship's block shape).  Against the CPU
    eager engine at 1e-6 of the spectrum scale (the bound of the
    engine's compressed-against-CPU tests); two runs and the unchunked
    run agree bit for bit; every solve received lead = mp - mv."""
    from fastfp_amd import FpEngine, get_mats_nmfp, initialize_pta, \
        make_synthetic_pta

    psrs = make_synthetic_pta(npsr=3, ntoa=500, ntm=10, seed=51,
                              ragged=False)
    noise = {"gw_gamma": 13.0 / 3.0, "gw_log10_A": float(np.log10(2e-15))}
    for p in psrs:
        noise[f"{p.name}_red_noise_gamma"] = 4.0
        noise[f"{p.name}_red_noise_log10_A"] = -14.5
    pta = initialize_pta(psrs, noise, inc_cp=True, rn_comps=comps,
                         gwb_comps=comps)
    TNTs, Nvecs, Ts = get_mats_nmfp(pta, noise)
    nd = 5
    rng = np.random.default_rng(5)
    pars = {
        n: (rng.uniform(2, 6, nd) if n.endswith("gamma")
            else rng.uniform(-16, -14, nd))
        for n in pta.params
    }
    phiinvs = [c.get_phiinv(pars).numpy() for c in pta.rn_containers]
    freqs = np.linspace(4e-9, 6e-8, 13)
    var_slices = [c.var_slice for c in pta.rn_containers]
    fixed = [c.get_phiinv(noise) for c in pta.rn_containers]

    cpu = FpEngine(psrs, Nvecs, Ts, device="cpu").precompute(freqs)
    cpu.enable_draw_compression(var_slices, fixed)
    want = cpu.sweep(phiinvs=phiinvs, draw_chunk=2).numpy()

    eng = FpEngine(psrs, Nvecs, Ts, device=DEV).precompute(freqs)
    eng.enable_draw_compression(var_slices, fixed)
    st = eng._comp_stack
    assert st is not None
    mv = 2 * comps
    mp = mv + lead
    assert st.lead == lead and st.A.shape[-2:] == (mp, mp)
    assert st.RHS.shape[1] == mp
    assert all(b.comp.A.shape[-1] == mv and b.comp.lead == 0
               for b in eng.blocks), "the pad belongs to the stack only"
    top = st.A[:, :lead]
    eye = torch.eye(lead, dtype=torch.float64, device=DEV)
    assert torch.equal(top[:, :, :lead], eye.expand(3, lead, lead))
    assert not bool(top[:, :, lead:].any())
    assert not bool(st.A[:, lead:, :lead].any())
    assert not bool(st.RHS[:, :lead].any())

    eng.DRAW_LOOP_MIN_DRAWS = 1
    leads = []
    real = eng._ext

    def store(*a, **k):
        leads.append(k.get("lead"))
        return real.trsm_fp_store(*a, **k)

    eng._ext = types.SimpleNamespace(
        chol_batch=real.chol_batch, chol_batch_into=real.chol_batch_into,
        trsm_fp_store=store, trsm_fp_accum=real.trsm_fp_accum)
    a = eng.sweep(phiinvs=phiinvs, draw_chunk=2)
    b = eng.sweep(phiinvs=phiinvs, draw_chunk=2)
    one = eng.sweep(phiinvs=phiinvs, draw_chunk=8)  # un-pipelined loop
    assert leads == [lead] * 7, leads
    assert torch.equal(a, b)
    assert torch.equal(a, one)
    err = np.abs(a.cpu().numpy() - want).max() / np.abs(want).max()
    print("max|gpu - cpu| / max|cpu| =", err)
    assert err < 1e-6
