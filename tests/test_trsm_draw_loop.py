"""The draw-looping solve ``trsm_fp_store`` (trsm_fp_draws_kernel<NBT>,
NBT 1..4): a workgroup keeps its RHS tile in registers over a slice of
draws and writes Fp with plain stores.

Every case starts ``out`` as NaN and is checked two ways: against the
longdouble oracle under the 16x rule of tests/hpref.py (the same rule
and the same CPU fp64 base as test_solve_templates.py), and with
``torch.equal`` against ``trsm_fp_accum`` accumulating into zeros — the
two kernels share their MFMA order, reduction and closure, so they must
agree bit for bit.  T is the kernel's frequencies per tile."""

import types

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


def _T():
    return int(_ext().trsm_fp_store_tile_freqs())


def _t(a):
    return torch.tensor(np.asarray(a, dtype=np.float64), device=DEV)


def _sq(case, a):
    """Single-pulsar cases use the unbatched signatures."""
    return a[0] if case.P == 1 else a


def _check_store(case, gsign, dpb, tag):
    ext = _ext()
    pr, pb, fr, fb = hpref.solve_refs(case, gsign)
    args = (_t(case.L), _t(case.invd), _t(_sq(case, case.RHS)),
            _t(_sq(case, case.S)), _t(_sq(case, case.R)))
    out = torch.full(_sq(case, fr).shape, float("nan"), dtype=torch.float64,
                     device=DEV)
    ext.trsm_fp_store(*args, out, gsign, dpb)
    old = torch.zeros_like(out)
    ext.trsm_fp_accum(*args, old, gsign)
    got = out.cpu().numpy().reshape(fr.shape)
    assert np.isfinite(got).all(), f"{tag}: entries left unwritten"
    for p in range(case.P):
        for d in range(case.D):
            label = f"{tag} g={gsign:+.0f} dpb={dpb} p={p} d={d} fp"
            err, tol = hpref.report(label, hpref.nerr(got[p, d], fr[p, d]),
                                    hpref.nerr(fb[p, d], fr[p, d]))
            assert err <= tol, f"{label}: {err:.3e} > tol {tol:.3e}"
    assert torch.equal(out, old), f"{tag}: differs from trsm_fp_accum"


@pytest.mark.parametrize("gsign", [1.0, -1.0], ids=["direct", "compressed"])
@pytest.mark.parametrize("nbt", range(1, 5))
def test_trsm_fp_store_every_nbt(nbt, gsign):
    """Every instantiation: P = 2 (m = mp and m = mp - 5), F = T + 1 (a
    full tile and a one-frequency tile), D = 5 in slices of 2, 2 and 1
    draws — both LDS buffers are used and the tail slice is one draw."""
    case = hpref.solve_case(nbt, _T() + 1, P=2, D=5)
    _check_store(case, gsign, 2, f"trsm_fp_store NBT={nbt}")


@pytest.mark.parametrize("k", ["1", "T-1", "T", "T+1", "2T", "2T+1"])
def test_trsm_fp_store_frequency_edges(k):
    """F around the tile width at NBT = 2, unbatched signatures, D = 3:
    the last live column pair, the u column and the dead column."""
    T = _T()
    F = {"1": 1, "T-1": T - 1, "T": T, "T+1": T + 1, "2T": 2 * T,
         "2T+1": 2 * T + 1}[k]
    case = hpref.solve_case(2, F, P=1, D=3)
    for gsign in (1.0, -1.0):
        for dpb in (2, 0):
            _check_store(case, gsign, dpb, f"trsm_fp_store NBT=2 F={F}")


@pytest.mark.parametrize("D,dpb", [(1, 1), (2, 1), (3, 2), (3, 8)],
                         ids=["one-draw", "slices-of-1", "tail-of-1",
                              "slice>D"])
def test_trsm_fp_store_slice_edges(D, dpb):
    """Slice lengths at NBT = 4, F = T + 1: the forced value, then the
    automatic choice (draws_per_block = 0)."""
    case = hpref.solve_case(4, _T() + 1, P=2, D=D)
    for gsign in (1.0, -1.0):
        _check_store(case, gsign, dpb, f"trsm_fp_store NBT=4 D={D}")
        _check_store(case, gsign, 0, f"trsm_fp_store NBT=4 D={D}")


def _empty(*shape):
    return torch.empty(shape, dtype=torch.float64, device=DEV)


def test_trsm_fp_store_empty_and_unsupported():
    """D = 0 or F = 0 returns without a launch and leaves no error
    behind; mp = 80 (no instantiation) raises before any launch; the
    next valid call passes its checks."""
    ext = _ext()
    case = hpref.solve_case(2, 1, P=1, D=2)
    mp, nbt, D = case.mp, 2, case.D
    L, invd, RHS = _t(case.L), _t(case.invd), _t(case.RHS[0])
    S, R = _t(case.S[0]), _t(case.R[0])
    ext.trsm_fp_store(_empty(0, mp, mp), _empty(0, nbt, 16, 16), RHS, S, R,
                      _empty(0, 1), 1.0)
    keep = torch.full((D, 0), 7.0, dtype=torch.float64, device=DEV)
    ext.trsm_fp_store(L, invd, _t(case.RHS[0][:, -1:]), _empty(3, 0),
                      _empty(2, 0), keep, 1.0, 3)
    with pytest.raises(RuntimeError):
        ext.trsm_fp_store(_empty(1, 80, 80), _empty(1, 5, 16, 16),
                          _empty(80, 3), _empty(3, 1), _empty(2, 1),
                          _empty(1, 1), 1.0)
    with pytest.raises(RuntimeError):
        ext.trsm_fp_store(L, invd, RHS, S, R, _empty(D, 1), 1.0, -1)
    torch.cuda.synchronize()
    _check_store(case, -1.0, 0, "after-empty trsm_fp_store")


def test_engine_stacked_sweep_uses_draw_loop():
    """A stacked compressed sweep (3 pulsars, 20 variable columns,
    mp = 32) over D = 5 draws in chunks of 2 — the factor/solve pipeline
    with a one-draw tail chunk — with the draw-looping kernel made
    eligible for every chunk.  Compared with the CPU eager engine at the
    tolerance of test_compressed_stacked_large_mv_multichunk_gpu; two
    runs agree bit for bit; every chunk went through trsm_fp_store."""
    from fastfp_amd import FpEngine, get_mats_nmfp, initialize_pta, \
        make_synthetic_pta

    psrs = make_synthetic_pta(npsr=3, ntoa=500, ntm=10, seed=51,
                              ragged=False)
    noise = {"gw_gamma": 13.0 / 3.0, "gw_log10_A": float(np.log10(2e-15))}
    for p in psrs:
        noise[f"{p.name}_red_noise_gamma"] = 4.0
        noise[f"{p.name}_red_noise_log10_A"] = -14.5
    pta = initialize_pta(psrs, noise, inc_cp=True, rn_comps=10,
                         gwb_comps=10)
    TNTs, Nvecs, Ts = get_mats_nmfp(pta, noise)
    D = 5
    rng = np.random.default_rng(5)
    pars = {
        n: (rng.uniform(2, 6, D) if n.endswith("gamma")
            else rng.uniform(-16, -14, D))
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
    assert eng._comp_stack is not None
    assert eng._comp_stack.A.shape[-1] <= 64
    eng.DRAW_LOOP_MIN_DRAWS = 1
    calls = {"store": 0, "accum": 0}
    real = eng._ext

    def counted(name, fn):
        def f(*a, **k):
            calls[name] += 1
            return fn(*a, **k)
        return f

    eng._ext = types.SimpleNamespace(
        chol_batch=real.chol_batch, chol_batch_into=real.chol_batch_into,
        trsm_fp_store=counted("store", real.trsm_fp_store),
        trsm_fp_accum=counted("accum", real.trsm_fp_accum))
    a = eng.sweep(phiinvs=phiinvs, draw_chunk=2)
    assert calls == {"store": 3, "accum": 0}, calls
    b = eng.sweep(phiinvs=phiinvs, draw_chunk=2)
    one = eng.sweep(phiinvs=phiinvs, draw_chunk=8)  # un-pipelined loop
    assert calls == {"store": 7, "accum": 0}, calls
    assert torch.equal(a, b)
    assert torch.equal(a, one)
    got = a.cpu().numpy()
    err = np.abs(got - want).max() / np.abs(want).max()
    print("max|gpu - cpu| / max|cpu| =", err)
    assert err < 1e-6
