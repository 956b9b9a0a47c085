"""The products mode of the draw-looping solve: ``trsm_prods_store``
(trsm_fp_draws_kernel<NBT, SKIP, true>, NBT 1..4, SKIP 0..3) stores the
five corrected products [M11, M22, M12, N1, N2] of every (pulsar, draw,
frequency) into ``out`` (P, D, 5, F) with plain stores.

Every case starts ``out`` as NaN and is checked two ways: each product
plane against the longdouble oracle under the 16x rule of tests/hpref.py
(the rule and the CPU fp64 base of test_solve_templates.py), and with
``torch.equal`` against ``trsm_prods`` on the same inputs — the two
kernels share their MFMA order, their reduction and the five closing
expressions, so they must agree bit for bit.  T is the kernel's
frequencies per tile."""

import numpy as np
import pytest
import torch

import hpref

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
NAMES = ["M11", "M22", "M12", "N1", "N2"]


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


def _nan(shape):
    return torch.full(tuple(shape), float("nan"), dtype=torch.float64,
                      device=DEV)


def _check_planes(tag, got, pr, pb):
    """Every (pulsar, draw, product) plane under the 16x rule."""
    assert np.isfinite(got).all(), f"{tag}: entries left unwritten"
    P, D = pr.shape[:2]
    for p in range(P):
        for d in range(D):
            for i in range(5):
                label = f"{tag} p={p} d={d} {NAMES[i]}"
                err, tol = hpref.report(
                    label, hpref.nerr(got[p, d, i], pr[p, d, i]),
                    hpref.nerr(pb[p, d, i], pr[p, d, i]))
                assert err <= tol, f"{label}: {err:.3e} > tol {tol:.3e}"


def _check_store(case, gsign, dpb, tag):
    ext = _ext()
    pr, pb, _, _ = hpref.solve_refs(case, gsign)
    args = (_t(case.L), _t(case.invd), _t(_sq(case, case.RHS)),
            _t(_sq(case, case.S)), _t(_sq(case, case.R)))
    out = _nan(_sq(case, pr).shape)
    ext.trsm_prods_store(*args, out, gsign, dpb)
    old = _nan(out.shape)
    ext.trsm_prods(*args, old, gsign)
    _check_planes(f"{tag} g={gsign:+.0f} dpb={dpb}",
                  out.cpu().numpy().reshape(pr.shape), pr, pb)
    assert torch.equal(out, old), f"{tag}: differs from trsm_prods"


@pytest.mark.parametrize("gsign", [1.0, -1.0], ids=["direct", "compressed"])
@pytest.mark.parametrize("nbt", range(1, 5))
def test_trsm_prods_store_every_nbt(nbt, gsign):
    """Every NBT: P = 2 (m = mp and m = mp - 5), F = T + 1 (a full tile
    and a one-frequency tile), D = 5 in slices of 2, 2 and 1 draws —
    both LDS buffers are used and the tail slice is one draw."""
    case = hpref.solve_case(nbt, _T() + 1, P=2, D=5)
    _check_store(case, gsign, 2, f"trsm_prods_store NBT={nbt}")


@pytest.mark.parametrize("k", ["1", "T-1", "T", "T+1", "2T", "2T+1"])
def test_trsm_prods_store_frequency_edges(k):
    """F around the tile width at NBT = 2, unbatched signatures, D = 3:
    the last live column pair, the u column and the dead column."""
    T = _T()
    F = {"1": 1, "T-1": T - 1, "T": T, "T+1": T + 1, "2T": 2 * T,
         "2T+1": 2 * T + 1}[k]
    case = hpref.solve_case(2, F, P=1, D=3)
    for gsign in (1.0, -1.0):
        for dpb in (2, 0):
            _check_store(case, gsign, dpb, f"trsm_prods_store NBT=2 F={F}")


@pytest.mark.parametrize("D,dpb", [(1, 1), (2, 1), (3, 2), (3, 8)],
                         ids=["one-draw", "slices-of-1", "tail-of-1",
                              "slice>D"])
def test_trsm_prods_store_slice_edges(D, dpb):
    """Slice lengths at NBT = 4, F = T + 1: the forced value, then the
    automatic choice (draws_per_block = 0)."""
    case = hpref.solve_case(4, _T() + 1, P=2, D=D)
    for gsign in (1.0, -1.0):
        _check_store(case, gsign, dpb, f"trsm_prods_store NBT=4 D={D}")
        _check_store(case, gsign, 0, f"trsm_prods_store NBT=4 D={D}")


# ----------------------------------------------------------------------
# leading pad (SKIP 1..3)
# ----------------------------------------------------------------------
P, D, DPB = 2, 5, 2  # slices of 2, 2 and 1 draws: both LDS buffers, a tail
_LEAD_CASES = {}


def _lead_case(nbt, lead):
    """A real system of size mp - lead under a lead x lead identity
    block over lead zero RHS rows, with the references of the unpadded
    system (the recipe of test_trsm_lead_pad.py); built once per
    (nbt, lead), shared, never modified."""
    key = (nbt, lead)
    if key in _LEAD_CASES:
        return _LEAD_CASES[key]
    F = _T() + 1
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
    _LEAD_CASES[key] = case
    return case


@pytest.mark.parametrize("gsign", [1.0, -1.0], ids=["direct", "compressed"])
@pytest.mark.parametrize("lead", [4, 8, 12])
@pytest.mark.parametrize("nbt", range(1, 5))
def test_trsm_prods_store_lead(nbt, lead, gsign):
    """Every NBT x SKIP: lead = k equals lead = 0 equals ``trsm_prods``
    on the padded system, bit for bit, and all are the products of the
    unpadded system."""
    ext = _ext()
    case = _lead_case(nbt, lead)
    L, invd = ext.chol_batch(_t(case.A), _t(case.diag), case.mp)
    args = (L, invd, _t(case.RHS), _t(case.S), _t(case.R))
    shape = (P, D, 5, case.F)
    full, skip, old = _nan(shape), _nan(shape), _nan(shape)
    ext.trsm_prods_store(*args, full, gsign, DPB, lead=0)
    ext.trsm_prods_store(*args, skip, gsign, DPB, lead=lead)
    ext.trsm_prods(*args, old, gsign)
    pr, pb, _, _ = hpref.solve_refs(case, gsign)
    _check_planes(f"lead={lead} NBT={nbt} g={gsign:+.0f}",
                  skip.cpu().numpy(), pr, pb)
    assert torch.equal(skip, full), "lead changes bits against lead = 0"
    assert torch.equal(full, old), "differs from trsm_prods"


# ----------------------------------------------------------------------
# empty and unsupported
# ----------------------------------------------------------------------
def _empty(*shape):
    return torch.empty(shape, dtype=torch.float64, device=DEV)


def test_trsm_prods_store_empty_and_unsupported():
    """D = 0 or F = 0 returns without a launch and leaves no error
    behind; mp = 80 (no instantiation), a lead of 5 or 16 and a negative
    draws_per_block raise before any launch and write nothing; the next
    valid call passes its checks."""
    ext = _ext()
    case = hpref.solve_case(2, 1, P=1, D=2)
    mp, nbt, nd = case.mp, 2, case.D
    L, invd, RHS = _t(case.L), _t(case.invd), _t(case.RHS[0])
    S, R = _t(case.S[0]), _t(case.R[0])
    ext.trsm_prods_store(_empty(0, mp, mp), _empty(0, nbt, 16, 16), RHS, S, R,
                         _empty(0, 5, 1), 1.0)
    ext.trsm_prods_store(L, invd, _t(case.RHS[0][:, -1:]), _empty(3, 0),
                         _empty(2, 0), _empty(nd, 5, 0), 1.0, 3)
    with pytest.raises(RuntimeError):
        ext.trsm_prods_store(_empty(1, 80, 80), _empty(1, 5, 16, 16),
                             _empty(80, 3), _empty(3, 1), _empty(2, 1),
                             _empty(1, 5, 1), 1.0)
    keep = torch.full((nd, 5, 1), 7.0, dtype=torch.float64, device=DEV)
    for lead in (5, 16):
        with pytest.raises(RuntimeError):
            ext.trsm_prods_store(L, invd, RHS, S, R, keep, 1.0, 0, lead=lead)
    with pytest.raises(RuntimeError):
        ext.trsm_prods_store(L, invd, RHS, S, R, keep, 1.0, -1)
    torch.cuda.synchronize()
    assert bool((keep == 7.0).all()), "a rejected call wrote to out"
    _check_store(case, -1.0, 0, "after-empty trsm_prods_store")
