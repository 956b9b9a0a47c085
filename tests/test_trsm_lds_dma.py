"""The draw-looping solve gathers each draw's factor from ``L`` and
``invd`` straight into LDS and negates the strict-lower panels in the
MFMA.

``trsm_fp_store`` / ``trsm_prods_store`` (trsm_fp_draws_kernel) must
give the numbers of the one-draw kernels bit for bit: ``trsm_fp_accum``
into zeros and ``trsm_prods``, which tests/test_solve_templates.py holds
against the longdouble oracle.  Every comparison below is
``torch.equal``; there is no tolerance.

The systems are factored on the device.  With ``lead`` > 0 they start
with a ``lead`` x ``lead`` identity block over ``lead`` zero RHS rows,
which is what the kernel is promised (tests/test_trsm_lead_pad.py)."""

import numpy as np
import pytest
import torch

import hpref

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
NAN = float("nan")


def _ext():
    from fastfp_amd import ops

    ops.require_hip()
    from fastfp_amd.ops import _fastfp_hip

    return _fastfp_hip


def _t(a):
    return torch.tensor(np.asarray(a, dtype=np.float64), device=DEV)


_SYSTEMS = {}


def _system(nbt, lead, P, D, F):
    """Device inputs (L, invd, RHS, S, R) of one padded system, built
    once per key, shared, never modified.  S and R close draw 0's plain
    fp64 solve without cancellation (hpref.gen_closure); the other draws
    perturb it by 1e-4."""
    key = (nbt, lead, P, D, F)
    if key in _SYSTEMS:
        return _SYSTEMS[key]
    mp = 16 * nbt
    mv = mp - lead
    rng = np.random.default_rng([11, nbt, lead, P, D, F])
    A = np.zeros((P, mp, mp))
    diag = np.zeros((P, D, mp))
    RHS = np.zeros((P, mp, 2 * F + 1))
    S, R = np.empty((P, 3, F)), np.empty((P, 2, F))
    for p in range(P):
        TNT, phiinv = hpref.gen_sigma(rng, mv, D)
        A[p, :lead, :lead] = np.eye(lead)
        A[p, lead:, lead:] = TNT
        diag[p, :, lead:] = phiinv
        B = hpref.gen_rhs(rng, mv, mv, F)
        RHS[p, lead:] = B
        L64 = np.linalg.cholesky(hpref.sigma_of(TNT, phiinv[0]))
        S[p], R[p] = hpref.gen_closure(
            hpref.gram(hpref._cpu_fsub64(L64, B), np.float64))
    L, invd = _ext().chol_batch(_t(A), _t(diag), mp)
    sys_ = (L, invd, _t(RHS), _t(S), _t(R))
    _SYSTEMS[key] = sys_
    return sys_


def _one_draw(sys_, prods, gsign, P, D, F):
    """The yardstick: the unchanged one-draw kernels."""
    ext = _ext()
    if prods:
        ref = torch.full((P, D, 5, F), NAN, dtype=torch.float64, device=DEV)
        ext.trsm_prods(*sys_, ref, gsign)
    else:
        ref = torch.zeros((P, D, F), dtype=torch.float64, device=DEV)
        ext.trsm_fp_accum(*sys_, ref, gsign)
    assert bool(torch.isfinite(ref).all()), "the reference is not finite"
    return ref


def _draws(sys_, prods, gsign, P, D, F, dpb, lead):
    """The kernel under test into a NaN-filled output."""
    ext = _ext()
    shape = (P, D, 5, F) if prods else (P, D, F)
    out = torch.full(shape, NAN, dtype=torch.float64, device=DEV)
    store = ext.trsm_prods_store if prods else ext.trsm_fp_store
    store(*sys_, out, gsign, dpb, lead=lead)
    return out


@pytest.mark.parametrize("gsign", [1.0, -1.0], ids=["direct", "compressed"])
@pytest.mark.parametrize("prods", [False, True], ids=["fp", "prods"])
@pytest.mark.parametrize("lead", [0, 4, 8, 12])
@pytest.mark.parametrize("nbt", range(1, 5))
def test_every_instantiation_equals_one_draw_kernel(nbt, lead, prods, gsign):
    """NBT 1..4 x lead 0..12 x Fp/products x gsign, P = 2, D = 3, F = 5,
    the three draws in one slice: both buffer parities, a last draw with
    nothing to prefetch, and the second pulsar's offsets in the gather
    pointers."""
    P, D, F = 2, 3, 5
    sys_ = _system(nbt, lead, P, D, F)
    ref = _one_draw(sys_, prods, gsign, P, D, F)
    got = _draws(sys_, prods, gsign, P, D, F, D, lead)
    assert torch.equal(got, ref)


def _blocks(nbt):
    """(rb, cb) of the strict-lower 16x16 blocks, in staging order."""
    return [(rb, cb) for rb in range(1, nbt) for cb in range(rb)]


@pytest.mark.parametrize("prods", [False, True], ids=["fp", "prods"])
@pytest.mark.parametrize("nbt", [3, 4])
def test_gather_reads_the_strict_lower_blocks_and_nothing_else(nbt, prods):
    """NaN in L's diagonal blocks and in every block above them changes
    nothing: the kernel reads the strict-lower blocks of L and all of
    invd only.  Rotating the strict-lower blocks among themselves does
    change the output, so a gather from the wrong block would show."""
    P, D, F, lead = 2, 3, 5, 4
    L, invd, RHS, S, R = _system(nbt, lead, P, D, F)
    clean = _draws((L, invd, RHS, S, R), prods, -1.0, P, D, F, D, lead)
    assert torch.equal(clean,
                       _one_draw((L, invd, RHS, S, R), prods, -1.0, P, D, F))

    poisoned = L.clone()
    for rb in range(nbt):
        poisoned[:, rb * 16:(rb + 1) * 16, rb * 16:] = NAN
    got = _draws((poisoned, invd, RHS, S, R), prods, -1.0, P, D, F, D, lead)
    assert bool(torch.isfinite(got).all())
    assert torch.equal(got, clean)

    blocks = _blocks(nbt)
    rotated = L.clone()
    for (rb, cb), (sb, tb) in zip(blocks, blocks[1:] + blocks[:1]):
        rotated[:, rb * 16:(rb + 1) * 16, cb * 16:(cb + 1) * 16] = \
            L[:, sb * 16:(sb + 1) * 16, tb * 16:(tb + 1) * 16]
    moved = _draws((rotated, invd, RHS, S, R), prods, -1.0, P, D, F, D, lead)
    assert not torch.equal(moved, clean), "the test cannot fail"


@pytest.mark.parametrize("prods", [False, True], ids=["fp", "prods"])
@pytest.mark.parametrize("F", [1, 63, 64, 127])
@pytest.mark.parametrize("D,dpb", [(1, 1), (2, 1), (5, 2), (5, 8)])
def test_slices_and_frequency_tile_edges(D, dpb, F, prods):
    """The flagship instantiation (NBT = 4, lead = 4) over slices of one
    draw, slices with a one-draw tail and a slice longer than D, at the
    edges of the 63-frequency tile."""
    assert int(_ext().trsm_fp_store_tile_freqs()) == 63
    P, nbt, lead = 2, 4, 4
    sys_ = _system(nbt, lead, P, D, F)
    ref = _one_draw(sys_, prods, -1.0, P, D, F)
    got = _draws(sys_, prods, -1.0, P, D, F, dpb, lead)
    assert torch.equal(got, ref)


@pytest.mark.parametrize("prods", [False, True], ids=["fp", "prods"])
def test_two_launches_agree(prods):
    P, D, F, nbt, lead = 2, 5, 64, 4, 4
    sys_ = _system(nbt, lead, P, D, F)
    a = _draws(sys_, prods, -1.0, P, D, F, 2, lead)
    b = _draws(sys_, prods, -1.0, P, D, F, 2, lead)
    assert bool(torch.isfinite(a).all())
    assert torch.equal(a, b)
