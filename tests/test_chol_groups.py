"""``chol_batch_kernel`` across draws and pulsars of one launch.

The diagonal factor broadcasts along 16-lane rows by DPP, and a launch
lays (pulsar, draw) out over the grid; a kernel that packs several
draws of a pulsar into one workgroup (one per 16-lane row, measured and
not kept, docs/TUNING_NOTES.md) has to pass the same file.

1. Position independence, exact: a draw's ``L`` and ``invd`` are the
   same bits whether it is factored alone or as any draw of a larger
   call, next to draws of very different scale.
2. The longdouble oracle (tests/hpref.py) under the 16x rule of
   tests/test_solve_templates.py, and the exact structure, for every D.
3. NBT 5..8 (512 threads): ``chol_batch_into`` a pre-filled buffer
   equals ``chol_batch`` bit for bit.

D = 1, 2, 3, 5, 9 with P = 2 puts a draw at every position of a group
of 2 or 4, with partly filled and full groups and the last draws of
pulsar 0 next to the first of pulsar 1."""

import numpy as np
import pytest
import torch

import hpref

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
P = 2
DRAWS = (1, 2, 3, 5, 9)
DMAX = max(DRAWS)


def _ext():
    from fastfp_amd import ops

    ops.require_hip()
    from fastfp_amd.ops import _fastfp_hip

    return _fastfp_hip


def _t(a):
    return torch.tensor(np.asarray(a, dtype=np.float64), device=DEV)


def _m(nbt, short):
    return 16 * nbt - 15 if short else 16 * nbt


_SHAPES = pytest.mark.parametrize(
    "short", [False, True], ids=["m=mp", "m=mp-15"])


# ----------------------------------------------------------------------
# 1. position independence
# ----------------------------------------------------------------------
@_SHAPES
@pytest.mark.parametrize("nbt", range(1, 5))
def test_group_position_independence(nbt, short):
    """Draw d's phiinv is scaled by 10**(-3 + 0.75 d), 1e-3 .. 1e3 over
    the nine draws, so no two matrices of a call are alike and a draw
    factored from its neighbour's matrix cannot pass."""
    ext = _ext()
    mp, m = 16 * nbt, _m(nbt, short)
    case = hpref.factor_case(m, P=P, D=DMAX)
    scale = 10.0 ** np.linspace(-3.0, 3.0, DMAX)
    TNT = _t(case.TNT)
    phiinv = _t(case.phiinv * scale[None, :, None])
    alone = [[ext.chol_batch(TNT[p], phiinv[p, d:d + 1].contiguous(), mp)
              for d in range(DMAX)] for p in range(P)]
    for p in range(P):
        for d in range(1, DMAX):  # the scaling took: the draws differ
            assert not torch.equal(alone[p][d][0], alone[p][0][0])
    for D in DRAWS:
        L, invd = ext.chol_batch(TNT, phiinv[:, :D].contiguous(), mp)
        assert L.shape == (P * D, mp, mp)
        assert invd.shape == (P * D, nbt, 16, 16)
        for p in range(P):
            for d in range(D):
                b = p * D + d
                L1, i1 = alone[p][d]
                tag = f"NBT={nbt} m={m} D={D} p={p} d={d}"
                assert torch.equal(L[b], L1[0]), tag + " L"
                assert torch.equal(invd[b], i1[0]), tag + " invd"


# ----------------------------------------------------------------------
# 2. oracle and structure
# ----------------------------------------------------------------------
def _check(label, got, ref, base64):
    err, tol = hpref.report(label, hpref.nerr(got, ref),
                            hpref.nerr(base64, ref))
    assert err <= tol, f"{label}: {err:.3e} > tol {tol:.3e}"


_REFS = {}


def _refs(case, mp, p, d):
    """Oracle and plain-fp64 block inverses of one (pulsar, draw),
    computed once per case."""
    key = (id(case), mp, p, d)
    if key not in _REFS:
        _REFS[key] = (
            hpref.diag_block_inverses(hpref.padded(case.Lref[p, d], mp)),
            hpref.block_inverses64(hpref.padded(case.L64[p, d], mp)))
    return _REFS[key]


def _check_oracle(nbt, short, flavour):
    ext = _ext()
    mp, m = 16 * nbt, _m(nbt, short)
    case = hpref.factor_case(m, P=P, D=DMAX, flavour=flavour)
    for D in DRAWS:
        L, invd = ext.chol_batch(
            _t(case.TNT), _t(np.ascontiguousarray(case.phiinv[:, :D])), mp)
        L, invd = L.cpu().numpy(), invd.cpu().numpy()
        for p in range(P):
            for d in range(D):
                b = p * D + d
                tag = f"chol NBT={nbt} m={m} {flavour} D={D} p={p} d={d}"
                _check(tag + " L", np.tril(L[b, :m, :m]), case.Lref[p, d],
                       case.L64[p, d])
                assert (np.triu(L[b], 1) == 0).all(), tag + " upper"
                assert (L[b, m:, m:] == np.eye(mp - m)).all(), tag + " pad"
                assert (L[b, m:, :m] == 0).all(), tag + " pad rows"
                ref, base = _refs(case, mp, p, d)
                for kb in range(nbt):
                    _check(f"{tag} invd[{kb}]", invd[b, kb], ref[kb],
                           base[kb])


@_SHAPES
@pytest.mark.parametrize("nbt", range(1, 5))
def test_group_oracle(nbt, short):
    for flavour in (["plain", "range"] if nbt in (2, 4) else ["plain"]):
        _check_oracle(nbt, short, flavour)


# ----------------------------------------------------------------------
# 3. NBT 5..8
# ----------------------------------------------------------------------
@_SHAPES
@pytest.mark.parametrize("nbt", range(5, 9))
def test_into_equals_alloc_large(nbt, short):
    ext = _ext()
    mp, m, D = 16 * nbt, _m(nbt, short), 3
    case = hpref.factor_case(m, P=P, D=D)
    TNT, phiinv = _t(case.TNT), _t(case.phiinv)
    L, invd = ext.chol_batch(TNT, phiinv, mp)
    L2 = torch.full((P * D, mp, mp), float("nan"), dtype=torch.float64,
                    device=DEV)
    i2 = torch.full((P * D, nbt, 16, 16), float("nan"), dtype=torch.float64,
                    device=DEV)
    ext.chol_batch_into(TNT, phiinv, mp, L2, i2)
    assert torch.isfinite(L).all() and torch.isfinite(invd).all()
    assert torch.equal(L, L2), f"NBT={nbt} m={m} L"
    assert torch.equal(invd, i2), f"NBT={nbt} m={m} invd"
