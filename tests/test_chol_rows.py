"""``chol_rows_into``: the batched factor with its diagonal read from
strided prior rows of one ``(P, D, width)`` tensor, against
``chol_batch_into`` fed with ``SolveSystem.diag`` of the gathered rows.
Same operations in the same order: ``L`` and ``invd`` are compared with
``torch.equal``."""

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
NTM = 5  # columns in front of the variable ones in the compressed cases
EXTRA = 4  # draws of the base behind the ones factored


def _ext():
    from fastfp_amd import ops

    ops.require_hip()
    from fastfp_amd.ops import _fastfp_hip

    return _fastfp_hip


def _spd(rng, P, n):
    X = rng.normal(size=(P, n, 2 * n + 3))
    return X @ X.transpose(0, 2, 1) / (2 * n + 3) + 0.1 * np.eye(n)


def _t(a):
    return torch.tensor(np.asarray(a, dtype=np.float64), device=DEV)


def _both(A, base, sy, var0, d0, D, mp):
    """(L, invd) of the existing entry on sy.diag(gathered rows) and of
    chol_rows_into on the rows in place; outputs pre-filled with NaN."""
    ext = _ext()
    P, m = A.shape[0], A.shape[-1]
    mv = m - sy.lead
    out = [torch.full((P * D, mp, mp), float("nan"), dtype=torch.float64,
                      device=DEV) for _ in range(2)]
    inv = [torch.full((P * D, mp // 16, 16, 16), float("nan"),
                      dtype=torch.float64, device=DEV) for _ in range(2)]
    pinv = torch.stack([base[p][d0:d0 + D, var0:var0 + mv] for p in range(P)])
    ext.chol_batch_into(A, sy.diag(pinv).contiguous(), mp, out[0], inv[0])
    ext.chol_rows_into(A, base[0], base.stride(0), d0, D, var0, sy.delta0,
                       sy.lead, mp, out[1], inv[1])
    torch.cuda.synchronize()
    assert torch.isfinite(out[0]).all() and torch.isfinite(inv[0]).all()
    return out, inv


@pytest.mark.parametrize("d0", [0, 3])
@pytest.mark.parametrize("D", [1, 2, 33])
@pytest.mark.parametrize("P", [1, 3])
@pytest.mark.parametrize("mv,lead,mp", [(12, 4, 16), (17, 15, 32),
                                        (28, 4, 32), (48, 0, 48),
                                        (60, 4, 64), (61, 3, 64),
                                        (24, 8, 32)])
def test_compressed_rows_equal_diag_entry(mv, lead, mp, P, D, d0):
    """The stacked compressed system: A = blockdiag(I_lead, G), diagonal
    0 on the lead and 1 / (rows - delta0) behind it.  The rows entry
    leaves the lead's whole 4-step groups out of diagonal block 0 (4, 12,
    4, none, 4, none and 8 steps), the reference entry factors them:
    every bit of L and invd is the same, the sign of exact zeros aside."""
    from fastfp_amd.engine import SolveSystem

    assert lead + mv == mp
    rng = np.random.default_rng([mv, P, D, d0])
    A = np.zeros((P, mp, mp))
    A[:, :lead, :lead] = np.eye(lead)
    A[:, lead:, lead:] = _spd(rng, P, mv)
    base = _t(10.0 ** rng.uniform(-2, 2, (P, d0 + D + EXTRA, NTM + mv)))
    delta0 = _t(1e-3 * rng.uniform(0.1, 1.0, (P, mv)))
    sy = SolveSystem(_t(A), None, None, None, -1.0,
                     var=[slice(NTM, NTM + mv)] * P, delta0=delta0, lead=lead)
    (L0, L1), (i0, i1) = _both(sy.A, base, sy, NTM, d0, D, mp)
    assert torch.equal(L1, L0)
    assert torch.equal(i1, i0)


@pytest.mark.parametrize("d0", [0, 3])
@pytest.mark.parametrize("D", [1, 2, 33])
@pytest.mark.parametrize("P", [1, 3])
@pytest.mark.parametrize("m", [12, 17, 48, 60, 61, 120])
def test_direct_rows_equal_diag_entry(m, P, D, d0):
    """The direct stack: no delta0, no lead, the rows themselves on the
    diagonal; m below mp leaves the identity pad behind."""
    from fastfp_amd import ops
    from fastfp_amd.engine import SolveSystem

    mp = ops.pad16(m)
    rng = np.random.default_rng([m, P, D, d0, 1])
    base = _t(10.0 ** rng.uniform(-2, 2, (P, d0 + D + EXTRA, m)))
    sy = SolveSystem(_t(_spd(rng, P, m)), None, None, None, 1.0)
    (L0, L1), (i0, i1) = _both(sy.A, base, sy, 0, d0, D, mp)
    assert torch.equal(L1, L0)
    assert torch.equal(i1, i0)


def test_rows_outside_the_storage_raise():
    """Draw, column and pulsar ranges that leave the rows' storage raise
    before any launch."""
    ext = _ext()
    rng = np.random.default_rng(3)
    P, D, m = 2, 3, 16
    A = _t(_spd(rng, P, m))
    base = _t(rng.uniform(1, 2, (P, D, m)))
    L = torch.full((P * D, 16, 16), 7.0, dtype=torch.float64, device=DEV)
    invd = torch.full((P * D, 1, 16, 16), 7.0, dtype=torch.float64,
                      device=DEV)
    for kw in (dict(d0=1), dict(var0=1), dict(pstride=2 * D * m),
               dict(d0=-1), dict(row0=base[0].cpu())):
        args = dict(TNT=A, row0=base[0], pstride=base.stride(0), d0=0, D=D,
                    var0=0, delta0=None, lead=0, mp=16, L=L, invd=invd)
        args.update(kw)
        with pytest.raises(RuntimeError):
            ext.chol_rows_into(**args)
    torch.cuda.synchronize()
    assert bool((L == 7.0).all()) and bool((invd == 7.0).all())
