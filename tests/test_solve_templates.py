"""Every instantiation of the per-draw solve kernels against the
longdouble oracle (tests/hpref.py).

``chol_batch_kernel<NBT>`` (NBT 1..8), ``trsm_fp_kernel<NBT,1>`` and its
products mode (NBT 1..8), ``trsm_fp_rl_kernel<NBT>`` (NBT 9..16) and
``diag_inv`` are each a separate piece of generated code; every one is
run here, in isolation where it can be, at tiny shapes.

Tolerance rule (hpref.tol_from_base): every comparison is normwise per
plane, ``max|got - ref| / max|ref|``, and must stay within
``16 * max(base, 64 eps)`` where ``base`` is the same error of a plain
CPU fp64 evaluation (numpy.linalg.cholesky, scipy solve_triangular,
numpy fp64 products) against the same oracle.  Structural facts are
exact equalities.  Each case prints got / base / tol; the measured
ratios are tabulated in docs/VALIDATION.md."""

import numpy as np
import pytest
import torch

import hpref
from hpref import LD

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def _ext():
    from fastfp_amd import ops

    ops.require_hip()
    from fastfp_amd.ops import _fastfp_hip

    return _fastfp_hip


def _t(a):
    return torch.tensor(np.asarray(a, dtype=np.float64), device=DEV)


def _np(t):
    return t.detach().cpu().numpy()


def _check(label, got, ref, base64):
    """One plane: kernel error vs the CPU fp64 error, both against the
    oracle, under the 16x rule."""
    err, tol = hpref.report(label, hpref.nerr(got, ref),
                            hpref.nerr(base64, ref))
    assert err <= tol, f"{label}: {err:.3e} > tol {tol:.3e}"


# ----------------------------------------------------------------------
# chol_batch_kernel<NBT>, NBT = 1..8
# ----------------------------------------------------------------------
def _check_chol(nbt, short, flavour, P=2, D=3):
    ext = _ext()
    mp = 16 * nbt
    m = mp - 15 if short else mp
    case = hpref.factor_case(m, P=P, D=D, flavour=flavour)
    L, invd = ext.chol_batch(_t(case.TNT), _t(case.phiinv), mp)
    assert L.shape == (P * D, mp, mp) and invd.shape == (P * D, nbt, 16, 16)
    L, invd = _np(L), _np(invd)
    for p in range(P):
        for d in range(D):
            b = p * D + d  # pulsar-major batch order
            tag = f"chol NBT={nbt} m={m} {flavour} p={p} d={d}"
            _check(tag + " L", np.tril(L[b, :m, :m]), case.Lref[p, d],
                   case.L64[p, d])
            # structure: exact
            assert (np.triu(L[b], 1) == 0).all(), tag + " upper"
            assert (L[b, m:, m:] == np.eye(mp - m)).all(), tag + " pad"
            assert (L[b, m:, :m] == 0).all(), tag + " pad rows"
            ref = hpref.diag_block_inverses(
                hpref.padded(case.Lref[p, d], mp))
            base = hpref.block_inverses64(hpref.padded(case.L64[p, d], mp))
            for kb in range(nbt):
                _check(f"{tag} invd[{kb}]", invd[b, kb], ref[kb], base[kb])


@pytest.mark.parametrize("short", [False, True], ids=["m=mp", "m=mp-15"])
@pytest.mark.parametrize("nbt", range(1, 9))
def test_chol_batch_every_nbt(nbt, short):
    """Pulsar-batched (P=2, D=3) factor at m = mp (no padding) and
    m = mp - 15 (one live row in the last block; m = 1 at NBT = 1);
    mp <= 64 launches 256 threads, above 512, NBT = 1 takes the nb = 1
    early break.  The 1e-40 / 1e12..1e18 prior spread joins at NBT 2,
    4, 5 and 8."""
    for flavour in (["plain", "range"] if nbt in (2, 4, 5, 8) else ["plain"]):
        _check_chol(nbt, short, flavour)


# ----------------------------------------------------------------------
# trsm_fp_kernel<NBT,1> (1..8) / trsm_fp_rl_kernel<NBT> (9..16)
# ----------------------------------------------------------------------
def _pattern(fr):
    """Nonzero fp64 pre-fill for the accumulating kernel, of the size
    of Fp itself so neither term hides the other."""
    scale = 0.125 * float(np.abs(fr).max())
    idx = np.arange(fr.size).reshape(fr.shape)
    return scale * (1.0 + idx % 7)


def _squeeze(case, a):
    """Single-pulsar cases use the unbatched signatures."""
    return a[0] if case.P == 1 else a


def _check_trsm_fp(case, gsign, tag):
    ext = _ext()
    pr, pb, fr, fb = hpref.solve_refs(case, gsign)
    pat = _pattern(fr)
    fp = _t(_squeeze(case, pat))
    ext.trsm_fp_accum(_t(case.L), _t(case.invd), _t(_squeeze(case, case.RHS)),
                      _t(_squeeze(case, case.S)), _t(_squeeze(case, case.R)),
                      fp, gsign)
    got = _np(fp).reshape(fr.shape)
    ref = pat.astype(LD) + fr  # accumulated, not overwritten
    for p in range(case.P):
        for d in range(case.D):
            _check(f"{tag} g={gsign:+.0f} p={p} d={d} fp", got[p, d],
                   ref[p, d], pat[p, d] + fb[p, d])


def _check_trsm_prods(case, gsign, tag):
    ext = _ext()
    pr, pb, fr, fb = hpref.solve_refs(case, gsign)
    out = torch.full(_squeeze(case, pr).shape, float("nan"),
                     dtype=torch.float64, device=DEV)
    ext.trsm_prods(_t(case.L), _t(case.invd), _t(_squeeze(case, case.RHS)),
                   _t(_squeeze(case, case.S)), _t(_squeeze(case, case.R)),
                   out, gsign)
    got = _np(out).reshape(pr.shape)
    assert np.isfinite(got).all(), f"{tag}: entries left unwritten"
    names = ["M11", "M22", "M12", "N1", "N2"]
    for p in range(case.P):
        for d in range(case.D):
            for i in range(5):
                _check(f"{tag} g={gsign:+.0f} p={p} d={d} {names[i]}",
                       got[p, d, i], pr[p, d, i], pb[p, d, i])


@pytest.mark.parametrize("gsign", [1.0, -1.0], ids=["direct", "compressed"])
@pytest.mark.parametrize("nbt", range(1, 17))
def test_trsm_fp_accum_every_nbt(nbt, gsign):
    """The solve alone: L and invd are the oracle's (rounded to fp64,
    identity-padded), P = 2 (m = mp and m = mp - 5), D = 2, F = 64 —
    one full 63-frequency tile plus a one-frequency tile."""
    _check_trsm_fp(hpref.solve_case(nbt, 64), gsign, f"trsm_fp NBT={nbt}")


@pytest.mark.parametrize("gsign", [1.0, -1.0], ids=["direct", "compressed"])
@pytest.mark.parametrize("nbt", range(1, 9))
def test_trsm_prods_every_nbt(nbt, gsign):
    """Products mode on the same inputs; ``out`` starts as NaN, so the
    plain stores must cover every entry."""
    _check_trsm_prods(hpref.solve_case(nbt, 64), gsign,
                      f"trsm_prods NBT={nbt}")


@pytest.mark.parametrize("F", [1, 62, 63, 64, 126, 127])
@pytest.mark.parametrize("nbt", [2, 9])
def test_trsm_frequency_tile_edges(nbt, F):
    """F around the 63-frequency tile: the last live column pair, the
    u column at block column 126 and the dead column 127 (unbatched
    signatures, D = 2)."""
    case = hpref.solve_case(nbt, F, P=1, D=2)
    for gsign in (1.0, -1.0):
        _check_trsm_fp(case, gsign, f"trsm_fp NBT={nbt} F={F}")
        if nbt == 2:
            _check_trsm_prods(case, gsign, f"trsm_prods NBT={nbt} F={F}")


# ----------------------------------------------------------------------
# diag_inv
# ----------------------------------------------------------------------
def _check_diag_inv(B, mp, pad):
    ext = _ext()
    m = mp - pad
    case = hpref.factor_case(m, P=1, D=B)
    L64 = np.stack([hpref.padded(case.Lref[0, d].astype(np.float64), mp)
                    for d in range(B)])
    invd = ext.diag_inv(_t(L64))
    assert invd.shape == (B, mp // 16, 16, 16)
    invd = _np(invd)
    for b in range(B):
        ref = hpref.diag_block_inverses(L64[b])
        base = hpref.block_inverses64(L64[b])
        for kb in range(mp // 16):
            _check(f"diag_inv B={B} mp={mp} b={b} kb={kb}", invd[b, kb],
                   ref[kb], base[kb])


@pytest.mark.parametrize("B,mp,pad", [(1, 16, 0), (3, 48, 7), (2, 144, 7),
                                      (1, 256, 0)])
def test_diag_inv_blocks(B, mp, pad):
    """(3, 48) is 9 blocks: a second workgroup with one live wave and
    seven that return early."""
    _check_diag_inv(B, mp, pad)


# ----------------------------------------------------------------------
# the chained op: factor (chol_batch / rocSOLVER + diag_inv) + solve
# ----------------------------------------------------------------------
_CHAIN = {}


def _chain_case(m, P, D=2, F=5):
    key = (m, P)
    if key in _CHAIN:
        return _CHAIN[key]
    from scipy.linalg import solve_triangular

    fc = hpref.factor_case(m, P=P, D=D, seed=5)
    mp = (m + 15) // 16 * 16
    rng = np.random.default_rng([5, m, P])
    RHS = np.stack([hpref.gen_rhs(rng, m, mp, F) for _ in range(P)])
    W = np.stack([np.stack([hpref.fsub(fc.Lref[p, d], RHS[p, :m])
                            for d in range(D)]) for p in range(P)])
    W64 = np.stack([np.stack([
        solve_triangular(fc.L64[p, d], RHS[p, :m], lower=True)
        for d in range(D)]) for p in range(P)])
    S, R = zip(*(hpref.gen_closure(hpref.gram(W[p, 0])) for p in range(P)))
    case = hpref.Case(m=np.full(P, m), mp=mp, F=F, P=P, D=D, RHS=RHS,
                      S=np.stack(S), R=np.stack(R), W=W, W64=W64,
                      TNT=fc.TNT, phiinv=fc.phiinv)
    _CHAIN[key] = case
    return case


@pytest.mark.parametrize("P", [1, 2], ids=["unbatched", "P=2"])
@pytest.mark.parametrize("m", [16, 128, 129, 241, 256])
def test_chol_trsm_fp_accum_chained(m, P):
    """ops.chol_trsm_fp_accum end to end against the oracle's own
    factor: m = 16 / 128 through chol_batch with no pad; 129 / 241 /
    256 through rocSOLVER + diag_inv + the right-looking solve (256:
    empty pad index, 241: the largest pad).  base: LAPACK on the CPU."""
    from fastfp_amd import ops

    case = _chain_case(m, P)
    sq = (lambda a: a[0]) if P == 1 else (lambda a: a)
    for gsign in (1.0, -1.0):
        pr, pb, fr, fb = hpref.solve_refs(case, gsign)
        fp = torch.zeros(sq(fr).shape, dtype=torch.float64, device=DEV)
        ops.chol_trsm_fp_accum(_t(sq(case.TNT)), _t(sq(case.phiinv)),
                               _t(sq(case.RHS)), _t(sq(case.S)),
                               _t(sq(case.R)), fp, gsign)
        got = _np(fp).reshape(fr.shape)
        for p in range(P):
            for d in range(case.D):
                _check(f"chained m={m} P={P} g={gsign:+.0f} p={p} d={d} fp",
                       got[p, d], fr[p, d], fb[p, d])


# ----------------------------------------------------------------------
# host side: empty launches return, unsupported sizes raise
# ----------------------------------------------------------------------
def _empty(*shape):
    return torch.empty(shape, dtype=torch.float64, device=DEV)


def test_empty_draws_or_frequencies_launch_nothing():
    """D = 0, F = 0 or B = 0: each op returns correctly shaped outputs
    without a launch, leaves no error behind, and the next valid call
    of the same op passes its oracle check."""
    ext = _ext()
    case = hpref.solve_case(2, 1, P=1, D=2)
    mp, nbt, D = case.mp, 2, case.D
    L, invd, RHS = _t(case.L), _t(case.invd), _t(case.RHS[0])
    S, R = _t(case.S[0]), _t(case.R[0])

    # chol_batch: no draws, unbatched and pulsar-batched
    fc = hpref.factor_case(17, P=2, D=3)
    L0, i0 = ext.chol_batch(_t(fc.TNT[0]), _empty(0, 17), 32)
    assert L0.shape == (0, 32, 32) and i0.shape == (0, 2, 16, 16)
    L0, i0 = ext.chol_batch(_t(fc.TNT), _empty(2, 0, 17), 32)
    assert L0.shape == (0, 32, 32) and i0.shape == (0, 2, 16, 16)
    torch.cuda.synchronize()
    _check_chol(2, True, "plain")

    # trsm_fp_accum / trsm_prods: no draws, then no frequencies
    fp = _empty(0, 1)
    ext.trsm_fp_accum(_empty(0, mp, mp), _empty(0, nbt, 16, 16), RHS, S, R,
                      fp, 1.0)
    out = _empty(0, 5, 1)
    ext.trsm_prods(_empty(0, mp, mp), _empty(0, nbt, 16, 16), RHS, S, R,
                   out, 1.0)
    keep = torch.full((D, 0), 7.0, dtype=torch.float64, device=DEV)
    ext.trsm_fp_accum(L, invd, _t(case.RHS[0][:, -1:]), _empty(3, 0),
                      _empty(2, 0), keep, 1.0)
    ext.trsm_prods(L, invd, _t(case.RHS[0][:, -1:]), _empty(3, 0),
                   _empty(2, 0), _empty(D, 5, 0), -1.0)
    torch.cuda.synchronize()
    _check_trsm_fp(case, 1.0, "after-empty trsm_fp")
    _check_trsm_prods(case, -1.0, "after-empty trsm_prods")

    # diag_inv: empty batch
    inv0 = ext.diag_inv(_empty(0, 32, 32))
    assert inv0.shape == (0, 2, 16, 16)
    torch.cuda.synchronize()
    _check_diag_inv(1, 16, 0)


def test_unsupported_solve_dimension_raises():
    """mp = 272 has no instantiation: the binding refuses it before any
    launch (nothing is submitted that is expected to be rejected)."""
    ext = _ext()
    mp, F = 272, 1
    args = (_empty(1, mp, mp), _empty(1, mp // 16, 16, 16),
            _empty(mp, 2 * F + 1), _empty(3, F), _empty(2, F))
    with pytest.raises(RuntimeError):
        ext.trsm_fp_accum(*args, _empty(1, F), 1.0)
    with pytest.raises(RuntimeError):
        ext.trsm_prods(*args, _empty(1, 5, F), 1.0)
    with pytest.raises(RuntimeError):
        ext.chol_batch(_empty(130, 130), _empty(1, 130), 144)
    torch.cuda.synchronize()
