"""CPU checks of the longdouble oracle (tests/hpref.py) and of the
input generators the kernel-level GPU tests share.

Two questions per oracle function: is it as precise as longdouble
allows (against mpmath at 40 digits on tiny inputs, within 8 longdouble
ulps of the plane maximum), and does it compute the right thing
(against the fp64 numpy/LAPACK/scipy evaluation, within 1e-13 normwise,
on the generators)?  A precise but wrong oracle fails the second."""

import mpmath
import numpy as np
import pytest
from scipy.linalg import solve_triangular

import hpref
from hpref import LD

mpmath.mp.dps = 40
ULP = float(np.finfo(LD).eps)


def test_longdouble_is_extended():
    assert np.finfo(LD).eps <= 2.0 ** -63
    # the constant really carries 64 bits: fp64 pi differs from it
    assert abs(mpmath.mpf(float(hpref.PI)) - mpmath.pi) > 1e-17
    assert abs(_mp(hpref.PI) - mpmath.pi) < 2.0 ** -62


# ----------------------------------------------------------------------
# mpmath helpers
# ----------------------------------------------------------------------
def _mp(x):
    """longdouble (or fp64) scalar -> mpf, exactly: a 64-bit
    significand splits into two doubles."""
    x = LD(x)
    hi = float(x)
    lo = float(x - LD(hi))
    return mpmath.mpf(hi) + mpmath.mpf(lo)


def _mpa(a):
    a = np.asarray(a)
    out = np.empty(a.shape, dtype=object)
    for idx in np.ndindex(a.shape):
        out[idx] = _mp(a[idx])
    return out


def _assert_ulps(got, want, what):
    """|got - want| <= 8 longdouble ulps of the plane maximum."""
    want = np.asarray(want, dtype=object)
    got = _mpa(got)
    assert got.shape == want.shape, what
    scale = max(abs(w) for w in want.flat)
    err = max(abs(g - w) for g, w in zip(got.flat, want.flat))
    print(f"{what}: {float(err / scale) / ULP:.2f} ulp")
    assert err <= 8 * ULP * scale, (what, float(err / scale) / ULP)


def _mp_chol(A):
    n = A.shape[0]
    L = np.full((n, n), mpmath.mpf(0), dtype=object)
    for j in range(n):
        for i in range(j, n):
            v = A[i, j] - sum((L[i, k] * L[j, k] for k in range(j)),
                              mpmath.mpf(0))
            L[i, j] = mpmath.sqrt(v) if i == j else v / L[j, j]
    return L


def _mp_fsub(L, B):
    n, k = B.shape
    X = np.empty((n, k), dtype=object)
    for c in range(k):
        for i in range(n):
            X[i, c] = (B[i, c] - sum((L[i, j] * X[j, c] for j in range(i)),
                                     mpmath.mpf(0))) / L[i, i]
    return X


def _mp_trig(toas, freqs):
    s = np.empty((len(freqs), len(toas)), dtype=object)
    c = np.empty_like(s)
    for i, f in enumerate(freqs):
        for k, t in enumerate(toas):
            arg = 2 * mpmath.pi * mpmath.mpf(float(f)) * mpmath.mpf(float(t))
            s[i, k], c[i, k] = mpmath.sin(arg), mpmath.cos(arg)
    return s, c


def _mp_gram(W):
    Ws, Wc, wu = W[:, 0:-1:2], W[:, 1:-1:2], W[:, -1]
    return np.stack([
        (Ws * Ws).sum(0), (Wc * Wc).sum(0), (Ws * Wc).sum(0),
        (Ws * wu[:, None]).sum(0), (Wc * wu[:, None]).sum(0),
    ])


# ----------------------------------------------------------------------
# oracle vs mpmath, tiny inputs: m = 6, ntoa = 8, F = 2, three blocks
# ----------------------------------------------------------------------
@pytest.fixture(scope="module")
def tiny():
    rng = np.random.default_rng(2024)
    m, F = 6, 2
    TNT, phiinv = hpref.gen_sigma(rng, m, 1, "range")
    Sig = hpref.sigma_of(TNT, phiinv[0])
    RHS = hpref.gen_rhs(rng, m, m, F)
    return m, F, Sig, RHS


def test_chol_fsub_vs_mpmath(tiny):
    m, F, Sig, RHS = tiny
    L = hpref.chol(Sig)
    Lmp = _mp_chol(_mpa(Sig))
    _assert_ulps(L, Lmp, "chol")
    assert (np.triu(L, 1) == 0).all()
    # substitution with the SAME (fp64-rounded) factor on both sides
    L64 = L.astype(np.float64)
    W = hpref.fsub(L64, RHS)
    _assert_ulps(W, _mp_fsub(_mpa(L64), _mpa(RHS)), "fsub")
    w1 = hpref.fsub(L64, RHS[:, 0])
    assert w1.shape == (m,) and (w1 == W[:, 0]).all()


def test_padded_and_block_inverses_vs_mpmath(tiny):
    m, F, Sig, RHS = tiny
    P = hpref.padded(Sig, 16)
    assert P.shape == (16, 16) and (P[:m, :m] == Sig).all()
    assert (P[m:, m:] == np.eye(16 - m)).all()
    assert (P[m:, :m] == 0).all() and (P[:m, m:] == 0).all()
    L64 = hpref.padded(hpref.chol(Sig).astype(np.float64), 32)
    inv = hpref.diag_block_inverses(L64)
    assert inv.shape == (2, 16, 16)
    eye = _mpa(np.eye(16))
    for kb in range(2):
        blk = _mpa(L64[kb * 16:kb * 16 + 16, kb * 16:kb * 16 + 16])
        _assert_ulps(inv[kb], _mp_fsub(blk, eye), f"diag_block_inverses[{kb}]")
    assert (inv[1] == np.eye(16)).all()  # all-pad block


@pytest.mark.parametrize("gsign", [1.0, -1.0])
def test_products_fp_vs_mpmath(tiny, gsign):
    m, F, Sig, RHS = tiny
    W = hpref.fsub(hpref.chol(Sig).astype(np.float64), RHS)
    S, R = hpref.gen_closure(hpref.gram(W))
    Wmp = _mpa(W)  # the oracle's W taken as exact input
    g = _mp_gram(Wmp)
    _assert_ulps(hpref.gram(W), g, "gram")
    Smp, Rmp = _mpa(S), _mpa(R)
    gs = mpmath.mpf(gsign)
    want = np.stack([Smp[0] - gs * g[0], Smp[1] - gs * g[1],
                     Smp[2] - gs * g[2], Rmp[0] - gs * g[3],
                     Rmp[1] - gs * g[4]])
    prods = hpref.products(W, S, R, gsign)
    for i in range(5):
        _assert_ulps(prods[i], want[i], f"products[{i}]")
    M11, M22, M12, N1, N2 = _mpa(prods)
    fp = (N1 * N1 * M22 - 2 * N1 * N2 * M12 + N2 * N2 * M11) \
        / (M11 * M22 - M12 * M12) / 2
    _assert_ulps(hpref.fp_from_products(prods), fp, "fp_from_products")


def test_trig_kernels_vs_mpmath():
    rng = np.random.default_rng(7)
    ntoa, F, m = 8, 2, 6
    # the offset case: |2 pi f t| ~ 1.5e3 must not cost the oracle
    toas, ninv, nr, freqs = hpref.gen_trig(rng, ntoa, F, offset=4.6e9)
    s, c = _mp_trig(toas, freqs)
    nv, nrv = _mpa(ninv), _mpa(nr)
    sNs, sNr = hpref.trig_dots(toas, ninv, nr, freqs)
    want = [(s * s * nv).sum(1), (c * c * nv).sum(1), (s * c * nv).sum(1)]
    for i in range(3):
        _assert_ulps(sNs[i], want[i], f"trig_dots sNs[{i}]")
    _assert_ulps(sNr[0], (s * nrv).sum(1), "trig_dots sNr[0]")
    _assert_ulps(sNr[1], (c * nrv).sum(1), "trig_dots sNr[1]")

    T = rng.normal(size=(ntoa, m))
    B = hpref.basis_rhs(T, ninv, toas, freqs)
    Tw = _mpa(T).T
    wantB = np.empty((m, 2 * F), dtype=object)
    wantB[:, 0::2] = Tw.dot((s * nv).T)
    wantB[:, 1::2] = Tw.dot((c * nv).T)
    _assert_ulps(B[:, 0::2], wantB[:, 0::2], "basis_rhs sin")
    _assert_ulps(B[:, 1::2], wantB[:, 1::2], "basis_rhs cos")

    # three blocks: a singleton (beta 0) and two real ones
    uvec, beta, offsets, sizes = hpref.gen_blocks(rng, [1, 3, 4])
    assert beta[0] == 0.0 and (beta[1:] > 0).all()
    bs, br = hpref.block_dots(toas, uvec, nr, freqs, beta, offsets, sizes)
    u, bt = _mpa(uvec), _mpa(beta)
    wantS = np.full((3, F), mpmath.mpf(0), dtype=object)
    for b, (o, sz) in enumerate(zip(offsets, sizes)):
        sl = slice(int(o), int(o + sz))
        for f in range(F):
            us, uc = (u[sl] * s[f, sl]).sum(), (u[sl] * c[f, sl]).sum()
            wantS[0, f] += (u[sl] * s[f, sl] ** 2).sum() - bt[b] * us * us
            wantS[1, f] += (u[sl] * c[f, sl] ** 2).sum() - bt[b] * uc * uc
            wantS[2, f] += (u[sl] * s[f, sl] * c[f, sl]).sum() \
                - bt[b] * us * uc
    for i in range(3):
        _assert_ulps(bs[i], wantS[i], f"block_dots sNs[{i}]")
    _assert_ulps(br[0], (s * nrv).sum(1), "block_dots sNr[0]")
    _assert_ulps(br[1], (c * nrv).sum(1), "block_dots sNr[1]")


# ----------------------------------------------------------------------
# oracle vs plain fp64 on the generators: precise AND right
# ----------------------------------------------------------------------
AGREE = 1e-13


@pytest.mark.parametrize("flavour", ["plain", "range"])
@pytest.mark.parametrize("m", [1, 9, 37, 113, 256])
def test_factor_and_solve_agree_with_lapack(m, flavour):
    case = hpref.factor_case(m, P=1, D=2, flavour=flavour)
    mp = (m + 15) // 16 * 16
    rng = np.random.default_rng(m)
    RHS = hpref.gen_rhs(rng, m, mp, 3)
    assert (RHS[m:] == 0).all() and RHS.shape == (mp, 7)
    for d in range(2):
        Lref, L64 = case.Lref[0, d], case.L64[0, d]
        assert hpref.nerr(L64, Lref) < AGREE
        Lp = hpref.padded(Lref.astype(np.float64), mp)
        W = hpref.fsub(Lp, RHS)
        W64 = solve_triangular(Lp, RHS, lower=True)
        assert hpref.nerr(W64, W) < AGREE
        assert (W[m:] == 0).all()  # zero pad rows stay zero
        inv = hpref.diag_block_inverses(Lp)
        inv64 = hpref.block_inverses64(Lp)
        for kb in range(mp // 16):
            assert hpref.nerr(inv64[kb], inv[kb]) < AGREE
        # L L^T = Sigma, checked in longdouble
        Sig = hpref.sigma_of(case.TNT[0], case.phiinv[0, d])
        assert hpref.nerr(Lref @ Lref.T, Sig) < 1e-17


def test_trig_kernels_agree_with_fp64():
    rng = np.random.default_rng(3)
    toas, ninv, nr, freqs = hpref.gen_trig(rng, 257, 5)
    ref = hpref.trig_dots(toas, ninv, nr, freqs)
    f64 = hpref.trig_dots(toas, ninv, nr, freqs, np.float64)
    # an independent spelling of the same dots
    arg = 2 * np.pi * freqs[:, None] * toas[None, :]
    s, c = np.sin(arg), np.cos(arg)
    alt = (np.stack([(s * s) @ ninv, (c * c) @ ninv, (s * c) @ ninv]),
           np.stack([s @ nr, c @ nr]))
    for i in range(3):
        assert hpref.nerr(f64[0][i], ref[0][i]) < AGREE
        assert hpref.nerr(alt[0][i], ref[0][i]) < AGREE
    for i in range(2):
        assert hpref.nerr(f64[1][i], ref[1][i]) < AGREE
        assert hpref.nerr(alt[1][i], ref[1][i]) < AGREE

    T = rng.normal(size=(257, 65))
    B = hpref.basis_rhs(T, ninv, toas, freqs)
    assert hpref.nerr((T.T * ninv) @ s.T, B[:, 0::2]) < AGREE
    assert hpref.nerr((T.T * ninv) @ c.T, B[:, 1::2]) < AGREE
    assert hpref.nerr(hpref.basis_rhs(T, ninv, toas, freqs, np.float64),
                      B) < AGREE

    sizes = [1, 1, 2, 40, 100] + [1, 2, 3] * 10
    uvec, beta, offsets, sizes = hpref.gen_blocks(rng, sizes)
    n = int(sizes.sum())
    toas, _, nr, freqs = hpref.gen_trig(rng, n, 3)
    bs, br = hpref.block_dots(toas, uvec, nr, freqs, beta, offsets, sizes)
    # Sherman-Morrison inverse of the block it claims to invert:
    # N_b = diag(1/u) + e2 J, beta = e2 / (1 + e2 sum u)
    o, sz = int(offsets[3]), int(sizes[3])
    ub = uvec[o:o + sz]
    e2 = beta[3] / (1 - beta[3] * ub.sum())
    Nb = np.diag(1 / ub) + e2
    Ninv = np.diag(ub) - beta[3] * np.outer(ub, ub)
    assert np.abs(Nb @ Ninv - np.eye(sz)).max() < 1e-10
    # and the rank-1 spelling the kernel uses, in fp64
    arg = 2 * np.pi * freqs[:, None] * toas[None, :]
    s, c = np.sin(arg), np.cos(arg)
    want = np.stack([(s * s) @ uvec, (c * c) @ uvec, (s * c) @ uvec])
    for b, (o, sz) in enumerate(zip(offsets, sizes)):
        us = s[:, o:o + sz] @ uvec[o:o + sz]
        uc = c[:, o:o + sz] @ uvec[o:o + sz]
        want -= beta[b] * np.stack([us * us, uc * uc, us * uc])
    for i in range(3):
        assert hpref.nerr(want[i], bs[i]) < AGREE
    assert hpref.nerr(s @ nr, br[0]) < AGREE
    assert hpref.nerr(c @ nr, br[1]) < AGREE


# ----------------------------------------------------------------------
# the generators keep their promises, so no GPU case is ever excluded
# ----------------------------------------------------------------------
@pytest.mark.parametrize("flavour", ["plain", "range"])
def test_sigma_conditioning_below_1e4(flavour):
    """cond(Sigma) < 1e4 at every m the GPU tests factor: mp and
    mp - 15 for NBT 1..16, and the chained op's sizes."""
    ms = sorted({16 * k for k in range(1, 17)}
                | {16 * k - 15 for k in range(1, 17)} | {129, 241})
    worst = 0.0
    for m in ms:
        rng = np.random.default_rng([11, m])
        TNT, phiinv = hpref.gen_sigma(rng, m, 2, flavour)
        assert (TNT == TNT.T).all()
        for d in range(2):
            cond = np.linalg.cond(hpref.sigma_of(TNT, phiinv[d]))
            worst = max(worst, cond)
            assert cond < 1e4, (m, flavour, cond)
    print(f"{flavour}: worst cond {worst:.3g}")


@pytest.mark.parametrize("nbt", range(1, 17))
def test_closure_has_no_cancellation(nbt):
    """det(M) >= 3 a1 b1 for every (pulsar, draw, frequency) of the
    solve cases the GPU tests use; the fp64 baseline of those cases
    agrees with the oracle."""
    case = hpref.solve_case(nbt, 64)
    assert case.L.shape == (4, 16 * nbt, 16 * nbt)
    assert list(case.m) == [16 * nbt, 16 * nbt - 5]
    assert (case.RHS[1, case.m[1]:] == 0).all()
    for gsign in (1.0, -1.0):
        pr, pb, fr, fb = hpref.solve_refs(case, gsign)
        det = pr[:, :, 0] * pr[:, :, 1] - pr[:, :, 2] ** 2
        assert (det >= 3 * case.g[:, :, 0] * case.g[:, :, 1]).all()
        assert (pr[:, :, :2] > 0).all()
        assert hpref.nerr(fb, fr) < AGREE
        for i in range(5):
            assert hpref.nerr(pb[:, :, i], pr[:, :, i]) < AGREE
    # identity padding of the given factor and its block inverses
    m1, mp = case.m[1], case.mp
    assert (case.L[2:, m1:, m1:] == np.eye(mp - m1)).all()
    assert (case.L[2:, m1:, :m1] == 0).all()


# ----------------------------------------------------------------------
# the Fe oracle: fe_points / fe_null_data vs mpmath, the host fp64 paths
# vs the oracle (the ``base`` of tests/test_fe_oracle.py), the classes of
# the conditioning ladder
# ----------------------------------------------------------------------
def _mp_fe_point(prods, ant_row, d, f):
    """(fe, a (4,), ratio (4,), cond) of one point in mpmath, by a route
    of its own: M and N summed entry by entry, a from an LU solve,
    fe = 1/2 N.a, the pivots as the squared Cholesky diagonal."""
    P = prods.shape[0]
    G = [[mpmath.mpf(float(prods[p, d, 0, f])),
          mpmath.mpf(float(prods[p, d, 2, f])),
          mpmath.mpf(float(prods[p, d, 1, f]))] for p in range(P)]
    M = mpmath.zeros(4, 4)
    N = mpmath.zeros(4, 1)
    for p in range(P):
        ss, sc, cc = G[p]
        blk = [[ss, sc], [sc, cc]]
        co = [mpmath.mpf(float(ant_row[p, 0])),
              mpmath.mpf(float(ant_row[p, 1]))]
        dat = [mpmath.mpf(float(prods[p, d, 3, f])),
               mpmath.mpf(float(prods[p, d, 4, f]))]
        for i in range(4):
            N[i] += co[i // 2] * dat[i % 2]
            for j in range(4):
                M[i, j] += co[i // 2] * co[j // 2] * blk[i % 2][j % 2]
    a = mpmath.lu_solve(M, N)
    fe = sum(N[i] * a[i] for i in range(4)) / 2
    L = mpmath.cholesky(M)
    ratio = [L[j, j] ** 2 / M[j, j] for j in range(4)]
    M64 = np.array([[float(M[i, j]) for j in range(4)] for i in range(4)])
    return fe, [a[i] for i in range(4)], ratio, float(np.linalg.cond(M64))


@pytest.mark.parametrize("P", [3, 5])
def test_fe_points_vs_mpmath(P):
    """Random table (rows 18, 19) and the 1e-3 rung (rows 8, 9) of the
    ladder case.  The 8-ulp rule of ``_assert_ulps`` is relative to a
    well-conditioned plane; here it is scaled by cond(M) of the point,
    computed from the mpmath M."""
    case = hpref.fe_ladder_case(P)
    for sky in (18, 19, 8, 9):
        for d, f in ((0, 0), (1, 8)):
            fe, a, ratio, cond = _mp_fe_point(case.prods, case.ant[sky], d, f)
            lim = 8 * ULP * cond
            e_fe = abs(_mp(case.fe[d, sky, f]) - fe) / abs(fe)
            amax = max(abs(x) for x in a)
            e_a = max(abs(_mp(g) - w) for g, w in
                      zip(case.amps[d, sky, f], a)) / amax
            e_r = max(abs(_mp(g) - w) for g, w in
                      zip(case.ratio[d, sky, f], ratio))
            print(f"P={P} sky={sky} ({d},{f}): cond {cond:.2e} fe "
                  f"{float(e_fe) / ULP:.1f} amps {float(e_a) / ULP:.1f} "
                  f"ratio {float(e_r) / ULP:.1f} ulp")
            assert e_fe <= lim and e_a <= lim and e_r <= lim


def test_fe_sums_layout():
    """The ten M entries are those of ``festat._moments`` and the four N
    sums those of ``_assemble_fe_draws``, in their order."""
    from fastfp_amd.festat import _moments, _psum

    case = hpref.fe_case(5, 3, 5, 17)
    M, N = hpref.fe_sums(case.prods, case.ant)
    assert M.shape == (3, 17, 5, 10) and N.shape == (3, 17, 5, 4)
    assert M.dtype == LD and N.dtype == LD
    for k in (0, 16):
        fplus, fcross = case.ant[k, :, 0], case.ant[k, :, 1]
        for i, m in enumerate(_moments(case.prods, fplus, fcross)):
            assert hpref.nerr(m, M[:, k, :, i]) < AGREE
        sr, cr = case.prods[:, :, 3], case.prods[:, :, 4]
        for i, n in enumerate([_psum(fplus, sr), _psum(fplus, cr),
                               _psum(fcross, sr), _psum(fcross, cr)]):
            assert hpref.nerr(n, N[:, k, :, i]) < AGREE


def test_fe_null_data_vs_mpmath():
    rng = np.random.default_rng(41)
    P, D, F, mp, R = 2, 2, 2, 16, 3
    white, rhs, X = hpref.gen_null_data(rng, P, D, F, 11, mp, R, wide=True)
    got = hpref.fe_null_data(white, rhs, X)
    assert got.shape == (D, F, P, 2, R) and got.dtype == LD
    want = np.empty(got.shape, dtype=object)
    for d, f, p, c, r in np.ndindex(got.shape):
        acc = mpmath.mpf(float(white[p, r, 2 * f + c]))
        for k in range(mp):
            acc -= (mpmath.mpf(float(rhs[p, k, 2 * f + c]))
                    * mpmath.mpf(float(X[p, d, k, r])))
        want[d, f, p, c, r] = acc
    _assert_ulps(got, want, "fe_null_data")
    # and the fp64 einsum the GPU test takes its base from
    e64, mag = hpref.null_data64(white, rhs, X)
    assert hpref.nerr(e64, got) < AGREE
    assert (np.abs(got) <= mag).all()


def test_fe_null_products_and_map():
    """n = L z against ``festat._null_draws``; the null map with the data
    planes themselves as n is the Fe map."""
    from fastfp_amd.festat import _null_draws

    case, refs = hpref.fe_null_case(5, 3, 5, 65, 17)
    n = hpref.fe_null_products(case.prods, refs.z)
    ns, nc = _null_draws(case.prods, refs.z)  # (P, D, F, R)
    assert hpref.nerr(np.moveaxis(ns, 0, 2), n[:, :, :, 0]) < AGREE
    assert hpref.nerr(np.moveaxis(nc, 0, 2), n[:, :, :, 1]) < AGREE
    assert refs.map_z.shape == (17, 3, 65, 5)
    data = case.prods[:, :, 3:].transpose(1, 3, 0, 2)[..., None]
    assert data.shape == (3, 5, 5, 2, 1)  # (D, F, P, 2, R = 1)
    fmap = hpref.fe_null_map(case.prods, case.ant, data)
    assert hpref.nerr(fmap[0], case.fe) < 8 * ULP


@pytest.mark.parametrize("P", hpref.LADDER_P)
def test_fe_host_base_per_rung(P):
    """The errors of the host fp64 paths against the oracle, one plane
    per rung: the ``base`` of the device tolerances.  Only finiteness is
    asserted, and 64 eps on the untouched rows (for P >= 3: the
    untouched rows of P = 2 reach cond(M) ~ 1e3 and are no
    well-conditioned rung)."""
    case = hpref.fe_ladder_case(P)
    for dl, rows in case.rungs.items():
        b_fe = hpref.nerr(case.fe64[:, rows], case.fe[:, rows])
        b_a = hpref.amp_err(case.amps64[:, rows], case.amps[:, rows])
        print(f"P={P} delta={dl}: host fe {b_fe:.3e} amps {b_a:.3e}")
        assert np.isfinite(b_fe) and np.isfinite(b_a)
        if dl is None and P >= 3:
            assert b_fe < 64 * hpref.EPS64 and b_a < 64 * hpref.EPS64
    refs = hpref.fe_ladder_null(P)
    for m in ("z", "n"):
        b = hpref.nerr(getattr(refs, "host_" + m), getattr(refs, "max_" + m))
        print(f"P={P} null maxima over the kept rows, mode {m}: host {b:.3e}")
        assert np.isfinite(b)


def test_fe_host_base_well_conditioned():
    worst = 0.0
    for shape in hpref.FE_SHAPES[:-1] + hpref.FE_AMP_SHAPES:
        case = hpref.fe_case(*shape)
        b_fe = hpref.nerr(case.fe64, case.fe)
        b_a = hpref.amp_err(case.amps64, case.amps)
        print(f"{shape}: host fe {b_fe:.3e} amps {b_a:.3e} smallest pivot "
              f"ratio {float(case.ratio.min()):.2e}")
        assert np.isfinite(b_fe) and np.isfinite(b_a)
        assert case.ratio.min() >= hpref.LADDER_KEEP_MIN
        if shape[0] >= 3:
            worst = max(worst, b_fe)
    assert worst < 64 * hpref.EPS64
    for shape in hpref.FE_NULL_SHAPES[:3]:
        case, refs = hpref.fe_null_case(*shape)
        assert case.ratio.min() >= hpref.LADDER_KEEP_MIN
        for m in ("z", "n"):
            b = hpref.nerr(getattr(refs, "host_" + m),
                           getattr(refs, "max_" + m))
            print(f"{shape} null mode {m}: host {b:.3e}")
            assert np.isfinite(b)
            if shape[0] >= 3:
                assert b < 64 * hpref.EPS64
    # the fp64 einsum of the null data
    rng = np.random.default_rng(43)
    white, rhs, X = hpref.gen_null_data(rng, 2, 2, 33, 43, 48, 65, wide=True)
    e64, _ = hpref.null_data64(white, rhs, X)
    b = hpref.nerr(e64, hpref.fe_null_data(white, rhs, X))
    print(f"null data, fp64 einsum: {b:.3e}")
    assert b < 64 * hpref.EPS64


@pytest.mark.parametrize("P", hpref.LADDER_P)
def test_fe_ladder_classes(P):
    """Every kept point has all four oracle pivot ratios >= 1e-10, every
    point of rows 16, 17 a smallest ratio < 1e-14, and nothing lies
    between: the kernels' 1e-12 rule is two decades from either class,
    so a device point may never be on the other side of it."""
    case = hpref.fe_ladder_case(P)
    assert sorted(list(case.keep) + list(case.skip)) == list(range(20))
    smallest = case.ratio.min(axis=-1)  # (D, nsky, F)
    assert np.isfinite(case.ratio.astype(np.float64)).all()
    for dl, rows in case.rungs.items():
        print(f"P={P} delta={dl}: smallest ratio "
              f"{float(smallest[:, rows].min()):.2e}")
    print(f"P={P} skipped rows: largest smallest ratio "
          f"{float(smallest[:, case.skip].max()):.2e}")
    assert (smallest[:, case.keep] >= hpref.LADDER_KEEP_MIN).all()
    assert (smallest[:, case.skip] < hpref.LADDER_SKIP_MAX).all()
    between = (smallest < hpref.LADDER_KEEP_MIN) \
        & (smallest >= hpref.LADDER_SKIP_MAX)
    assert not between.any()


def test_fe_tie_case_margin():
    """The five equal rows of the tie case are the largest of every
    column of the oracle's map, by 5 % at least: eleven orders above the
    device tolerance (16 * 64 eps), so no rounding decides between a tie
    row and another row.

    A factor of 4 is out of reach on a random antenna table: a signal
    from row 70 lies in span(F+, Fx)_70 (x) R^2 of the 2 P = 18 data
    dimensions, another row recovers on average the share 2 / P = 0.22
    of it, and the largest share among 125 random rows is near 0.9
    whatever amplitudes the signal has."""
    prods, ant, ant2 = hpref.fe_tie_case()
    fe, _, ratio = hpref.fe_points(prods, ant)
    assert ratio.min() >= hpref.LADDER_KEEP_MIN
    ties = list(hpref.TIE_ROWS)
    for r in ties:
        assert (fe[:, r] == fe[:, 70]).all()
    others = np.setdiff1d(np.arange(130), ties)
    margin = (fe[:, 70][:, None] / fe[:, others]).min()
    print(f"tie rows over the best other row: factor {float(margin):.3f}")
    assert margin > 1.05
    assert (fe.argmax(axis=1) == 3).all()
    fe2, _, _ = hpref.fe_points(prods, ant2)
    margin2 = (fe2[:, 70] / fe2[:, 3]).min()
    print(f"tie rows over the replaced row 3: factor {float(margin2):.3f}")
    assert margin2 > 1.05
    assert (fe2.argmax(axis=1) == 19).all()
