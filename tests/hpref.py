"""Extended-precision oracle for the solve, precompute and Fe kernels.

Plain numpy in ``np.longdouble`` (x87 80-bit, 64-bit significand):
every kernel-level GPU test compares a HIP kernel with these functions
and sizes its tolerance from the error a plain CPU fp64 evaluation of
the same operation makes against them (``tol_from_base``), so the bound
is measured for the inputs at hand rather than chosen.

All functions take fp64 arrays, treat them as exact, and return
longdouble.  Tiny systems only: the factor and the substitution are
O(m^3) / O(m^2 n) interpreted loops over longdouble vector operations.

The second half of the module holds the input generators the GPU tests
share (``gen_sigma``, ``gen_rhs``, ``gen_closure``, ``gen_trig``,
``gen_blocks``, ``gen_fe_case``) and the cached cases built from them;
``tests/test_hpref.py`` checks both halves on the CPU.
"""

import numpy as np

LD = np.longdouble
EPS64 = float(np.finfo(np.float64).eps)

# fail loudly, never skip: a platform whose long double is fp64 would
# turn every comparison below into fp64-vs-fp64
assert np.finfo(LD).eps <= 2.0 ** -63, (
    "tests/hpref.py needs an extended-precision np.longdouble "
    f"(eps <= 2**-63); this platform has eps = {np.finfo(LD).eps}"
)

PI = LD("3.14159265358979323846264338327950288")


def _ld(a):
    """fp64 input -> longdouble, exactly."""
    return np.asarray(a, dtype=np.float64).astype(LD)


# ----------------------------------------------------------------------
# dense linear algebra
# ----------------------------------------------------------------------
def chol(A):
    """Column Cholesky of a symmetric positive definite (n, n) matrix;
    only the lower triangle of ``A`` is read."""
    A = _ld(A)
    n = A.shape[0]
    L = np.zeros((n, n), dtype=LD)
    for j in range(n):
        v = A[j:, j] - L[j:, :j] @ L[j, :j]
        assert v[0] > 0, f"chol: pivot {j} not positive"
        d = np.sqrt(v[0])
        L[j, j] = d
        L[j + 1:, j] = v[1:] / d
    return L


def fsub(L, B):
    """Forward substitution X = L^-1 B, L lower triangular (n, n),
    B (n,) or (n, k).  ``L`` / ``B`` may already be longdouble."""
    L = np.asarray(L, dtype=LD)
    B = np.asarray(B, dtype=LD)
    vec = B.ndim == 1
    X = np.array(B.reshape(B.shape[0], -1), dtype=LD)
    for i in range(L.shape[0]):
        X[i] = (X[i] - L[i, :i] @ X[:i]) / L[i, i]
    return X[:, 0] if vec else X


def diag_block_inverses(L):
    """Inverse of each 16x16 diagonal block of lower-triangular L
    (mp, mp), by substitution -> (mp/16, 16, 16)."""
    L = np.asarray(L, dtype=LD)
    mp = L.shape[0]
    assert mp % 16 == 0 and L.shape == (mp, mp)
    eye = np.eye(16, dtype=LD)
    return np.stack([
        fsub(np.tril(L[k:k + 16, k:k + 16]), eye) for k in range(0, mp, 16)
    ])


def padded(Sigma, mp):
    """Sigma (m, m) identity-padded to (mp, mp) — the kernels'
    convention: pad rows/columns of Sigma are the identity, so L's pad
    block is the identity and zero RHS pad rows stay zero."""
    Sigma = np.asarray(Sigma)
    m = Sigma.shape[0]
    assert mp >= m
    out = np.eye(mp, dtype=Sigma.dtype)
    out[:m, :m] = Sigma
    return out


# ----------------------------------------------------------------------
# the fused 2x2 closure of the solve
# ----------------------------------------------------------------------
def gram(W, dtype=LD):
    """The five raw dots of the solved columns W (rows, 2F+1) laid out
    as the kernel's ``[s0 c0 s1 c1 ... | u]`` ->
    (5, F) = [Ws.Ws, Wc.Wc, Ws.Wc, Ws.wu, Wc.wu].

    ``dtype=np.float64`` here and below evaluates the same formula in
    plain fp64: the CPU baseline whose error sizes the tolerance."""
    W = np.asarray(W, dtype=dtype)
    assert W.shape[1] % 2 == 1
    Ws, Wc, wu = W[:, 0:-1:2], W[:, 1:-1:2], W[:, -1]
    return np.stack([
        (Ws * Ws).sum(0), (Wc * Wc).sum(0), (Ws * Wc).sum(0),
        (Ws * wu[:, None]).sum(0), (Wc * wu[:, None]).sum(0),
    ])


def products(W, S, R, gsign, dtype=LD):
    """The five corrected planes [M11, M22, M12, N1, N2] (5, F):
    M = S - gsign * W.W, N = R - gsign * W.wu, with S (3, F) =
    [ss, cc, sc] and R (2, F) = [sr, cr]."""
    g = gram(W, dtype)
    S, R = _ld(S).astype(dtype), _ld(R).astype(dtype)
    gs = dtype(gsign)
    return np.stack([
        S[0] - gs * g[0], S[1] - gs * g[1], S[2] - gs * g[2],
        R[0] - gs * g[3], R[1] - gs * g[4],
    ])


def fp_from_products(prods, dtype=LD):
    """Fp (..., F) = 0.5 N^T M^-1 N from the planes (..., 5, F)."""
    p = np.asarray(prods, dtype=dtype)
    M11, M22, M12, N1, N2 = (p[..., i, :] for i in range(5))
    det = M11 * M22 - M12 * M12
    num = N1 * N1 * M22 - 2 * N1 * N2 * M12 + N2 * N2 * M11
    return num / det / 2


# ----------------------------------------------------------------------
# the precompute kernels
# ----------------------------------------------------------------------
def _trig(toas, freqs, dtype=LD):
    """sin, cos of 2 pi f t, (F, ntoa); the argument is formed in
    longdouble from the fp64 inputs.  In fp64 it is rounded as the
    kernels round it, fl(fl(2 pi f) t), so a large |2 pi f t| costs the
    baseline what it costs them.

    The longdouble argument is reduced before it is rounded: f and t
    are split into 26/27-bit halves, whose four partial products are
    exact in a 64-bit significand, and whole cycles are dropped from
    each, so the phase error stays at a few 1e-19 of a cycle however
    large |f t| is (a rounded 2 pi f t at 1.5e3 rad is already off by
    1.6e-16 rad)."""
    if dtype is not LD:
        w = dtype(2) * dtype(PI) * _ld(freqs).astype(dtype)
        arg = w[:, None] * _ld(toas).astype(dtype)[None, :]
        return np.sin(arg), np.cos(arg)

    def split(x):  # Veltkamp, exact in fp64
        x = np.asarray(x, dtype=np.float64)
        c = 134217729.0 * x  # 2**27 + 1
        hi = c - (c - x)
        return hi.astype(LD), (x - hi).astype(LD)

    fh, fl = split(freqs)
    th, tl = split(toas)
    cyc = np.zeros((fh.size, th.size), dtype=LD)
    for a in (fh, fl):
        for b in (th, tl):
            p = a[:, None] * b[None, :]  # exact
            cyc += p - np.rint(p)
    cyc -= np.rint(cyc)
    arg = 2 * PI * cyc
    return np.sin(arg), np.cos(arg)


def trig_dots(toas, ninv, nr, freqs, dtype=LD):
    """sigdots: sNs (3, F) = [s.Ns, c.Nc, s.Nc] with diagonal weights
    ``ninv``, sNr (2, F) = [s.nr, c.nr]."""
    s, c = _trig(toas, freqs, dtype)
    ninv, nr = _ld(ninv).astype(dtype), _ld(nr).astype(dtype)
    sNs = np.stack([(s * s * ninv).sum(1), (c * c * ninv).sum(1),
                    (s * c * ninv).sum(1)])
    sNr = np.stack([(s * nr).sum(1), (c * nr).sum(1)])
    return sNs, sNr


def basis_rhs(T, weights, toas, freqs, dtype=LD):
    """sbgemm: out[j, 2f] = sum_k T[k, j] w[k] sin(2 pi f t_k), the
    cosine in column 2f + 1 -> (m, 2F)."""
    s, c = _trig(toas, freqs, dtype)
    # weight the trig panel, as the kernel does, not T
    w = _ld(weights).astype(dtype)
    s, c = s * w, c * w
    Tw = _ld(T).astype(dtype).T  # (m, ntoa)
    out = np.empty((Tw.shape[0], 2 * s.shape[0]), dtype=dtype)
    out[:, 0::2] = Tw @ s.T
    out[:, 1::2] = Tw @ c.T
    return out


def block_dots(toas, uvec, nr, freqs, beta, offsets, sizes, dtype=LD):
    """sigdots_block: the five dots with block-diagonal N whose block
    inverses are written out densely as diag(u) - beta u u^T.  The
    blocks must tile [0, ntoa) in order."""
    s, c = _trig(toas, freqs, dtype)
    u, nr, beta = (_ld(x).astype(dtype) for x in (uvec, nr, beta))
    F = s.shape[0]
    sNs = np.zeros((3, F), dtype=dtype)
    end = 0
    for b, (o, sz) in enumerate(zip(offsets, sizes)):
        o, sz = int(o), int(sz)
        assert o == end, "blocks must be contiguous and ordered"
        end = o + sz
        ub = u[o:end]
        Ninv = np.diag(ub) - beta[b] * np.outer(ub, ub)
        sb, cb = s[:, o:end], c[:, o:end]
        sNs[0] += ((sb @ Ninv) * sb).sum(1)
        sNs[1] += ((cb @ Ninv) * cb).sum(1)
        sNs[2] += ((sb @ Ninv) * cb).sum(1)
    assert end == len(u), "blocks must cover every TOA"
    sNr = np.stack([(s * nr).sum(1), (c * nr).sum(1)])
    return sNs, sNr


# ----------------------------------------------------------------------
# the Fe sky kernels (fe_kernels.hip)
# ----------------------------------------------------------------------
def fe_sums(prods, ant):
    """The sums over pulsars of one Fe point: M (D, nsky, F, 10), the ten
    unique entries (m00, m01, m02, m03, m11, m12, m13, m22, m23, m33) of
    the symmetric 4x4 M over the filters F+ sin, F+ cos, Fx sin, Fx cos,
    and N (D, nsky, F, 4).  ``prods`` (P, D, 5, F) = [ss, cc, sc, sr, cr],
    ``ant`` (nsky, P, 2) = [F+, Fx]; the coefficient products F+^2, F+ Fx,
    Fx^2 are formed in longdouble too."""
    prods, ant = _ld(prods), _ld(ant)
    P, D, _, F = prods.shape
    fp, fx = ant[:, :, 0], ant[:, :, 1]  # (nsky, P)
    ss, cc, sc, sr, cr = (prods[:, :, i].reshape(P, D * F) for i in range(5))

    def psum(coeff, q):  # (nsky, P) x (P, D F) -> (D, nsky, F)
        return np.moveaxis((coeff @ q).reshape(-1, D, F), 0, 1)

    p2, px, x2 = fp * fp, fp * fx, fx * fx
    pxsc = psum(px, sc)
    M = np.stack([psum(p2, ss), psum(p2, sc), psum(px, ss), pxsc,
                  psum(p2, cc), pxsc, psum(px, cc),
                  psum(x2, ss), psum(x2, sc), psum(x2, cc)], axis=-1)
    N = np.stack([psum(fp, sr), psum(fp, cr), psum(fx, sr), psum(fx, cr)],
                 axis=-1)
    return M, N


def _fe_ldl(M):
    """Unpivoted LDL^T of the 4x4 matrices M (..., 10): the six unit-lower
    entries (l10, l20, l30, l21, l31, l32) and the pivots d (..., 4).
    Nothing is rejected: a zero or negative pivot gives what the
    arithmetic gives (inf / nan / a negative d)."""
    m00, m01, m02, m03, m11, m12, m13, m22, m23, m33 = (
        M[..., i] for i in range(10))
    with np.errstate(all="ignore"):
        d0 = m00
        l10, l20, l30 = m01 / d0, m02 / d0, m03 / d0
        d1 = m11 - l10 * m01
        t21 = m12 - l20 * m01
        t31 = m13 - l30 * m01
        l21, l31 = t21 / d1, t31 / d1
        d2 = m22 - l20 * m02 - l21 * t21
        t32 = m23 - l30 * m02 - l31 * t21
        l32 = t32 / d2
        d3 = m33 - l30 * m03 - l31 * t31 - l32 * t32
    return (l10, l20, l30, l21, l31, l32), np.stack([d0, d1, d2, d3], axis=-1)


def _fe_solve(low, d, N):
    """Forward solve z = L^-1 N, fe = 1/2 sum z_j^2 / d_j and the back
    substitution a = L^-T D^-1 z; N (..., 4), ``low`` and ``d`` from
    ``_fe_ldl`` (broadcast against N's leading axes)."""
    l10, l20, l30, l21, l31, l32 = low
    with np.errstate(all="ignore"):
        z0 = N[..., 0]
        z1 = N[..., 1] - l10 * z0
        z2 = N[..., 2] - l20 * z0 - l21 * z1
        z3 = N[..., 3] - l30 * z0 - l31 * z1 - l32 * z2
        y = [z0 / d[..., 0], z1 / d[..., 1], z2 / d[..., 2], z3 / d[..., 3]]
        fe = (z0 * y[0] + z1 * y[1] + z2 * y[2] + z3 * y[3]) / 2
        a3 = y[3]
        a2 = y[2] - l32 * a3
        a1 = y[1] - l21 * a2 - l31 * a3
        a0 = y[0] - l10 * a1 - l20 * a2 - l30 * a3
    return fe, np.stack([a0, a1, a2, a3], axis=-1)


def fe_points(prods, ant):
    """Fe, the maximum-likelihood amplitudes a = M^-1 N and the four
    pivot ratios d_j / M_jj of every point -> ``(fe (D, nsky, F), amps
    (D, nsky, F, 4), ratio (D, nsky, F, 4))``.  No pivot rule is applied;
    the ratios let a test say on which side of the kernels' rule
    (``d_j > 1e-12 M_jj``) a point lies."""
    M, N = fe_sums(prods, ant)
    low, d = _fe_ldl(M)
    fe, amps = _fe_solve(low, d, N)
    with np.errstate(all="ignore"):
        ratio = d / M[..., [0, 4, 7, 9]]
    return fe, amps, ratio


def fe_null_products(prods, z):
    """Noise-only data products n = L_p z_p (D, F, P, 2, R), with L_p the
    2x2 Cholesky factor of [[ss, sc], [sc, cc]]_p and ``z``
    (D, F, P, 2, R)."""
    prods, z = _ld(prods), _ld(z)
    ss, cc, sc = (np.moveaxis(prods[:, :, i], 0, 2) for i in (0, 1, 2))
    assert (ss > 0).all()
    l00 = np.sqrt(ss)
    l10 = sc / l00
    schur = cc - l10 * l10
    assert (schur > 0).all()
    l11 = np.sqrt(schur)  # (D, F, P)
    z0, z1 = z[:, :, :, 0], z[:, :, :, 1]  # (D, F, P, R)
    return np.stack([l00[..., None] * z0,
                     l10[..., None] * z0 + l11[..., None] * z1], axis=3)


def fe_null_map(prods, ant, n):
    """The Fe map of every realisation (R, D, nsky, F) from the data
    products ``n`` (D, F, P, 2, R) (fp64 or longdouble, taken as exact)
    in place of the planes sr, cr."""
    n = np.asarray(n, dtype=LD)
    ant_ld = _ld(ant)
    M, _ = fe_sums(prods, ant)
    low, d = _fe_ldl(M)  # (D, nsky, F)
    D, F, P, _, R = n.shape
    ns = np.moveaxis(n[:, :, :, 0], 2, 0).reshape(P, D * F * R)
    nc = np.moveaxis(n[:, :, :, 1], 2, 0).reshape(P, D * F * R)

    def psum(coeff, q):  # -> (D, nsky, F, R)
        return np.moveaxis((coeff @ q).reshape(-1, D, F, R), 0, 1)

    fp, fx = ant_ld[:, :, 0], ant_ld[:, :, 1]
    N = np.stack([psum(fp, ns), psum(fp, nc), psum(fx, ns), psum(fx, nc)],
                 axis=-1)  # (D, nsky, F, R, 4)
    fe, _ = _fe_solve([x[..., None] for x in low], d[..., None, :], N)
    return np.moveaxis(fe, 3, 0)


def fe_null_data(white, rhs, X):
    """Joint null data ``white[p, r, 2f+c] - sum_k rhs[p, k, 2f+c]
    X[p, d, k, r]`` in the (D, F, P, 2, R) layout.  ``white``
    (P, Rp >= R, ldw >= 2F), ``rhs`` (P, mp, 2F+1), ``X`` (P, D, mp, R);
    only the entries of the formula are read."""
    X = np.asarray(X, dtype=np.float64)
    P, D, mp, R = X.shape
    F = (rhs.shape[2] - 1) // 2
    w = _ld(np.asarray(white)[:, :R, :2 * F])
    B = _ld(np.asarray(rhs)[:, :, :2 * F])
    X = X.astype(LD)
    out = np.empty((D, F, P, 2, R), dtype=LD)
    for p in range(P):
        for d in range(D):
            nd = w[p].T - B[p].T @ X[p, d]  # (2F, R)
            out[d, :, p] = nd.reshape(F, 2, R)
    return out


# ----------------------------------------------------------------------
# error measure and the tolerance rule
# ----------------------------------------------------------------------
def nerr(got, ref):
    """Normwise error of one plane: max|got - ref| / max|ref|."""
    ref = np.asarray(ref, dtype=LD)
    d = np.abs(np.asarray(got).astype(LD) - ref).max() if ref.size else LD(0)
    if not np.isfinite(d):
        return float("inf")
    scale = np.abs(ref).max() if ref.size else LD(0)
    return float(d / scale) if scale > 0 else float(d)


def tol_from_base(base):
    """tol = 16 * max(base, 64 eps64): ``base`` is the normwise error
    of a plain CPU fp64 evaluation of the same operation against this
    oracle — never a figure from the code under test.  16x covers the
    blocked/inverted-diagonal algorithm (within 2x of LAPACK in a CPU
    emulation) and the MFMA accumulation order and fused rounding."""
    return 16.0 * max(float(base), 64.0 * EPS64)


def report(label, got, base):
    """Print got / base / tol for one case and return (got, tol)."""
    tol = tol_from_base(base)
    print(f"{label}: got={got:.3e} base={base:.3e} tol={tol:.3e} "
          f"got/base={got / max(base, 1e-300):.2f}")
    return got, tol


# ----------------------------------------------------------------------
# input generators (shared by the GPU tests)
# ----------------------------------------------------------------------
def gen_sigma(rng, m, D=1, flavour="plain"):
    """(TNT (m, m), phiinv (D, m)) in fp64.

    TNT = T^T diag(1/nvec) T, T ~ N(0,1) (max(333, 2m), m),
    nvec ~ U(0.5, 2) 1e-12, mirrored from its lower triangle so every
    consumer sees one symmetric matrix.  ``plain``: phiinv ~
    U(0.5, 2) 1e10.  ``range``: the production prior spread — the first
    min(8, m-1) entries 1e-40, the rest 10**U(12, 18).  Both keep
    cond(Sigma) < 1e4 up to m = 256 (asserted in test_hpref.py)."""
    ntoa = max(333, 2 * m)
    T = rng.normal(size=(ntoa, m))
    nvec = rng.uniform(0.5, 2.0, ntoa) * 1e-12
    TNT = T.T @ (T / nvec[:, None])
    TNT = np.tril(TNT) + np.tril(TNT, -1).T
    if flavour == "plain":
        phiinv = rng.uniform(0.5, 2.0, (D, m)) * 1e10
    elif flavour == "range":
        phiinv = 10.0 ** rng.uniform(12, 18, (D, m))
        phiinv[:, :min(8, m - 1)] = 1e-40
    else:
        raise ValueError(flavour)
    return np.ascontiguousarray(TNT), phiinv


def sigma_of(TNT, phiinv_d):
    """Sigma = TNT + diag(phiinv_d), the fp64 sum the kernel forms."""
    S = np.array(TNT, dtype=np.float64)
    S[np.diag_indices_from(S)] += phiinv_d
    return S


def gen_rhs(rng, m, mp, F):
    """RHS (mp, 2F+1) ~ N(0,1) 1e6 with zero pad rows.  Random, not an
    sbgemm output: a solve failure cannot be a precompute failure."""
    B = rng.normal(size=(mp, 2 * F + 1)) * 1e6
    B[m:] = 0.0
    return B


def gen_closure(g):
    """fp64 (S (3, F), R (2, F)) from the oracle's raw dots ``g`` =
    gram(W) (5, F): S = [3 a1, 3 b1, a3 / 2], R = [2 a2, 2 b2].  For
    gsign = +1, M = [[2 a1, -a3/2], [., 2 b1]] with det >= 3.75 a1 b1
    (Cauchy-Schwarz); for gsign = -1 everything is a sum.  Neither has
    cancellation, so no (d, f) entry needs masking."""
    g = np.asarray(g, dtype=LD)
    S = np.stack([3 * g[0], 3 * g[1], g[2] / 2]).astype(np.float64)
    R = np.stack([2 * g[3], 2 * g[4]]).astype(np.float64)
    return S, R


def gen_trig(rng, ntoa, F, offset=0.0):
    """(toas, ninv, nr, freqs) in fp64: sorted TOAs over 4e8 s (plus
    ``offset``), nvec ~ U(0.5, 2) 1e-12, r ~ N(0, 1e-6), freqs
    linspace(3e-9, 5e-8, F)."""
    toas = np.sort(rng.uniform(0, 4e8, ntoa)) + offset
    nvec = rng.uniform(0.5, 2.0, ntoa) * 1e-12
    r = rng.normal(0, 1e-6, ntoa)
    freqs = np.linspace(3e-9, 5e-8, F)
    return toas, 1.0 / nvec, r / nvec, freqs


def gen_blocks(rng, sizes, log10_ecorr=-6.4):
    """Synthetic Sherman-Morrison block structure over contiguous TOA
    blocks of the given sizes: (uvec (ntoa,), beta (nblk,), offsets,
    sizes (int64)).  uvec = 1 / nvec; beta_b = e2 / (1 + e2 sum(u_b)),
    and 0 on singleton blocks (the kernel's no-ecorr convention)."""
    sizes = np.asarray(sizes, dtype=np.int64)
    offsets = np.concatenate([[0], np.cumsum(sizes)[:-1]]).astype(np.int64)
    ntoa = int(sizes.sum())
    uvec = 1.0 / (rng.uniform(0.5, 2.0, ntoa) * 1e-12)
    e2 = (10.0 ** log10_ecorr) ** 2
    beta = np.array([
        0.0 if sz == 1 else e2 / (1.0 + e2 * uvec[o:o + sz].sum())
        for o, sz in zip(offsets, sizes)
    ])
    return uvec, beta, offsets, sizes


def gen_fe_case(rng, P, D, F, nsky, delta=None, rows=None):
    """(prods (P, D, 5, F), ant (nsky, P, 2)) in fp64, the synthetic
    products of the Fe tests: ss, cc ~ U(1, 2), sc = 0.1 N(0, 1), sr, cr
    ~ N(0, 1) and a normal antenna table, so every M is a sum of
    independent positive-definite terms.

    With ``delta`` the sky rows ``rows`` (all rows if ``None``) get
    ``Fx = 2 F+ + delta g``, g ~ N(0, 1): M is singular at delta = 0 and
    its two last pivots shrink like delta^2.  ``delta`` is a scalar or
    one value per entry of ``rows``."""
    prods = np.empty((P, D, 5, F))
    prods[:, :, 0:2] = rng.uniform(1.0, 2.0, (P, D, 2, F))
    prods[:, :, 2] = 0.1 * rng.normal(size=(P, D, F))
    prods[:, :, 3:] = rng.normal(size=(P, D, 2, F))
    ant = rng.normal(size=(nsky, P, 2))
    if delta is not None:
        rows = np.arange(nsky) if rows is None else np.asarray(rows)
        delta = np.broadcast_to(np.asarray(delta, dtype=np.float64),
                                rows.shape)
        g = rng.normal(size=(len(rows), P))
        ant[rows, :, 1] = 2.0 * ant[rows, :, 0] + delta[:, None] * g
    return prods, ant


def amp_err(got, ref):
    """Amplitude error (docs/VALIDATION.md): max|da| / max|a| per point,
    the largest over the points; ``got`` and ``ref`` (..., 4)."""
    ref = np.asarray(ref, dtype=LD)
    d = np.abs(np.asarray(got).astype(LD) - ref).max(axis=-1)
    q = d / np.abs(ref).max(axis=-1)
    return float(q.max()) if np.isfinite(q).all() else float("inf")


def gen_null_data(rng, P, D, F, m, mp, R, wide=False):
    """(white (P, Rp, ldw), rhs (P, mp, 2F+1), X (P, D, mp, R)) of
    ``fe_null_data`` with NaN in everything that must not be read: the
    last column of rhs, the columns >= 2F and the rows >= R of white.
    X has zero padding rows m..mp.  Rp = pad16(R) and ldw = 2F + 1 as the
    engine allocates them; ``wide``: ldw = 2F + 3 and 16 more rows."""
    Rp = (R + 15) // 16 * 16 + (16 if wide else 0)
    ldw = 2 * F + (3 if wide else 1)
    white = np.full((P, Rp, ldw), np.nan)
    white[:, :R, :2 * F] = rng.normal(size=(P, R, 2 * F))
    rhs = np.full((P, mp, 2 * F + 1), np.nan)
    rhs[:, :, :2 * F] = rng.normal(size=(P, mp, 2 * F))
    X = np.zeros((P, D, mp, R))
    X[:, :, :m] = rng.normal(size=(P, D, m, R))
    return white, rhs, X


def null_data64(white, rhs, X):
    """The plain fp64 einsum of ``fe_null_data`` and the componentwise
    forward bound of its length-mp dot products without the leading
    ``4 mp eps``: ``|white| + |B|^T |X|``, both (D, F, P, 2, R)."""
    P, D, mp, R = X.shape
    F = (rhs.shape[2] - 1) // 2
    B = rhs[:, :, :2 * F]
    w = white[:, :R, :2 * F].transpose(0, 2, 1)[:, None]  # (P, 1, 2F, R)

    def lay(a):
        return a.reshape(P, D, F, 2, R).transpose(1, 2, 0, 3, 4)

    return (lay(w - np.einsum("pkj,pdkr->pdjr", B, X)),
            lay(np.abs(w) + np.einsum("pkj,pdkr->pdjr", np.abs(B), np.abs(X))))


# ----------------------------------------------------------------------
# assembled cases (cached: built once, shared, never modified)
# ----------------------------------------------------------------------
class Case:
    """Bag of read-only arrays."""

    def __init__(self, **kw):
        for k, v in kw.items():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
            setattr(self, k, v)


def _cpu_fsub64(L64, B64):
    from scipy.linalg import solve_triangular

    return solve_triangular(L64, B64, lower=True)


_SOLVE_CASES = {}


def solve_case(nbt, F, P=2, D=2, pad=5, seed=0):
    """Inputs and references for one isolated solve at mp = 16 nbt.

    Even pulsars have m = mp (no identity padding), odd ones
    m = mp - pad.  L and invd are the oracle's factor and block
    inverses rounded to fp64 (identity-padded), so a failure belongs to
    the solve and not to a factor; the reference W solves with that
    rounded L exactly.  S, R come from ``gen_closure`` of draw 0 (a
    pulsar's sNs/sNr are shared by its draws; the plain phiinv is a
    1e-4 perturbation of TNT, so every draw keeps det >= 3 a1 b1 —
    asserted in test_hpref.py).

    Fields: m (P,), mp, L (P*D, mp, mp), invd (P*D, nbt, 16, 16),
    RHS (P, mp, 2F+1), S (P, 3, F), R (P, 2, F), W (P, D, mp, 2F+1)
    longdouble and W64 its scipy fp64 counterpart, g (P, D, 5, F)."""
    key = (nbt, F, P, D, pad, seed)
    if key in _SOLVE_CASES:
        return _SOLVE_CASES[key]
    rng = np.random.default_rng([seed, nbt, F, P, D])
    mp = 16 * nbt
    ms = np.array([mp if p % 2 == 0 else max(1, mp - pad) for p in range(P)])
    ncol = 2 * F + 1
    L = np.empty((P * D, mp, mp))
    invd = np.empty((P * D, nbt, 16, 16))
    RHS = np.empty((P, mp, ncol))
    S, R = np.empty((P, 3, F)), np.empty((P, 2, F))
    W = np.empty((P, D, mp, ncol), dtype=LD)
    W64 = np.empty((P, D, mp, ncol))
    g = np.empty((P, D, 5, F), dtype=LD)
    for p in range(P):
        m = int(ms[p])
        TNT, phiinv = gen_sigma(rng, m, D)
        RHS[p] = gen_rhs(rng, m, mp, F)
        for d in range(D):
            Lref = chol(sigma_of(TNT, phiinv[d]))
            L64 = padded(Lref.astype(np.float64), mp)
            L[p * D + d] = L64
            invd[p * D + d] = diag_block_inverses(L64).astype(np.float64)
            W[p, d] = fsub(L64, RHS[p])
            W64[p, d] = _cpu_fsub64(L64, RHS[p])
            g[p, d] = gram(W[p, d])
        S[p], R[p] = gen_closure(g[p, 0])
    case = Case(m=ms, mp=mp, F=F, P=P, D=D, L=L, invd=invd, RHS=RHS, S=S,
                R=R, W=W, W64=W64, g=g)
    _SOLVE_CASES[key] = case
    return case


def solve_refs(case, gsign):
    """(prods_ref, prods_base64, fp_ref, fp_base64), each (P, D, ...):
    the oracle's planes and Fp, and the plain fp64 ones from the scipy
    solve."""
    P, D = case.P, case.D
    pr = np.stack([np.stack([
        products(case.W[p, d], case.S[p], case.R[p], gsign)
        for d in range(D)]) for p in range(P)])
    pb = np.stack([np.stack([
        products(case.W64[p, d], case.S[p], case.R[p], gsign, np.float64)
        for d in range(D)]) for p in range(P)])
    return pr, pb, fp_from_products(pr), fp_from_products(pb, np.float64)


_FACTOR_CASES = {}


def factor_case(m, P=1, D=1, flavour="plain", seed=0):
    """Sigma inputs with the oracle's and LAPACK's factors.

    Fields: TNT (P, m, m), phiinv (P, D, m), Lref (P, D, m, m)
    longdouble, L64 (P, D, m, m) numpy.linalg.cholesky."""
    key = (m, P, D, flavour, seed)
    if key in _FACTOR_CASES:
        return _FACTOR_CASES[key]
    rng = np.random.default_rng([seed, m, P, D, len(flavour)])
    TNT = np.empty((P, m, m))
    phiinv = np.empty((P, D, m))
    Lref = np.empty((P, D, m, m), dtype=LD)
    L64 = np.empty((P, D, m, m))
    for p in range(P):
        TNT[p], phiinv[p] = gen_sigma(rng, m, D, flavour)
        for d in range(D):
            Sig = sigma_of(TNT[p], phiinv[p, d])
            Lref[p, d] = chol(Sig)
            L64[p, d] = np.linalg.cholesky(Sig)
    case = Case(m=m, P=P, D=D, TNT=TNT, phiinv=phiinv, Lref=Lref, L64=L64)
    _FACTOR_CASES[key] = case
    return case


def block_inverses64(L64):
    """Plain fp64 counterpart of ``diag_block_inverses`` (scipy)."""
    eye = np.eye(16)
    return np.stack([
        _cpu_fsub64(np.tril(L64[k:k + 16, k:k + 16]), eye)
        for k in range(0, L64.shape[0], 16)
    ])


# ----------------------------------------------------------------------
# Fe cases: inputs, the oracle's planes and the host fp64 planes
# ----------------------------------------------------------------------
def fe_host(prods, ant):
    """The host fp64 path of the project on the same inputs:
    ``festat._assemble_fe_draws`` per sky row -> ``(fe (D, nsky, F),
    amps (D, nsky, F, 4))``.  Its error against the oracle is the
    ``base`` of every Fe tolerance."""
    from fastfp_amd.festat import _assemble_fe_draws

    out = [_assemble_fe_draws(prods, ant[k, :, 0], ant[k, :, 1],
                              amplitudes=True) for k in range(ant.shape[0])]
    return (np.stack([o[0] for o in out], axis=1),
            np.stack([o[1] for o in out], axis=1))


def _fe_case(prods, ant, **kw):
    fe, amps, ratio = fe_points(prods, ant)
    fe64, amps64 = fe_host(prods, ant)
    P, D, _, F = prods.shape
    return Case(P=P, D=D, F=F, nsky=ant.shape[0], prods=prods, ant=ant,
                fe=fe, amps=amps, ratio=ratio, fe64=fe64, amps64=amps64, **kw)


_FE_CASES = {}


def fe_case(P, D, F, nsky, seed=0):
    """One well-conditioned ``gen_fe_case`` with its references.

    Fields: prods, ant, the oracle's fe (D, nsky, F), amps and ratio
    (D, nsky, F, 4), and the host's fe64, amps64."""
    key = (P, D, F, nsky, seed)
    if key not in _FE_CASES:
        rng = np.random.default_rng([seed, P, D, F, nsky])
        _FE_CASES[key] = _fe_case(*gen_fe_case(rng, P, D, F, nsky))
    return _FE_CASES[key]


# The conditioning ladder: D = 2, F = 9, nsky = 20, four sky rows per
# rung; rows 16, 17 lie far below the kernels' pivot rule, rows 18, 19
# are untouched.  P = 2 has no 1e-3 / 1e-4 rungs (its fourth pivot is
# already at 1e-13 M_33 there): rows 8..15 stay untouched.  With these
# seeds every kept point has all pivot ratios >= 1e-10 and every skipped
# one a ratio < 1e-14 (tests/test_hpref.py), two decades on either side
# of the kernels' 1e-12 rule.
LADDER_P = (2, 3, 5, 8, 67)
LADDER_SKIP = (16, 17)
LADDER_KEEP_MIN, LADDER_SKIP_MAX = 1e-10, 1e-14
_LADDER_CASES = {}


def ladder_rungs(P):
    """{delta or None: sky rows} of the kept rungs of the ladder case."""
    if P == 2:
        return {1e-1: range(0, 4), 1e-2: range(4, 8),
                None: list(range(8, 16)) + [18, 19]}
    return {1e-1: range(0, 4), 1e-2: range(4, 8), 1e-3: range(8, 12),
            1e-4: range(12, 16), None: [18, 19]}


def fe_ladder_case(P):
    """The ladder case of ``P`` pulsars with the references of
    ``fe_case`` and ``rungs`` (``ladder_rungs``), ``keep`` (sky rows the
    kernels must keep) and ``skip`` (rows they must skip)."""
    if P not in _LADDER_CASES:
        rungs = ladder_rungs(P)
        rows, delta = [], []
        for dl, rr in rungs.items():
            if dl is not None:
                rows += list(rr)
                delta += [dl] * len(rr)
        rows += list(LADDER_SKIP)
        delta += [1e-8] * len(LADDER_SKIP)
        rng = np.random.default_rng([0, P, 1234])
        prods, ant = gen_fe_case(rng, P, 2, 9, 20, delta=delta, rows=rows)
        keep = np.array(sorted(r for rr in rungs.values() for r in rr))
        _LADDER_CASES[P] = _fe_case(
            prods, ant, rungs={k: np.array(list(v)) for k, v in rungs.items()},
            keep=keep, skip=np.array(LADDER_SKIP))
    return _LADDER_CASES[P]


def fe_null_refs(prods, ant, z, rows=None):
    """References of ``fe_null_skymax`` on the sky rows ``rows`` (all if
    ``None``), in both modes.  ``z`` (D, F, P, 2, R) standard normals.

    Fields: z, n64 (the oracle's n = L z rounded to fp64: the input of
    the data mode); per mode ``m`` in ("z", "n"): map_m (R, D, nrows, F)
    longdouble, max_m / arg_m (R, D, F) from it (the index is into
    ``rows``), and host_m, the femax of ``festat._null_max_host``."""
    from fastfp_amd.festat import _null_max_host

    sub = ant if rows is None else ant[np.asarray(rows)]
    n = fe_null_products(prods, z)
    n64 = np.ascontiguousarray(n.astype(np.float64))
    out = dict(z=z, n64=n64)
    for m, src in (("z", n), ("n", n64)):
        fmap = fe_null_map(prods, sub, src)
        out["map_" + m] = fmap
        out["max_" + m] = fmap.max(axis=2)
        out["arg_" + m] = fmap.argmax(axis=2)
    out["host_z"] = _null_max_host(prods, sub, z)[0]
    out["host_n"] = _null_max_host(prods, sub, n=n64)[0]
    return Case(**out)


_LADDER_NULL = {}


def fe_ladder_null(P, R=17):
    """``fe_null_refs`` of the ladder case over its kept rows."""
    if (P, R) not in _LADDER_NULL:
        case = fe_ladder_case(P)
        z = np.random.default_rng([7, P, R]).standard_normal((2, 9, P, 2, R))
        _LADDER_NULL[P, R] = fe_null_refs(case.prods, case.ant, z,
                                          rows=case.keep)
    return _LADDER_NULL[P, R]


_NULL_CASES = {}


def fe_null_case(P, D, F, nsky, R, seed=0):
    """``fe_case(P, D, F, nsky)`` with R realisations -> (case, refs of
    ``fe_null_refs``)."""
    key = (P, D, F, nsky, R, seed)
    if key not in _NULL_CASES:
        case = fe_case(P, D, F, nsky, seed)
        rng = np.random.default_rng([seed, P, D, F, nsky, R])
        z = rng.standard_normal((D, F, P, 2, R))
        _NULL_CASES[key] = (case, fe_null_refs(case.prods, case.ant, z))
    return _NULL_CASES[key]


# the tie case: P = 9, D = 2, F = 9, nsky = 130; row 70 copied into rows
# 3, 19, 35 (waves 0, 1, 2 of the first sky round) and 99 (wave 2 of the
# second; row 70 itself is wave 0 of the second)
TIE_ROWS = (3, 19, 35, 70, 99)
_TIE_CASES = {}


def fe_tie_case(scaled=True):
    """(prods, ant, ant2) of the tie case; ``ant2`` is ``ant`` with row 3
    replaced by a fresh random row.  ``scaled``: sr, cr are a signal of
    random amplitudes from row 70, a hundred times the unit noise, which
    makes the equal rows the largest of every column."""
    if scaled not in _TIE_CASES:
        P, D, F, nsky = 9, 2, 9, 130
        rng = np.random.default_rng([0, P, D, F, nsky, 99])
        prods, ant = gen_fe_case(rng, P, D, F, nsky)
        for r in TIE_ROWS:
            ant[r] = ant[70]
        if scaled:
            a = rng.normal(size=(D, F, 4))
            fp, fx = ant[70, :, 0, None, None], ant[70, :, 1, None, None]
            s = fp * a[..., 0] + fx * a[..., 2]  # (P, D, F)
            c = fp * a[..., 1] + fx * a[..., 3]
            ss, cc, sc = prods[:, :, 0], prods[:, :, 1], prods[:, :, 2]
            prods[:, :, 3] += 100.0 * (ss * s + sc * c)
            prods[:, :, 4] += 100.0 * (sc * s + cc * c)
        ant2 = ant.copy()
        ant2[3] = np.random.default_rng(98).normal(size=(P, 2))
        for a in (prods, ant, ant2):
            a.setflags(write=False)
        _TIE_CASES[scaled] = (prods, ant, ant2)
    return _TIE_CASES[scaled]


# shapes of tests/test_fe_oracle.py; tests/test_hpref.py checks on the
# CPU that every one of them is far on the kept side of the pivot rule
FE_SHAPES = [  # (P, D, F, nsky)
    (2, 1, 1, 1), (3, 1, 16, 16), (4, 3, 5, 17), (5, 1, 17, 64),
    (7, 3, 11, 65), (8, 2, 8, 81), (9, 5, 7, 130), (12, 1, 33, 65),
    (13, 2, 17, 15), (76, 1, 3, 65), (77, 3, 5, 17), (248, 1, 17, 65),
]
FE_AMP_SHAPES = [(5, 5, 7, 20), (9, 4, 16, 65), (3, 5, 13, 17),
                 (67, 2, 65, 81)]
FE_NULL_SHAPES = [  # (P, D, F, nsky, R)
    (2, 1, 1, 1, 1), (3, 1, 16, 17, 16), (5, 3, 5, 65, 17),
    (8, 2, 8, 81, 33), (9, 1, 17, 130, 70), (67, 3, 11, 65, 65),
]
