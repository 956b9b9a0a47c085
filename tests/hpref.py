"""Extended-precision oracle for the solve and precompute kernels.

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
``gen_blocks``); ``tests/test_hpref.py`` checks both halves on the CPU.
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
