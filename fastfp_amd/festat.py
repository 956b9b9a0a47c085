"""Earth-term Fe-statistic: sky-coherent continuous-wave detection.

The reference lists this as an open to-do (its README: "Include
Fe-statistic?") and never implemented it; this module completes that
roadmap natively.  Where Fp maximizes a per-pulsar 2-amplitude
filter incoherently (one 2x2 solve per pulsar), Fe maximizes the
EARTH-TERM signal coherently across the array (Ellis, Siemens &
Creighton 2012): four sky-dependent filters

    A1 = F+(p) sin(2 pi f t),  A2 = F+(p) cos(2 pi f t),
    A3 = Fx(p) sin(2 pi f t),  A4 = Fx(p) cos(2 pi f t),

with the antenna patterns F+/Fx of each pulsar toward a trial sky
location, and

    Fe(f, sky) = 1/2 N^T M^-1 N,
    N_i = sum_p (A_i | r)_p,   M_ij = sum_p (A_i | A_j)_p,

inner products ``(x|y) = x^T C_p^{-1} y`` exactly as in Fp.  Because
every filter is an antenna-coefficient multiple of the SAME per-pulsar
sin/cos pair, the whole sky dependence factors out of the expensive
linear algebra: the engine computes the five corrected per-pulsar
products (s|s), (c|c), (s|c), (s|r), (c|r) ONCE per frequency (the
same quantities the Fp kernels reduce), and any number of sky
locations costs only an O(P) 4x4 assembly each.  A full (sky x freq)
Fe map is therefore nearly free on top of an Fp sweep — the
MI355X-native restructure of the statistic.

Two assemblies exist.  The default (``assemble="host"``) takes the
products from the torch path and solves the 4x4 systems in numpy
(:func:`_assemble_fe_draws`).  On a HIP engine ``assemble="device"`` and
``sweep_max`` take the products from the HIP solve
(``FpEngine.sweep_products_hip``) and run the sky assembly in the MFMA
kernels ``ops.fe_assemble`` / ``ops.fe_skymax``; ``sweep_max`` returns
the statistic maximised over the sky with its argmax and never forms the
(draws x sky x freqs) cube.  :class:`FastFe` and :class:`NMFe` differ
only in where the products (P, draws, 5, F) come from; the sky layer
:class:`_Sky` under both chooses between the kernels and the host.

The same solve yields the maximum-likelihood amplitudes ``a = M^-1 N``:
``sweep_max(amplitudes=True)`` returns them at the sky maximum and
``FastFe.amplitudes`` at one chosen sky position (``ops.fe_amplitudes``
on a HIP engine, the host solve otherwise); :func:`cw_amplitudes` and
:func:`cw_parameters` map between ``a`` and the source parameters
(zeta or h0, cos iota, psi, phi0) — docs/DESIGN.md section 12.

Significance of the sky maximum: ``FastFe.null_max`` / ``NMFe.null_max``
draw the maximum under noise alone and ``FastFe.false_alarm`` turns the
observed maximum into a false-alarm probability, without a solve per
realisation — for ``r ~ N(0, C)`` the data products of a pulsar are
exactly ``(sr, cr) ~ N(0, [[ss, sc], [sc, cc]])`` (``ops.fe_null_skymax``
on a HIP engine, :func:`_null_max_host` otherwise; docs/DESIGN.md
section 13).  With ``joint=True`` the realisations are drawn jointly
across frequencies — one noise realisation per pulsar for the whole grid,
``FpEngine.null_data`` — and :func:`global_false_alarm` gives the
probability that noise alone makes ANY frequency as loud as the loudest
observed one (section 14).
"""

from __future__ import annotations

import math

import numpy as np
import torch

from fastfp_amd import ops
from fastfp_amd.engine import FpEngine, _t64
from fastfp_amd.noise import batch_phiinv
from fastfp_amd.xcy import get_xCy


def gw_antenna_pattern(pos, gwtheta: float, gwphi: float):
    """Antenna pattern functions (F+, Fx) of a pulsar at unit vector
    ``pos`` for a GW source at sky colatitude ``gwtheta`` / longitude
    ``gwphi`` (standard PTA convention; enterprise's
    ``create_gw_antenna_pattern``):

        m = [sin phi, -cos phi, 0]
        n = [-cos theta cos phi, -cos theta sin phi, sin theta]
        omhat = -[sin theta cos phi, sin theta sin phi, cos theta]
        F+ = 1/2 ((m.p)^2 - (n.p)^2) / (1 + omhat.p)
        Fx = (m.p)(n.p) / (1 + omhat.p)

    ``pos`` may be (3,) or (P, 3); returns scalars or (P,) arrays.
    Singular when the pulsar lies exactly at the source direction
    (omhat.p = -1).
    """
    st, ct = math.sin(gwtheta), math.cos(gwtheta)
    sp, cp = math.sin(gwphi), math.cos(gwphi)
    m = np.array([sp, -cp, 0.0])
    n = np.array([-ct * cp, -ct * sp, st])
    omhat = np.array([-st * cp, -st * sp, -ct])
    pos = np.asarray(pos, dtype=np.float64)
    mp_ = pos @ m
    np_ = pos @ n
    denom = 1.0 + pos @ omhat
    fplus = 0.5 * (mp_**2 - np_**2) / denom
    fcross = mp_ * np_ / denom
    return fplus, fcross


def cw_amplitudes(zeta, cosi, psi, phi0):
    """The four Fe amplitudes of an Earth-term continuous wave.

    Signal model (docs/DESIGN.md, "Fe amplitudes"): with ``Phi(t) = 2 pi
    f t + phi0``, ``zeta = h0 / (2 pi f)`` and ``c = cosi``,

        r+ = zeta [ (1 + c^2) sin Phi cos 2psi + 2c cos Phi sin 2psi]
        rx = zeta [-(1 + c^2) sin Phi sin 2psi + 2c cos Phi cos 2psi]
        r_p = F+_p r+ + Fx_p rx
            = F+_p (a1 sin + a2 cos) + Fx_p (a3 sin + a4 cos),

    sin / cos of ``2 pi f t`` — the filter order of :class:`FastFe`.
    The arguments broadcast; returns (..., 4) = [a1, a2, a3, a4].
    """
    zeta, cosi, psi, phi0 = np.broadcast_arrays(
        *(np.asarray(x, dtype=np.float64) for x in (zeta, cosi, psi, phi0)))
    Ap = zeta * (1.0 + cosi**2)
    Ac = 2.0 * zeta * cosi
    c2, s2 = np.cos(2.0 * psi), np.sin(2.0 * psi)
    cp, sp = np.cos(phi0), np.sin(phi0)
    return np.stack([
        Ap * c2 * cp - Ac * s2 * sp,
        Ap * c2 * sp + Ac * s2 * cp,
        -Ap * s2 * cp - Ac * c2 * sp,
        -Ap * s2 * sp + Ac * c2 * cp,
    ], axis=-1)


def cw_parameters(a, f=None) -> dict:
    """Inverse of :func:`cw_amplitudes`: ``a`` (..., 4) -> dict of
    ``zeta``, ``cosi``, ``psi``, ``phi0`` arrays of the leading shape,
    plus ``h0 = 2 pi f zeta`` when the frequency ``f`` (broadcast against
    the leading shape) is given.

    ``psi`` is returned in [0, pi/2) and ``phi0`` in [0, 2 pi):
    ``(psi + pi/2, phi0 + pi)`` is the same signal.  At circular
    polarisation (``|cosi| = 1``) only ``phi0 +- 2 psi`` is determined;
    the returned pair still reproduces ``a``.
    """
    a = np.asarray(a, dtype=np.float64)
    a1, a2, a3, a4 = a[..., 0], a[..., 1], a[..., 2], a[..., 3]
    S = a1**2 + a2**2 + a3**2 + a4**2  # Ap^2 + Ac^2
    Dd = a1 * a4 - a2 * a3  # Ap Ac
    r = np.sqrt(np.maximum(S**2 - 4.0 * Dd**2, 0.0))
    Ap = np.sqrt(0.5 * (S + r))
    Ac = np.sign(Dd) * np.sqrt(np.maximum(0.5 * (S - r), 0.0))
    zeta = 0.5 * (Ap + np.sqrt(np.maximum(Ap**2 - Ac**2, 0.0)))
    pos = zeta > 0.0
    cosi = np.where(pos, Ac, 0.0) / np.where(pos, 2.0 * zeta, 1.0)
    alpha = np.arctan2(a2 - a3, a1 + a4)  # 2 psi + phi0
    beta = np.arctan2(a2 + a3, a1 - a4)  # phi0 - 2 psi
    psi = 0.25 * (alpha - beta)
    phi0 = 0.5 * (alpha + beta)
    # canonical range: every quarter turn of psi is half a turn of phi0
    k = np.floor(psi / (0.5 * np.pi))
    psi = psi - k * (0.5 * np.pi)
    over = psi >= 0.5 * np.pi  # rounding of a psi just below zero
    psi = np.where(over, psi - 0.5 * np.pi, psi)
    k = np.where(over, k + 1.0, k)
    psi = np.maximum(psi, 0.0)
    phi0 = np.mod(phi0 - k * np.pi, 2.0 * np.pi)
    phi0 = np.where(phi0 >= 2.0 * np.pi, 0.0, phi0)
    out = {"zeta": zeta, "cosi": cosi, "psi": psi, "phi0": phi0}
    if f is not None:
        out["h0"] = 2.0 * np.pi * np.asarray(f, dtype=np.float64) * zeta
    return out


def _solve4(M, N, rcond):
    """``M^-1 N`` for stacked 4x4 systems ``M`` (..., 4, 4) and ``N``
    (..., 4).  If LAPACK finds any system of the stack singular, every
    one of them goes through the pseudo-inverse."""
    try:
        return np.linalg.solve(M, N[..., None])[..., 0]
    except np.linalg.LinAlgError:
        flatM = M.reshape(-1, 4, 4)
        flatN = N.reshape(-1, 4)
        return np.stack([np.linalg.pinv(Mi, rcond=rcond) @ Ni
                         for Mi, Ni in zip(flatM, flatN)]).reshape(N.shape)


def _psum(coeff, q):
    """``sum_p coeff_p q_p``: (P,) x (P, ...) -> (...)."""
    return np.einsum("p,p...->...", coeff, q)


# (row, column) of the ten unique entries of the symmetric 4x4 M
_UPPER = [(i, j) for i in range(4) for j in range(i, 4)]


def _moments(prods, fplus, fcross):
    """The ten unique entries of ``M`` for one sky row, ``(m00, m01, m02,
    m03, m11, m12, m13, m22, m23, m33)`` as in ``_UPPER``, each (D, F), from
    the planes ss, cc, sc of ``prods`` (P, D, 5, F) and (P,) coefficients."""
    ss, cc, sc = prods[:, :, 0], prods[:, :, 1], prods[:, :, 2]
    fp2, fx2, fpx = fplus**2, fcross**2, fplus * fcross
    m03 = _psum(fpx, sc)  # = m12
    return (_psum(fp2, ss), _psum(fp2, sc), _psum(fpx, ss), m03,
            _psum(fp2, cc), m03, _psum(fpx, cc),
            _psum(fx2, ss), _psum(fx2, sc), _psum(fx2, cc))


def _full_m(moments):
    """The symmetric ``M`` (..., 4, 4) from its ten unique entries."""
    M = np.empty(moments[0].shape + (4, 4))
    for (i, j), m in zip(_UPPER, moments):
        M[..., i, j] = M[..., j, i] = m
    return M


def _assemble_fe_draws(prods, fplus, fcross, rcond=1e-12, amplitudes=False):
    """Fe(draw, f) from per-pulsar corrected products, the one 4x4
    assembly of the host side.  ``prods``: (P, D, 5, F) array of [ss, cc,
    sc, sr, cr]; ``fplus`` / ``fcross``: (P,) antenna coefficients.
    Returns (D, F), or with ``amplitudes`` the pair ``(fe (D, F), a (D, F,
    4))`` with the maximum-likelihood amplitudes ``a = M^-1 N``.

    M is assembled per (draw, frequency) from sums over pulsars and
    solved as a 4x4 system; near-degenerate skies (e.g. all pulsars
    clustered: F+/Fx columns collinear) go through the pseudo-inverse —
    the maximized likelihood is well-defined on the column space."""
    M = _full_m(_moments(prods, fplus, fcross))
    sr, cr = prods[:, :, 3], prods[:, :, 4]
    N = np.stack([_psum(fplus, sr), _psum(fplus, cr),
                  _psum(fcross, sr), _psum(fcross, cr)], axis=-1)  # (D, F, 4)
    x = _solve4(M, N, rcond)
    fe = 0.5 * np.einsum("dfi,dfi->df", N, x)
    return (fe, x) if amplitudes else fe


def _assemble_fe(prods, fplus, fcross, rcond=1e-12, amplitudes=False):
    """:func:`_assemble_fe_draws` for one draw: ``prods`` (P, 5, F) ->
    (F,), or with ``amplitudes`` -> ``(fe (F,), a (F, 4))``."""
    out = _assemble_fe_draws(prods[:, None], fplus, fcross, rcond, amplitudes)
    return (out[0][0], out[1][0]) if amplitudes else out[0]


def _default_device(device):
    return device or ("cuda" if torch.cuda.is_available() else "cpu")


def _check_assemble(assemble, device, engine):
    """Validate the ``assemble=`` keyword and resolve the default
    device.  ``"device"`` needs a HIP engine: a CPU device (or a CPU
    engine) is rejected before any precompute runs."""
    if assemble not in ("host", "device"):
        raise ValueError(
            f"assemble must be 'host' or 'device', got {assemble!r}")
    device = _default_device(device)
    if assemble == "device":
        dev = engine.device if engine is not None else torch.device(device)
        if dev.type != "cuda":
            raise ValueError(
                "assemble='device' runs the sky assembly in the HIP "
                f"kernels and needs a GPU engine (got device {dev}); use "
                "assemble='host' on the CPU")
    return device


def _obtain_engine(engine, psrs, freqs, Nvecs, Ts, device, freq_chunk=2048,
                   compress=None):
    """The caller's engine as it is, or a fresh one on ``device`` (by
    default the GPU where there is one) precomputed on ``freqs``, with
    draw compression around ``compress = (rn_sigs, samples)`` if given."""
    if engine is not None:
        return engine
    engine = FpEngine(psrs, Nvecs, Ts, device=_default_device(device))
    engine.precompute(freqs, freq_chunk=freq_chunk)
    if compress is not None:
        engine.compress_around_first_draw(*compress)
    return engine


def _phiinvs_from_sigmas(engine, sigmas, improper=False):
    """Fixed-noise (m, m) sigmas -> per-pulsar diagonal phi^-1 (the
    ``get_mats_fp`` contract sigma = TNT + diag(phi^-1), as in
    ``FpEngine.sweep``).

    The difference knows a prior only to the rounding of ``TNT_kk``, up to
    ``ntoa eps TNT_kk`` for a sum of ``ntoa`` positive terms.  That is
    harmless where the prior is added back to ``TNT``; the joint null
    also takes its square root, which turns rounding of relative size
    ``1e-16`` into a term of relative size ``1e-8`` that differs from
    device to device.  With ``improper`` every entry not above ``ntoa eps
    TNT_kk`` is therefore set to zero, an improper prior: a proper prior
    that weak moves the data by at most ``sqrt(ntoa eps)`` of their
    white-noise scatter."""
    out = []
    for blk, sg in zip(engine.blocks, sigmas):
        tnt = torch.diagonal(blk.TNT)
        p = (torch.diagonal(_t64(sg, engine.device)) - tnt).contiguous()
        if improper:
            floor = blk.ntoa * torch.finfo(torch.float64).eps * tnt
            p = torch.where(p > floor, p, torch.zeros_like(p))
        out.append(p)
    return out


def _antenna_table(pos, sky, device=None):
    """(nsky, P, 2) = [F+, Fx] of every pulsar toward every sky point;
    a numpy array, or an fp64 tensor on ``device``."""
    ant = np.empty((len(sky), pos.shape[0], 2))
    for k, (gwtheta, gwphi) in enumerate(sky):
        ant[k, :, 0], ant[k, :, 1] = gw_antenna_pattern(pos, gwtheta, gwphi)
    if device is None:
        return ant
    return torch.as_tensor(ant, dtype=torch.float64).to(device)


_NOT_PD = ("the product block [[ss, sc], [sc, cc]] of (pulsar {p}, draw {d}, "
           "frequency {f}) is not positive definite: it is no covariance to "
           "draw noise-only products from")


def _null_factors(prods, xp=np):
    """Cholesky factors ``(l00, l10, l11)``, each (P, D, F), of the
    per-pulsar blocks ``[[ss, sc], [sc, cc]]`` of ``prods`` (P, D, 5, F):
    numpy arrays, or with ``xp=torch`` tensors beside ``prods`` (one
    sync).  Raises ``ValueError`` naming the first (pulsar, draw,
    frequency) whose block is not positive definite (``ss <= 0``, a Schur
    complement ``<= 0`` or a non-finite value)."""
    ss, cc, sc = prods[:, :, 0], prods[:, :, 1], prods[:, :, 2]
    with np.errstate(all="ignore"):
        l00 = xp.sqrt(ss)
        l10 = sc / l00
        schur = cc - l10 * l10
        l11 = xp.sqrt(schur)
    ok = (xp.isfinite(ss) & xp.isfinite(cc) & xp.isfinite(sc)
          & xp.isfinite(l10) & xp.isfinite(schur) & (ss > 0) & (schur > 0))
    if not bool(ok.all()):
        p, d, f = (int(i) for i in xp.argwhere(~ok)[0])
        raise ValueError(_NOT_PD.format(p=p, d=d, f=f))
    return l00, l10, l11


def _null_draws(prods, z):
    """Noise-only data products ``n = L z``: ``prods`` (P, D, 5, F) and
    standard normals ``z`` (D, F, P, 2, R) -> ``(n_s, n_c)``, each
    (P, D, F, R), distributed as ``(sr, cr)`` under noise alone."""
    l00, l10, l11 = _null_factors(prods)
    z0 = np.moveaxis(z[:, :, :, 0, :], 2, 0)  # (P, D, F, R)
    z1 = np.moveaxis(z[:, :, :, 1, :], 2, 0)
    return l00[..., None] * z0, l10[..., None] * z0 + l11[..., None] * z1


def _ldl4(moments, rcond):
    """Elementwise LDL^T of the 4x4 ``M`` given by its ten unique entries
    (the factorisation and pivot rule of the kernels).  Returns ``(ok,
    (l10, l20, l30, l21, l31, l32, i0, i1, i2, i3))``: ``ok`` where all
    four pivots pass, the unit-lower entries and the inverse pivots."""
    m00, m01, m02, m03, m11, m12, m13, m22, m23, m33 = moments

    def pivot_ok(s, mjj):
        return (s > rcond * mjj) & (s < np.inf)

    d0 = m00
    ok = pivot_ok(d0, m00)
    i0 = 1.0 / d0
    l10, l20, l30 = m01 * i0, m02 * i0, m03 * i0
    d1 = m11 - l10 * m01
    ok &= pivot_ok(d1, m11)
    i1 = 1.0 / d1
    t21 = m12 - l20 * m01
    t31 = m13 - l30 * m01
    l21, l31 = t21 * i1, t31 * i1
    d2 = m22 - l20 * m02 - l21 * t21
    ok &= pivot_ok(d2, m22)
    i2 = 1.0 / d2
    t32 = m23 - l30 * m02 - l31 * t21
    l32 = t32 * i2
    d3 = m33 - l30 * m03 - l31 * t31 - l32 * t32
    ok &= pivot_ok(d3, m33)
    i3 = 1.0 / d3
    return ok, (l10, l20, l30, l21, l31, l32, i0, i1, i2, i3)


def _null_max_host(prods, ant, z=None, rcond=1e-12, n=None):
    """Host reference of ``ops.fe_null_skymax``: the sky maximum of Fe for
    ``R`` noise-only realisations per (draw, frequency) column.

    ``prods`` (P, D, 5, F) (planes ss, cc, sc are read), ``ant``
    (nsky, P, 2), ``z`` (D, F, P, 2, R).  Returns ``(femax (R, D, F),
    argmax (R, D, F) int64)``, the lowest sky index on ties.

    ``n=`` (in place of ``z``, same layout) holds the data products
    ``(n_s, n_c)`` themselves, e.g. the joint null of
    ``FpEngine.null_data``: nothing is drawn from the blocks, which are
    then not checked for positive definiteness.

    Per sky point M (the moments of :func:`_assemble_fe_draws`) is
    factored ONCE, elementwise over the columns, and all R realisations
    go through the forward solve; the columns whose M fails a pivot take
    the pseudo-inverse, as in :func:`_assemble_fe_draws`.  Every step is
    elementwise in R: a realisation's value does not depend on how many
    others are computed with it."""
    prods = np.asarray(prods, dtype=np.float64)
    ant = np.asarray(ant, dtype=np.float64)
    if (z is None) == (n is None):
        raise ValueError("give either z or n")
    name = "z" if n is None else "n"
    z = np.asarray(z if n is None else n, dtype=np.float64)
    P, D, _, F = prods.shape
    if z.shape[:4] != (D, F, P, 2):
        raise ValueError(f"{name} must be (D, F, P, 2, R) = ({D}, {F}, {P}, "
                         f"2, R), got {z.shape}")
    R = z.shape[4]
    if n is None:
        ns, nc = _null_draws(prods, z)
    else:
        ns = np.moveaxis(z[:, :, :, 0, :], 2, 0)  # (P, D, F, R)
        nc = np.moveaxis(z[:, :, :, 1, :], 2, 0)
    femax = np.full((D, F, R), -np.inf)
    argmax = np.full((D, F, R), -1, dtype=np.int64)
    for k in range(ant.shape[0]):
        fplus, fcross = ant[k, :, 0], ant[k, :, 1]
        moments = _moments(prods, fplus, fcross)
        N = [_psum(fplus, ns), _psum(fplus, nc),
             _psum(fcross, ns), _psum(fcross, nc)]
        with np.errstate(all="ignore"):
            ok, fac = _ldl4(moments, rcond)
            e = [x[..., None] for x in fac]
            z0 = N[0]
            z1 = N[1] - e[0] * z0
            z2 = N[2] - e[1] * z0 - e[3] * z1
            z3 = N[3] - e[2] * z0 - e[4] * z1 - e[5] * z2
            fe = 0.5 * (z0 * z0 * e[6] + z1 * z1 * e[7] + z2 * z2 * e[8]
                        + z3 * z3 * e[9])  # (D, F, R)
        if not ok.all():
            M = _full_m(moments)
            for d, f in np.argwhere(~ok):
                Mi = np.linalg.pinv(M[d, f], rcond=rcond)
                acc = 0.0
                for i in range(4):
                    xi = sum(Mi[i, j] * N[j][d, f] for j in range(4))
                    acc = acc + N[i][d, f] * xi
                fe[d, f] = 0.5 * acc
        better = fe > femax  # strict: the first maximum stays
        femax = np.where(better, fe, femax)
        argmax = np.where(better, k, argmax)
    return np.moveaxis(femax, 2, 0), np.moveaxis(argmax, 2, 0)


class _Sky:
    """The sky layer under :class:`FastFe` and :class:`NMFe`: the antenna
    table of ``sky`` and the four sky operations on a product set
    (P, D, 5, F).  With ``hip`` (default: ``engine`` is on the HIP path)
    table and products are device tensors and the operations the
    ``ops.fe_*`` kernels, otherwise numpy arrays and the host assembly.
    Only this class makes that choice; every result is a numpy array."""

    def __init__(self, pos, sky, engine, hip=None):
        self.hip = engine._use_hip if hip is None else hip
        if self.hip and not engine._use_hip:
            raise ValueError(
                "assemble='device' needs an engine on the HIP path "
                "(force_eager engines have no HIP products)")
        self.device = engine.device
        self.ant = _antenna_table(pos, sky, self.device if self.hip else None)

    def _grid(self, prods):
        """The host assembly stacked over the sky: (nsky, D, F)."""
        return np.stack([_assemble_fe_draws(prods, a[:, 0], a[:, 1])
                         for a in self.ant])

    def map(self, prods):
        """Fe over (draw, sky, frequency): (D, nsky, F)."""
        if self.hip:
            return ops.fe_assemble(prods, self.ant).cpu().numpy()
        return np.moveaxis(self._grid(prods), 0, 1)

    def max(self, prods, amplitudes=False):
        """Fe maximised over the sky: ``(femax (D, F), argmax (D, F) int64)``,
        with ``amplitudes`` also ``amps (D, F, 4)`` at the maximum: on the
        host re-solved only at the sky rows that hold a maximum."""
        if self.hip:
            femax, argmax, _ = ops.fe_skymax(prods, self.ant)
            out = (femax.cpu().numpy(), argmax.cpu().numpy().astype(np.int64))
            if amplitudes:
                amps, _, _ = ops.fe_amplitudes(prods, self.ant, argmax)
                out += (amps.cpu().numpy(),)
            return out
        grid = self._grid(prods)
        argmax = np.nanargmax(grid, axis=0)
        out = (np.nanmax(grid, axis=0), argmax)
        if amplitudes:
            amps = np.empty(argmax.shape + (4,))
            for k in np.unique(argmax):
                sel = argmax == k
                amps[sel] = self.amplitudes(prods, k)[1][sel]
            out += (amps,)
        return out

    def amplitudes(self, prods, k=0):
        """``(fe (D, F), amps (D, F, 4))`` at sky row ``k``."""
        if self.hip:
            idx = torch.full((prods.shape[1], prods.shape[3]), int(k),
                             dtype=torch.int32, device=prods.device)
            amps, fe, _ = ops.fe_amplitudes(prods, self.ant, idx)
            return fe.cpu().numpy(), amps.cpu().numpy()
        return _assemble_fe_draws(prods, self.ant[k, :, 0], self.ant[k, :, 1],
                                  amplitudes=True)

    def null_max(self, prods, nreal, seed, real_chunk, z=None, gen=None,
                 data=None):
        """(nreal, D, F) null sky maxima of one product set, ``real_chunk``
        realisations at a time.  ``z`` (D, F, P, 2, nreal) bypasses the
        generator; otherwise each chunk is ONE ``torch.randn`` call on the
        engine's device from ``gen`` (by default a fresh one of ``seed``).
        ``data`` (D, F, P, 2, nreal), in place of ``z``, holds the data
        products ``n`` themselves (``FpEngine.null_data``)."""
        P, D, F = prods.shape[0], prods.shape[1], prods.shape[3]
        nreal, real_chunk = int(nreal), int(real_chunk)
        if nreal < 1 or real_chunk < 1:
            raise ValueError("nreal and real_chunk must be at least 1")
        if data is not None:
            if z is not None:
                raise ValueError("give z or data, not both")
            if tuple(data.shape) != (D, F, P, 2, nreal):
                raise ValueError(
                    f"data must be (D, F, P, 2, nreal) = ({D}, {F}, {P}, 2, "
                    f"{nreal}), got {tuple(data.shape)}")
            data = torch.as_tensor(data, dtype=torch.float64)
            out = np.empty((nreal, D, F))
            for lo in range(0, nreal, real_chunk):
                hi = min(lo + real_chunk, nreal)
                nc = data[..., lo:hi]
                if self.hip:
                    fm, _, _ = ops.fe_null_skymax(
                        prods, self.ant, nc.to(prods.device).contiguous(),
                        data=True)
                    out[lo:hi] = fm.cpu().numpy()
                else:
                    out[lo:hi] = _null_max_host(prods, self.ant,
                                                n=nc.cpu().numpy())[0]
            return out
        if z is not None:
            if tuple(z.shape) != (D, F, P, 2, nreal):
                raise ValueError(
                    f"z must be (D, F, P, 2, nreal) = ({D}, {F}, {P}, 2, "
                    f"{nreal}), got {tuple(z.shape)}")
            z = torch.as_tensor(z, dtype=torch.float64)
        elif gen is None:
            gen = torch.Generator(device=self.device)
            gen.manual_seed(int(seed))
        out = np.empty((nreal, D, F))
        for lo in range(0, nreal, real_chunk):
            hi = min(lo + real_chunk, nreal)
            zc = z[..., lo:hi] if z is not None else torch.randn(
                (D, F, P, 2, hi - lo), generator=gen, dtype=torch.float64,
                device=self.device)
            if self.hip:
                fm, _, _ = ops.fe_null_skymax(
                    prods, self.ant, zc.to(prods.device).contiguous())
                out[lo:hi] = fm.cpu().numpy()
            else:
                out[lo:hi] = _null_max_host(prods, self.ant,
                                            zc.cpu().numpy())[0]
        return out


    def null_max_joint(self, engine, chunks, nreal, seed, real_chunk,
                       w=None, u=None):
        """(nreal, D, F) null sky maxima drawn JOINTLY across frequencies
        (docs/DESIGN.md section 14).  ``chunks``: ``(prods, phiinvs)`` per
        draw chunk, in draw order — the products (P, Dc, 5, F) as this
        layer takes them and the per-pulsar (Dc, m) or (m,) prior rows
        they came from.

        Realisation chunks are the OUTER loop: per chunk of ``real_chunk``
        realisations one ``(w, u)`` per pulsar — ``engine.null_normals``
        on one generator of ``seed``, or the columns of the explicit
        ``w`` / ``u`` lists — and one white term serve every draw chunk
        (common random numbers across noise draws); per draw chunk only
        ``engine._null_combine`` and the sky maximum run."""
        nreal, real_chunk = int(nreal), int(real_chunk)
        if nreal < 1 or real_chunk < 1:
            raise ValueError("nreal and real_chunk must be at least 1")
        if (w is None) != (u is None):
            raise ValueError("give both w and u, or neither")
        if w is not None and any(
                x.shape[1] != nreal for x in list(w) + list(u)):
            raise ValueError(f"w and u must hold nreal = {nreal} columns")
        gen = None
        if w is None:
            gen = torch.Generator(device=engine.device)
            gen.manual_seed(int(seed))
        chunks = list(chunks)
        D = sum(prods.shape[1] for prods, _ in chunks)
        out = np.empty((nreal, D, chunks[0][0].shape[3]))
        for lo in range(0, nreal, real_chunk):
            hi = min(lo + real_chunk, nreal)
            if gen is not None:
                wc, uc = engine.null_normals(hi - lo, gen)
            else:
                wc = [torch.as_tensor(x)[:, lo:hi] for x in w]
                uc = [torch.as_tensor(x)[:, lo:hi] for x in u]
            white = engine._null_white(wc)
            d0 = 0
            for prods, phiinvs in chunks:
                n = engine._null_combine(white, phiinvs, uc)
                d1 = d0 + prods.shape[1]
                out[lo:hi, d0:d1] = self.null_max(
                    prods, hi - lo, seed, hi - lo,
                    data=n if self.hip else n.cpu())
                d0 = d1
        return out


def false_alarm_probability(femax, null):
    """False-alarm probability of observed maxima ``femax`` (...) against
    null maxima ``null`` (nreal, ...), ``(1 + #{null >= femax}) / (1 +
    nreal)`` along the first axis of ``null``: never zero, the observed
    value counts as one draw of its own null."""
    null = np.asarray(null)
    return (1.0 + (null >= np.asarray(femax)[None]).sum(axis=0)) \
        / (1.0 + null.shape[0])


def global_false_alarm(femax, null):
    """Search-wide significance of the loudest (sky, frequency) point:
    ``(femax_global, f_index, pfa_global)`` for observed sky maxima
    ``femax`` (..., F) and JOINT null sky maxima ``null`` (nreal, ..., F)
    (``null_max(joint=True)``).  Both sides are maximised over the
    frequency axis — ``f_index`` is where the observed maximum lies, the
    lowest index on ties — and ``pfa_global`` is
    :func:`false_alarm_probability` of the one against the other: ties
    count, and it is never zero.  With a null drawn independently per
    frequency the result is not a probability of anything."""
    femax = np.asarray(femax)
    null = np.asarray(null)
    if femax.ndim < 1 or null.shape[1:] != femax.shape:
        raise ValueError(f"null must be (nreal,) + femax.shape = (nreal, "
                         f"{femax.shape}), got {null.shape}")
    fg = femax.max(axis=-1)
    return fg, femax.argmax(axis=-1), \
        false_alarm_probability(fg, null.max(axis=-1))


class FastFe:
    """Fe detection statistic over (frequency, sky).

    Same construction contract as :class:`fastfp_amd.FastFp`; pulsars
    must carry ``.pos`` unit vectors (``PulsarData.pos`` — present on
    synthetic PTAs, enterprise pickles, and the npz/feather formats).
    """

    def __init__(self, psrs, pta=None):
        self.psrs = psrs
        self.pta = pta
        for p in psrs:
            if getattr(p, "pos", None) is None:
                raise ValueError(
                    f"pulsar {p.name} has no sky position (.pos); the "
                    "sky-coherent Fe statistic requires one"
                )
        self.pos = np.stack([np.asarray(p.pos, dtype=np.float64)
                             for p in psrs])
        self.toas = [np.asarray(p.toas, dtype=np.float64) for p in psrs]
        self.residuals = [np.asarray(p.residuals, dtype=np.float64)
                          for p in psrs]

    # ------------------------------------------------------------------
    # parity-style path: one (frequency, sky) point via get_xCy
    # ------------------------------------------------------------------
    def calculate_Fe(self, fgw, gwtheta, gwphi, Nvecs, Ts, sigmas) -> float:
        """Single-point Fe through explicit Woodbury products (the slow,
        obviously-correct path; ``sweep`` reuses the engine)."""
        fplus, fcross = gw_antenna_pattern(self.pos, gwtheta, gwphi)
        prods = np.empty((len(self.psrs), 5, 1))
        for i, (Nvec, T, sigma, toa, resid) in enumerate(
            zip(Nvecs, Ts, sigmas, self.toas, self.residuals)
        ):
            arg = 2.0 * math.pi * fgw * toa
            s, c = np.sin(arg), np.cos(arg)
            prods[i, 0, 0] = get_xCy(Nvec, T, sigma, s, s)
            prods[i, 1, 0] = get_xCy(Nvec, T, sigma, c, c)
            prods[i, 2, 0] = get_xCy(Nvec, T, sigma, s, c)
            prods[i, 3, 0] = get_xCy(Nvec, T, sigma, s, resid)
            prods[i, 4, 0] = get_xCy(Nvec, T, sigma, c, resid)
        return float(_assemble_fe(prods, fplus, fcross)[0])

    # ------------------------------------------------------------------
    # production path: whole (sky x freq) grid from one engine pass
    # ------------------------------------------------------------------
    @staticmethod
    def _products(engine, sigmas, hip):
        """The fixed-noise products as the one-draw set (P, 1, 5, F): a
        device tensor from the HIP solve (``hip``), otherwise a numpy
        array from the torch path on the dense ``sigmas``."""
        if hip:
            return engine.sweep_products_hip(
                _phiinvs_from_sigmas(engine, sigmas))[:, None].contiguous()
        return engine.sweep_products(sigmas=sigmas).cpu().numpy()[:, None]

    def _setup(self, freqs, sky, Nvecs, Ts, sigmas, device, engine,
               freq_chunk=2048, hip=None):
        """``(layer, prods)``: the sky layer of ``sky`` on the caller's
        engine (or one built here) and the products it takes."""
        engine = _obtain_engine(engine, self.psrs, freqs, Nvecs, Ts, device,
                                freq_chunk)
        layer = _Sky(self.pos, sky, engine, hip)
        return layer, self._products(engine, sigmas, layer.hip)

    def sweep(self, freqs, sky, Nvecs, Ts, sigmas, device: str = None,
              freq_chunk: int = 2048, engine: FpEngine = None,
              assemble: str = "host") -> np.ndarray:
        """Fe over ``freqs`` x ``sky`` (list of (gwtheta, gwphi)).

        Returns (nsky, F).  The per-pulsar corrected products are
        computed once on the engine (GPU precompute kernels + one
        m-dim solve per pulsar); each sky point is then an O(P) 4x4
        assembly per frequency.

        ``assemble="device"`` (HIP engines only) takes the products
        from the HIP solve and runs the sky assembly in the
        ``fe_assemble`` kernel; the default ``"host"`` is the numpy
        assembly.
        """
        device = _check_assemble(assemble, device, engine)
        layer, prods = self._setup(freqs, sky, Nvecs, Ts, sigmas, device,
                                   engine, freq_chunk, assemble == "device")
        return layer.map(prods)[0]

    def sweep_max(self, freqs, sky, Nvecs, Ts, sigmas, device: str = None,
                  engine: FpEngine = None, amplitudes: bool = False):
        """Fe maximised over ``sky`` per frequency.

        Returns ``(femax (F,), argmax (F,))``; ``argmax`` indexes into
        ``sky``.  On a HIP engine the products come from the HIP solve
        and the ``fe_skymax`` kernel keeps the running maximum, so only
        (F,)-sized results leave the device; on a CPU engine this is the
        host assembly followed by the NaN-ignoring maximum over the sky
        (the reference implementation).

        ``amplitudes``: return ``(femax, argmax, amps (F, 4))`` with the
        maximum-likelihood amplitudes ``M^-1 N`` at the maximum
        (:func:`cw_parameters` turns them into source parameters).  On a
        HIP engine the ``fe_amplitudes`` kernel reads the same device
        products at ``argmax``; on a CPU engine it is the host solve.
        """
        layer, prods = self._setup(freqs, sky, Nvecs, Ts, sigmas, device,
                                   engine)
        return tuple(x[0] for x in layer.max(prods, amplitudes))

    def amplitudes(self, freqs, gwtheta, gwphi, Nvecs, Ts, sigmas,
                   device: str = None, engine: FpEngine = None):
        """Targeted search at one sky position: ``(fe (F,), amps (F,
        4))``, the statistic and the maximum-likelihood amplitudes
        ``M^-1 N`` per frequency.  HIP engine: products from the HIP
        solve, ``fe_amplitudes`` kernel; CPU engine: the host solve."""
        layer, prods = self._setup(freqs, [(float(gwtheta), float(gwphi))],
                                   Nvecs, Ts, sigmas, device, engine)
        fe, amps = layer.amplitudes(prods)
        return fe[0], amps[0]

    # ------------------------------------------------------------------
    # significance of the sky maximum
    # ------------------------------------------------------------------
    def null_max(self, freqs, sky, Nvecs, Ts, sigmas, nreal: int,
                 seed: int = 0, device: str = None, engine: FpEngine = None,
                 real_chunk: int = 256, z=None, joint: bool = False,
                 w=None, u=None) -> np.ndarray:
        """The sky-maximised Fe of ``nreal`` noise-only realisations per
        frequency: ``(nreal, F)``, the Monte-Carlo null distribution of
        what :meth:`sweep_max` returns.

        No solve runs per realisation.  For residuals ``r ~ N(0, C)`` the
        data products of pulsar ``p`` are exactly ``(sr, cr)_p ~ N(0,
        [[ss, sc], [sc, cc]]_p)``, so a realisation is one standard-normal
        pair per pulsar and frequency and a sky assembly in which only
        the four ``N`` sums are new.  On a HIP engine the products come
        from ``sweep_products_hip`` and ``ops.fe_null_skymax`` runs per
        chunk of ``real_chunk`` realisations; on a CPU engine it is
        :func:`_null_max_host`.

        ``z`` is drawn on the engine's device by a ``torch.Generator``
        seeded with ``seed``, one ``torch.randn`` call of shape (1, F, P,
        2, chunk) per chunk: the stream, and so the result, is
        reproducible for a given ``(seed, real_chunk, device type)`` and
        is NOT the same on the CPU and on the GPU.  ``z=`` takes explicit
        normals of shape (1, F, P, 2, nreal) and bypasses the generator
        (the result then does not depend on ``real_chunk``).

        Scope.  The null is exact per frequency.  By default realisations
        are drawn independently per frequency, so the joint distribution
        across frequencies is not modelled.  ``joint=True`` draws ONE
        noise realisation per pulsar for all frequencies
        (``FpEngine.null_data``, docs/DESIGN.md section 14; diagonal white
        noise only): row ``r`` of the result is then one noise-only data
        set seen at every frequency, which is what
        :func:`global_false_alarm` needs.  Its normals come from one
        generator of ``seed`` per ``real_chunk`` (reproducible per
        ``(seed, real_chunk, device type)``), or from the explicit lists
        ``w`` ((ntoa_p, nreal) each) and ``u`` ((m_p, nreal) each).  A
        signal-present mean for detection-probability curves is out of
        scope.
        """
        if joint:
            if z is not None:
                raise ValueError("joint=True takes w= and u=, not z=")
            engine = _obtain_engine(engine, self.psrs, freqs, Nvecs, Ts,
                                    device)
        elif w is not None or u is not None:
            raise ValueError("w= and u= need joint=True")
        layer, prods = self._setup(freqs, sky, Nvecs, Ts, sigmas, device,
                                   engine)
        return self._null(layer, prods, engine, sigmas, nreal, seed,
                          real_chunk, z, joint, w, u)

    @staticmethod
    def _null(layer, prods, engine, sigmas, nreal, seed, real_chunk, z,
              joint, w, u):
        """(nreal, F) null maxima of the one-draw product set ``prods``."""
        if not joint:
            return layer.null_max(prods, nreal, seed, real_chunk, z)[:, 0, :]
        chunk = (prods, _phiinvs_from_sigmas(engine, sigmas, improper=True))
        return layer.null_max_joint(engine, [chunk], nreal, seed, real_chunk,
                                    w, u)[:, 0, :]

    def false_alarm(self, freqs, sky, Nvecs, Ts, sigmas, nreal: int,
                    seed: int = 0, device: str = None, engine: FpEngine = None,
                    real_chunk: int = 256, z=None, joint: bool = False,
                    w=None, u=None):
        """The observed sky maximum and its false-alarm probability:
        ``(femax (F,), argmax (F,), pfa (F,))`` with ``femax, argmax`` as
        :meth:`sweep_max` returns them and

            pfa = (1 + #{null >= femax}) / (1 + nreal)

        per frequency against the ``nreal`` realisations of
        :meth:`null_max` (same arguments, same stream, same scope: a
        single-frequency probability, no trials factor over frequency).
        The products and the antenna table are computed once and serve
        both passes.

        ``joint=True``: the null is drawn jointly across frequencies
        (:meth:`null_max`), ``pfa`` comes from those realisations, and the
        result grows to ``(femax, argmax, pfa, femax_global, fglobal,
        pfa_global)``: the loudest observed maximum over the grid, its
        frequency index, and the probability that noise alone makes ANY
        frequency that loud (:func:`global_false_alarm`)."""
        if joint:
            if z is not None:
                raise ValueError("joint=True takes w= and u=, not z=")
            engine = _obtain_engine(engine, self.psrs, freqs, Nvecs, Ts,
                                    device)
        elif w is not None or u is not None:
            raise ValueError("w= and u= need joint=True")
        layer, prods = self._setup(freqs, sky, Nvecs, Ts, sigmas, device,
                                   engine)
        femax, argmax = (x[0] for x in layer.max(prods))
        null = self._null(layer, prods, engine, sigmas, nreal, seed,
                          real_chunk, z, joint, w, u)
        out = (femax, argmax, false_alarm_probability(femax, null))
        return out + global_false_alarm(femax, null) if joint else out


def compute_Fe(psrs, pta, noise, freqs, sky, device=None) -> np.ndarray:
    """One-call convenience: precompute mats and sweep the grid."""
    from fastfp_amd.model import get_mats_fp

    Nvecs, Ts, sigmas = get_mats_fp(pta, noise)
    return FastFe(psrs, pta).sweep(freqs, sky, Nvecs, Ts, sigmas,
                                   device=device)


class NMFe:
    """Noise-marginalized Fe: the Fe statistic evaluated across MCMC
    red-noise draws, symmetric to :class:`fastfp_amd.NMFp` for the
    sky-coherent statistic (no reference counterpart — the reference
    has neither Fe nor its marginalized form).

    ``rn_sigs``: the per-pulsar phi containers (``pta.rn_containers``).
    """

    def __init__(self, psrs, rn_sigs):
        self.psrs = psrs
        self.rn_sigs = rn_sigs
        self.fe = FastFe(psrs)  # validates .pos, holds antenna inputs

    def _layer(self, freqs, sky, samples, Nvecs, Ts, device, engine, compress,
               freq_chunk=2048, hip=None):
        """``(engine, layer)``: the caller's engine, or one built here (with
        draw compression when ``compress``), and the sky layer on it."""
        engine = _obtain_engine(
            engine, self.psrs, freqs, Nvecs, Ts, device, freq_chunk,
            (self.rn_sigs, samples) if compress else None)
        return engine, _Sky(self.fe.pos, sky, engine, hip)

    @staticmethod
    def _products(engine, chunk, compress: bool, hip: bool):
        """(P, Dc, 5, F) products of one draw chunk, on the HIP solve
        (``hip``) or the eager one.  With ``compress``, the per-draw
        guard of ``NMFp.sweep`` (``FpEngine.margin_split``): draws whose
        compression margin reaches the guard go through the compressed
        systems, the (rare) prior-corner draws through the exact direct
        ones, and the rows are scattered back in order."""
        if hip:
            run = engine.sweep_products_hip
        else:
            def run(p, **kw):
                return engine.sweep_products(phiinvs=p, **kw)
        if not (compress and any(b.comp is not None for b in engine.blocks)):
            return run(chunk)
        # one copy to the engine's device serves the margin and the solve
        chunk = [p.to(engine.device) for p in chunk]
        return engine.margin_split(
            chunk, lambda rows: run(rows, compressed=True), run, dim=1)

    def _draw_chunks(self, engine, samples, draw_chunk, compress, hip):
        """The products of ``samples``, ``draw_chunk`` draws at a time and
        in draw order, as the sky layer takes them: (P, Dc, 5, F) device
        tensors (``hip``) or numpy arrays."""
        phiinvs = batch_phiinv(self.rn_sigs, samples)
        phiinvs = [p[None, :] if p.dim() == 1 else p for p in phiinvs]
        for lo in range(0, phiinvs[0].shape[0], draw_chunk):
            chunk = [p[lo:lo + draw_chunk] for p in phiinvs]
            prods = self._products(engine, chunk, compress, hip)
            yield prods if hip else prods.cpu().numpy()

    def sweep(self, freqs, sky, samples: dict, Nvecs, Ts, device: str = None,
              draw_chunk: int = 128, freq_chunk: int = 2048,
              engine: FpEngine = None, assemble: str = "host",
              compress: bool = False) -> np.ndarray:
        """Fe over (draws x sky x freqs).  ``samples``: parameter-name
        -> (D,) arrays (the ``map_params`` format).  Returns
        (D, nsky, F).

        ``assemble="device"`` (HIP engines only): products from the HIP
        solve, sky assembly in the ``fe_assemble`` kernel; only the
        finished map is copied to the host.  The default ``"host"`` is
        the numpy assembly.

        ``compress``: take the products from the Schur-compressed
        per-draw systems (``NMFp.sweep``'s ``compress``), draw by draw
        where the compression margin allows.  An engine built here gets
        compression enabled; a caller's engine is used as it is."""
        device = _check_assemble(assemble, device, engine)
        engine, layer = self._layer(freqs, sky, samples, Nvecs, Ts, device,
                                    engine, compress, freq_chunk,
                                    assemble == "device")
        return np.concatenate([
            layer.map(prods) for prods in self._draw_chunks(
                engine, samples, draw_chunk, compress, layer.hip)])

    def sweep_max(self, freqs, sky, samples: dict, Nvecs, Ts,
                  device: str = None, draw_chunk: int = 128,
                  engine: FpEngine = None, compress: bool = False,
                  amplitudes: bool = False):
        """Fe maximised over ``sky`` for every (draw, frequency).

        Returns ``(femax (D, F), argmax (D, F))``; ``argmax`` indexes
        into ``sky``.  The (D, nsky, F) cube is never formed: on a HIP
        engine each draw chunk goes products (HIP solve) ->
        ``fe_skymax`` kernel and only (Dc, F)-sized results leave the
        device; on a CPU engine each chunk is assembled on the host and
        reduced with the NaN-ignoring maximum over the sky (the reference
        implementation).  ``compress``: as in :meth:`sweep`.

        ``amplitudes``: return ``(femax, argmax, amps (D, F, 4))`` with
        the maximum-likelihood amplitudes at each maximum, as in
        :meth:`FastFe.sweep_max`.
        """
        engine, layer = self._layer(freqs, sky, samples, Nvecs, Ts, device,
                                    engine, compress)
        parts = [layer.max(prods, amplitudes) for prods in self._draw_chunks(
            engine, samples, draw_chunk, compress, layer.hip)]
        return tuple(np.concatenate(col) for col in zip(*parts))

    def null_max(self, freqs, sky, samples: dict, Nvecs, Ts, nreal: int,
                 seed: int = 0, draw_chunk: int = 8, real_chunk: int = 128,
                 engine: FpEngine = None, compress: bool = False,
                 device: str = None, joint: bool = False, w=None,
                 u=None) -> np.ndarray:
        """:meth:`FastFe.null_max` over noise draws: ``(nreal, D, F)``,
        the sky-maximised Fe of ``nreal`` noise-only realisations for
        every (draw, frequency), each draw's realisations drawn from that
        draw's own products (``_products``; ``compress`` as in
        :meth:`sweep`).

        One generator seeded with ``seed`` serves all chunks, draw chunks
        outermost: the stream is reproducible for a given ``(seed,
        draw_chunk, real_chunk, device type)``.  On a HIP engine a chunk
        holds the M factors of ``draw_chunk * F * nsky`` points (80 bytes
        each) and ``draw_chunk * F * P * 2 * real_chunk`` normals, which
        is what the two chunk sizes bound.  Scope as in
        :meth:`FastFe.null_max`.

        ``joint=True``: realisations are drawn jointly across frequencies
        as in :meth:`FastFe.null_max` (``w`` / ``u`` likewise).  The
        products of all draw chunks are kept (5 F doubles per pulsar and
        draw) and the realisation chunks become the outer loop, so one
        ``(w, u)`` and one white term per realisation chunk serve EVERY
        noise draw: common random numbers across draws — realisation
        ``r`` is the same white and basis normals coloured by each draw's
        prior, which removes Monte-Carlo scatter from draw-to-draw
        comparisons and leaves each draw's own null exact.  The data
        always go through the direct system (``compress`` only chooses
        where the products come from).  The stream is reproducible per
        ``(seed, real_chunk, device type)`` and does not depend on
        ``draw_chunk``."""
        engine, layer = self._layer(freqs, sky, samples, Nvecs, Ts, device,
                                    engine, compress)
        if joint:
            phiinvs = batch_phiinv(self.rn_sigs, samples)
            phiinvs = [p[None, :] if p.dim() == 1 else p for p in phiinvs]
            rows = [[p[lo:lo + draw_chunk] for p in phiinvs]
                    for lo in range(0, phiinvs[0].shape[0], draw_chunk)]
            prods = self._draw_chunks(engine, samples, draw_chunk, compress,
                                      layer.hip)
            return layer.null_max_joint(engine, zip(prods, rows), nreal, seed,
                                        real_chunk, w, u)
        if w is not None or u is not None:
            raise ValueError("w= and u= need joint=True")
        gen = torch.Generator(device=engine.device)
        gen.manual_seed(int(seed))
        return np.concatenate([
            layer.null_max(prods, nreal, seed, real_chunk, gen=gen)
            for prods in self._draw_chunks(engine, samples, draw_chunk,
                                           compress, layer.hip)], axis=1)
