"""Earth-term Fe-statistic: sky-coherent continuous-wave detection.

The reference lists this as an open to-do (``/root/reference/README.md:23``
"Include Fe-statistic?") and never implemented it; this module completes
that roadmap natively.  Where Fp maximizes a per-pulsar 2-amplitude
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
products from the torch path and solves the 4x4 systems in numpy.  On a
HIP engine ``assemble="device"`` and ``sweep_max`` take the products
from the HIP solve (``FpEngine.sweep_products_hip``) and run the sky
assembly in the MFMA kernels ``ops.fe_assemble`` / ``ops.fe_skymax``;
``sweep_max`` returns the statistic maximised over the sky with its
argmax and never forms the (draws x sky x freqs) cube.

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
section 13).
"""

from __future__ import annotations

import math

import numpy as np
import torch

from fastfp_amd.engine import FpEngine, _t64
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


def _assemble_fe(prods, fplus, fcross, rcond=1e-12, amplitudes=False):
    """Fe(f) from per-pulsar corrected products.

    ``prods``: (P, 5, F) array of [ss, cc, sc, sr, cr]; ``fplus`` /
    ``fcross``: (P,) antenna coefficients.  Returns (F,), or with
    ``amplitudes`` the pair ``(fe (F,), a (F, 4))`` with the
    maximum-likelihood amplitudes ``a = M^-1 N``.

    M is assembled per frequency from sums over pulsars and solved as
    a 4x4 system; near-degenerate skies (e.g. all pulsars clustered:
    F+/Fx columns collinear) go through the pseudo-inverse — the
    maximized likelihood is well-defined on the column space.
    """
    ss, cc, sc = prods[:, 0, :], prods[:, 1, :], prods[:, 2, :]
    sr, cr = prods[:, 3, :], prods[:, 4, :]
    fp2 = fplus**2
    fx2 = fcross**2
    fpx = fplus * fcross

    def w(coeff, q):  # sum_p coeff_p * q_p(f)  -> (F,)
        return np.einsum("p,pf->f", coeff, q)

    F = prods.shape[2]
    M = np.empty((F, 4, 4))
    M[:, 0, 0] = w(fp2, ss)
    M[:, 0, 1] = M[:, 1, 0] = w(fp2, sc)
    M[:, 0, 2] = M[:, 2, 0] = w(fpx, ss)
    M[:, 0, 3] = M[:, 3, 0] = w(fpx, sc)
    M[:, 1, 1] = w(fp2, cc)
    M[:, 1, 2] = M[:, 2, 1] = w(fpx, sc)
    M[:, 1, 3] = M[:, 3, 1] = w(fpx, cc)
    M[:, 2, 2] = w(fx2, ss)
    M[:, 2, 3] = M[:, 3, 2] = w(fx2, sc)
    M[:, 3, 3] = w(fx2, cc)
    N = np.stack(
        [w(fplus, sr), w(fplus, cr), w(fcross, sr), w(fcross, cr)], axis=1
    )  # (F, 4)
    x = _solve4(M, N, rcond)
    fe = 0.5 * np.einsum("fi,fi->f", N, x)
    return (fe, x) if amplitudes else fe


def _check_assemble(assemble, device, engine):
    """Validate the ``assemble=`` keyword and resolve the default
    device.  ``"device"`` needs a HIP engine: a CPU device (or a CPU
    engine) is rejected before any precompute runs."""
    if assemble not in ("host", "device"):
        raise ValueError(
            f"assemble must be 'host' or 'device', got {assemble!r}")
    if device is None:
        device = "cuda" if torch.cuda.is_available() else "cpu"
    if assemble == "device":
        dev = engine.device if engine is not None else torch.device(device)
        if dev.type != "cuda":
            raise ValueError(
                "assemble='device' runs the sky assembly in the HIP "
                f"kernels and needs a GPU engine (got device {dev}); use "
                "assemble='host' on the CPU")
    return device


def _require_hip_engine(engine):
    if not engine._use_hip:
        raise ValueError(
            "assemble='device' needs an engine on the HIP path "
            "(force_eager engines have no HIP products)")


def _phiinvs_from_sigmas(engine, sigmas):
    """Fixed-noise (m, m) sigmas -> per-pulsar diagonal phi^-1 (the
    ``get_mats_fp`` contract sigma = TNT + diag(phi^-1), as in
    ``FpEngine.sweep``)."""
    out = []
    for blk, sg in zip(engine.blocks, sigmas):
        sg = _t64(sg, engine.device)
        out.append((torch.diagonal(sg) - torch.diagonal(blk.TNT)).contiguous())
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


def _host_max_amplitudes(assemble, prods, coeffs):
    """Host reference of the sky maximum with amplitudes.  ``assemble``
    is ``_assemble_fe`` or ``_assemble_fe_draws``, ``coeffs`` the (F+,
    Fx) pair of every sky point.  Returns ``(femax, argmax, amps)`` of
    the assembly's output shape (+ (4,) for ``amps``); the solve is
    repeated with amplitudes only at the sky points that hold a
    maximum."""
    grid = np.stack([assemble(prods, fplus, fcross)
                     for fplus, fcross in coeffs])  # (nsky, ...)
    femax = np.nanmax(grid, axis=0)
    argmax = np.nanargmax(grid, axis=0)
    amps = np.empty(argmax.shape + (4,))
    for k in np.unique(argmax):
        _, a = assemble(prods, *coeffs[k], amplitudes=True)
        sel = argmax == k
        amps[sel] = a[sel]
    return femax, argmax, amps


_NOT_PD = ("the product block [[ss, sc], [sc, cc]] of (pulsar {p}, draw {d}, "
           "frequency {f}) is not positive definite: it is no covariance to "
           "draw noise-only products from")


def _null_factors(prods):
    """Cholesky factors ``(l00, l10, l11)``, each (P, D, F), of the
    per-pulsar blocks ``B_p = [[ss, sc], [sc, cc]]`` of ``prods``
    (P, D, 5, F).  Raises ``ValueError`` naming the first (pulsar, draw,
    frequency) whose block is not positive definite (``ss <= 0``, a Schur
    complement ``<= 0`` or a non-finite value)."""
    ss, cc, sc = prods[:, :, 0], prods[:, :, 1], prods[:, :, 2]
    with np.errstate(all="ignore"):
        l00 = np.sqrt(ss)
        l10 = sc / l00
        schur = cc - l10 * l10
        l11 = np.sqrt(schur)
    ok = (np.isfinite(ss) & np.isfinite(cc) & np.isfinite(sc)
          & np.isfinite(l10) & np.isfinite(schur) & (ss > 0) & (schur > 0))
    if not ok.all():
        p, d, f = (int(i) for i in np.argwhere(~ok)[0])
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


def _null_max_host(prods, ant, z, rcond=1e-12):
    """Host reference of ``ops.fe_null_skymax``: the sky maximum of Fe for
    ``R`` noise-only realisations per (draw, frequency) column.

    ``prods`` (P, D, 5, F) (planes ss, cc, sc are read), ``ant``
    (nsky, P, 2), ``z`` (D, F, P, 2, R).  Returns ``(femax (R, D, F),
    argmax (R, D, F) int64)``, the lowest sky index on ties.

    Per sky point M is factored ONCE (the LDL^T and pivot rule of the
    kernels, elementwise over the columns) and all R realisations go
    through the forward solve; the columns whose M fails a pivot take the
    pseudo-inverse, as in :func:`_assemble_fe_draws`.  Every step is
    elementwise in R: a realisation's value does not depend on how many
    others are computed with it."""
    prods = np.asarray(prods, dtype=np.float64)
    ant = np.asarray(ant, dtype=np.float64)
    z = np.asarray(z, dtype=np.float64)
    P, D, _, F = prods.shape
    if z.shape[:4] != (D, F, P, 2):
        raise ValueError(f"z must be (D, F, P, 2, R) = ({D}, {F}, {P}, 2, R),"
                         f" got {z.shape}")
    R = z.shape[4]
    ns, nc = _null_draws(prods, z)
    ss, cc, sc = prods[:, :, 0], prods[:, :, 1], prods[:, :, 2]
    femax = np.full((D, F, R), -np.inf)
    argmax = np.full((D, F, R), -1, dtype=np.int64)

    def w(coeff, q):  # (P,) x (P, D, F[, R]) -> (D, F[, R])
        return np.einsum("p,p...->...", coeff, q)

    for k in range(ant.shape[0]):
        fplus, fcross = ant[k, :, 0], ant[k, :, 1]
        fp2, fx2, fpx = fplus**2, fcross**2, fplus * fcross
        m00, m01, m11 = w(fp2, ss), w(fp2, sc), w(fp2, cc)
        m02, m03, m13 = w(fpx, ss), w(fpx, sc), w(fpx, cc)
        m22, m23, m33 = w(fx2, ss), w(fx2, sc), w(fx2, cc)
        m12 = m03
        N = [w(fplus, ns), w(fplus, nc), w(fcross, ns), w(fcross, nc)]

        def pivot_ok(s, mjj):
            return (s > rcond * mjj) & (s < np.inf)

        with np.errstate(all="ignore"):
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
            e = [x[..., None] for x in
                 (l10, l20, l30, l21, l31, l32, i0, i1, i2, i3)]
            z0 = N[0]
            z1 = N[1] - e[0] * z0
            z2 = N[2] - e[1] * z0 - e[3] * z1
            z3 = N[3] - e[2] * z0 - e[4] * z1 - e[5] * z2
            fe = 0.5 * (z0 * z0 * e[6] + z1 * z1 * e[7] + z2 * z2 * e[8]
                        + z3 * z3 * e[9])  # (D, F, R)
        if not ok.all():
            M = np.empty((D, F, 4, 4))
            M[..., 0, 0] = m00
            M[..., 0, 1] = M[..., 1, 0] = m01
            M[..., 0, 2] = M[..., 2, 0] = m02
            M[..., 0, 3] = M[..., 3, 0] = m03
            M[..., 1, 1] = m11
            M[..., 1, 2] = M[..., 2, 1] = m12
            M[..., 1, 3] = M[..., 3, 1] = m13
            M[..., 2, 2] = m22
            M[..., 2, 3] = M[..., 3, 2] = m23
            M[..., 3, 3] = m33
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


def _null_chunks(prods, ant, nreal, seed, real_chunk, z, device, hip,
                 gen=None):
    """(nreal, D, F) null sky maxima of one product set, ``real_chunk``
    realisations at a time.  ``prods`` / ``ant``: device tensors (``hip``)
    or numpy arrays.  ``z`` (D, F, P, 2, nreal) bypasses the generator;
    otherwise each chunk is ONE ``torch.randn`` call on ``device`` from
    ``gen`` (a fresh generator seeded with ``seed`` when none is
    passed)."""
    P, D, F = prods.shape[0], prods.shape[1], prods.shape[3]
    nreal, real_chunk = int(nreal), int(real_chunk)
    if nreal < 1 or real_chunk < 1:
        raise ValueError("nreal and real_chunk must be at least 1")
    if z is not None:
        if tuple(z.shape) != (D, F, P, 2, nreal):
            raise ValueError(
                f"z must be (D, F, P, 2, nreal) = ({D}, {F}, {P}, 2, "
                f"{nreal}), got {tuple(z.shape)}")
        z = torch.as_tensor(z, dtype=torch.float64)
    elif gen is None:
        gen = torch.Generator(device=device)
        gen.manual_seed(int(seed))
    out = np.empty((nreal, D, F))
    for lo in range(0, nreal, real_chunk):
        hi = min(lo + real_chunk, nreal)
        if z is None:
            zc = torch.randn((D, F, P, 2, hi - lo), generator=gen,
                             dtype=torch.float64, device=device)
        else:
            zc = z[..., lo:hi]
        if hip:
            from fastfp_amd import ops

            fm, _, _ = ops.fe_null_skymax(
                prods, ant, zc.to(prods.device).contiguous())
            out[lo:hi] = fm.cpu().numpy()
        else:
            out[lo:hi] = _null_max_host(prods, ant, zc.cpu().numpy())[0]
    return out


def false_alarm_probability(femax, null):
    """False-alarm probability of observed maxima ``femax`` (...) against
    null maxima ``null`` (nreal, ...), ``(1 + #{null >= femax}) / (1 +
    nreal)`` along the first axis of ``null``: never zero, the observed
    value counts as one draw of its own null."""
    null = np.asarray(null)
    return (1.0 + (null >= np.asarray(femax)[None]).sum(axis=0)) \
        / (1.0 + null.shape[0])


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
    def sweep(
        self,
        freqs,
        sky,
        Nvecs,
        Ts,
        sigmas,
        device: str = None,
        freq_chunk: int = 2048,
        engine: FpEngine = None,
        assemble: str = "host",
    ) -> np.ndarray:
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
        if engine is None:
            engine = FpEngine(self.psrs, Nvecs, Ts, device=device)
            engine.precompute(freqs, freq_chunk=freq_chunk)
        if assemble == "device":
            from fastfp_amd import ops

            _require_hip_engine(engine)
            prods = engine.sweep_products_hip(
                _phiinvs_from_sigmas(engine, sigmas))  # (P, 5, F)
            fe = ops.fe_assemble(prods[:, None].contiguous(),
                                 _antenna_table(self.pos, sky, engine.device))
            return fe[0].cpu().numpy()
        prods = engine.sweep_products(sigmas=sigmas)  # (P, 5, F) tensor
        prods = prods.cpu().numpy()
        out = np.empty((len(sky), prods.shape[2]))
        for k, (gwtheta, gwphi) in enumerate(sky):
            fplus, fcross = gw_antenna_pattern(self.pos, gwtheta, gwphi)
            out[k] = _assemble_fe(prods, fplus, fcross)
        return out

    def sweep_max(
        self,
        freqs,
        sky,
        Nvecs,
        Ts,
        sigmas,
        device: str = None,
        engine: FpEngine = None,
        amplitudes: bool = False,
    ):
        """Fe maximised over ``sky`` per frequency.

        Returns ``(femax (F,), argmax (F,))``; ``argmax`` indexes into
        ``sky``.  On a HIP engine the products come from the HIP solve
        and the ``fe_skymax`` kernel keeps the running maximum, so only
        (F,)-sized results leave the device; on a CPU engine this is the
        host assembly followed by ``np.nanmax`` / ``np.nanargmax`` (the
        reference implementation).

        ``amplitudes``: return ``(femax, argmax, amps (F, 4))`` with the
        maximum-likelihood amplitudes ``M^-1 N`` at the maximum
        (:func:`cw_parameters` turns them into source parameters).  On a
        HIP engine the ``fe_amplitudes`` kernel reads the same device
        products at ``argmax``; on a CPU engine it is the host solve.
        """
        if device is None:
            device = "cuda" if torch.cuda.is_available() else "cpu"
        if engine is None:
            engine = FpEngine(self.psrs, Nvecs, Ts, device=device)
            engine.precompute(freqs)
        if engine._use_hip:
            from fastfp_amd import ops

            prods = engine.sweep_products_hip(
                _phiinvs_from_sigmas(engine, sigmas))  # (P, 5, F)
            prods = prods[:, None].contiguous()
            ant_d = _antenna_table(self.pos, sky, engine.device)
            femax, argmax, _ = ops.fe_skymax(prods, ant_d)
            out = (femax[0].cpu().numpy(),
                   argmax[0].cpu().numpy().astype(np.int64))
            if amplitudes:
                amps, _, _ = ops.fe_amplitudes(prods, ant_d, argmax)
                out += (amps[0].cpu().numpy(),)
            return out
        if amplitudes:
            # the assembly of ``sweep``, call for call
            prods = engine.sweep_products(sigmas=sigmas).cpu().numpy()
            return _host_max_amplitudes(
                _assemble_fe, prods,
                [gw_antenna_pattern(self.pos, th, ph) for th, ph in sky])
        grid = self.sweep(freqs, sky, Nvecs, Ts, sigmas, engine=engine)
        return np.nanmax(grid, axis=0), np.nanargmax(grid, axis=0)

    def amplitudes(
        self,
        freqs,
        gwtheta,
        gwphi,
        Nvecs,
        Ts,
        sigmas,
        device: str = None,
        engine: FpEngine = None,
    ):
        """Targeted search at one sky position: ``(fe (F,), amps (F,
        4))``, the statistic and the maximum-likelihood amplitudes
        ``M^-1 N`` per frequency.  HIP engine: products from the HIP
        solve, ``fe_amplitudes`` kernel; CPU engine: the host solve."""
        if device is None:
            device = "cuda" if torch.cuda.is_available() else "cpu"
        if engine is None:
            engine = FpEngine(self.psrs, Nvecs, Ts, device=device)
            engine.precompute(freqs)
        sky = [(float(gwtheta), float(gwphi))]
        if engine._use_hip:
            from fastfp_amd import ops

            prods = engine.sweep_products_hip(
                _phiinvs_from_sigmas(engine, sigmas))  # (P, 5, F)
            prods = prods[:, None].contiguous()
            idx = torch.zeros((1, prods.shape[3]), dtype=torch.int32,
                              device=prods.device)
            amps, fe, _ = ops.fe_amplitudes(
                prods, _antenna_table(self.pos, sky, engine.device), idx)
            return fe[0].cpu().numpy(), amps[0].cpu().numpy()
        prods = engine.sweep_products(sigmas=sigmas).cpu().numpy()
        fplus, fcross = gw_antenna_pattern(self.pos, *sky[0])
        return _assemble_fe(prods, fplus, fcross, amplitudes=True)

    # ------------------------------------------------------------------
    # significance of the sky maximum
    # ------------------------------------------------------------------
    def _null_inputs(self, freqs, sky, Nvecs, Ts, sigmas, device, engine):
        """``(engine, prods (P, 1, 5, F), ant (nsky, P, 2))``: device
        tensors from the HIP solve on a HIP engine, numpy arrays
        otherwise."""
        if device is None:
            device = "cuda" if torch.cuda.is_available() else "cpu"
        if engine is None:
            engine = FpEngine(self.psrs, Nvecs, Ts, device=device)
            engine.precompute(freqs)
        if engine._use_hip:
            prods = engine.sweep_products_hip(
                _phiinvs_from_sigmas(engine, sigmas))  # (P, 5, F)
            return (engine, prods[:, None].contiguous(),
                    _antenna_table(self.pos, sky, engine.device))
        prods = engine.sweep_products(sigmas=sigmas).cpu().numpy()
        return engine, prods[:, None], _antenna_table(self.pos, sky)

    def null_max(
        self,
        freqs,
        sky,
        Nvecs,
        Ts,
        sigmas,
        nreal: int,
        seed: int = 0,
        device: str = None,
        engine: FpEngine = None,
        real_chunk: int = 256,
        z=None,
    ) -> np.ndarray:
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

        Scope.  The null is exact per frequency.  Realisations are drawn
        independently per frequency, so the joint distribution across
        frequencies is not modelled and a trials factor over frequency is
        out of scope; so is a signal-present mean for detection-
        probability curves.
        """
        engine, prods, ant = self._null_inputs(freqs, sky, Nvecs, Ts, sigmas,
                                               device, engine)
        return _null_chunks(prods, ant, nreal, seed, real_chunk, z,
                            engine.device, engine._use_hip)[:, 0, :]

    def false_alarm(
        self,
        freqs,
        sky,
        Nvecs,
        Ts,
        sigmas,
        nreal: int,
        seed: int = 0,
        device: str = None,
        engine: FpEngine = None,
        real_chunk: int = 256,
        z=None,
    ):
        """The observed sky maximum and its false-alarm probability:
        ``(femax (F,), argmax (F,), pfa (F,))`` with ``femax, argmax`` as
        :meth:`sweep_max` returns them and

            pfa = (1 + #{null >= femax}) / (1 + nreal)

        per frequency against the ``nreal`` realisations of
        :meth:`null_max` (same arguments, same stream, same scope: a
        single-frequency probability, no trials factor over frequency).
        The products and the antenna table are computed once and serve
        both passes."""
        engine, prods, ant = self._null_inputs(freqs, sky, Nvecs, Ts, sigmas,
                                               device, engine)
        if engine._use_hip:
            from fastfp_amd import ops

            fm, am, _ = ops.fe_skymax(prods, ant)
            femax = fm[0].cpu().numpy()
            argmax = am[0].cpu().numpy().astype(np.int64)
        else:
            # the assembly of ``sweep_max`` on a CPU engine, call for call
            grid = np.stack([_assemble_fe(prods[:, 0], ant[k, :, 0],
                                          ant[k, :, 1])
                             for k in range(ant.shape[0])])
            femax, argmax = np.nanmax(grid, axis=0), np.nanargmax(grid, axis=0)
        null = _null_chunks(prods, ant, nreal, seed, real_chunk, z,
                            engine.device, engine._use_hip)[:, 0, :]
        return femax, argmax, false_alarm_probability(femax, null)


def compute_Fe(psrs, pta, noise, freqs, sky, device=None) -> np.ndarray:
    """One-call convenience: precompute mats and sweep the grid."""
    from fastfp_amd.model import get_mats_fp

    Nvecs, Ts, sigmas = get_mats_fp(pta, noise)
    return FastFe(psrs, pta).sweep(freqs, sky, Nvecs, Ts, sigmas,
                                   device=device)


def _assemble_fe_draws(prods, fplus, fcross, rcond=1e-12, amplitudes=False):
    """Draw-batched Fe assembly: ``prods`` (P, D, 5, F) -> (D, F), or
    with ``amplitudes`` -> ``(fe (D, F), a (D, F, 4))``."""
    ss, cc, sc = prods[:, :, 0], prods[:, :, 1], prods[:, :, 2]
    sr, cr = prods[:, :, 3], prods[:, :, 4]
    fp2, fx2, fpx = fplus**2, fcross**2, fplus * fcross

    def w(coeff, q):  # (P,) x (P, D, F) -> (D, F)
        return np.einsum("p,pdf->df", coeff, q)

    D, F = prods.shape[1], prods.shape[3]
    M = np.empty((D, F, 4, 4))
    M[..., 0, 0] = w(fp2, ss)
    M[..., 0, 1] = M[..., 1, 0] = w(fp2, sc)
    M[..., 0, 2] = M[..., 2, 0] = w(fpx, ss)
    M[..., 0, 3] = M[..., 3, 0] = w(fpx, sc)
    M[..., 1, 1] = w(fp2, cc)
    M[..., 1, 2] = M[..., 2, 1] = w(fpx, sc)
    M[..., 1, 3] = M[..., 3, 1] = w(fpx, cc)
    M[..., 2, 2] = w(fx2, ss)
    M[..., 2, 3] = M[..., 3, 2] = w(fx2, sc)
    M[..., 3, 3] = w(fx2, cc)
    N = np.stack(
        [w(fplus, sr), w(fplus, cr), w(fcross, sr), w(fcross, cr)], axis=-1
    )  # (D, F, 4)
    x = _solve4(M, N, rcond)
    fe = 0.5 * np.einsum("dfi,dfi->df", N, x)
    return (fe, x) if amplitudes else fe


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

    def _engine(self, engine, freqs, samples, Nvecs, Ts, device, compress,
                freq_chunk=2048):
        """The caller's engine, or a fresh one on ``device`` — with draw
        compression enabled around the first draw when ``compress``."""
        if engine is not None:
            return engine
        engine = FpEngine(self.psrs, Nvecs, Ts, device=device)
        engine.precompute(freqs, freq_chunk=freq_chunk)
        if compress:
            engine.compress_around_first_draw(self.rn_sigs, samples)
        return engine

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

    def sweep(
        self,
        freqs,
        sky,
        samples: dict,
        Nvecs,
        Ts,
        device: str = None,
        draw_chunk: int = 128,
        freq_chunk: int = 2048,
        engine: FpEngine = None,
        assemble: str = "host",
        compress: bool = False,
    ) -> np.ndarray:
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
        from fastfp_amd.noise import batch_phiinv

        device = _check_assemble(assemble, device, engine)
        engine = self._engine(engine, freqs, samples, Nvecs, Ts, device,
                              compress, freq_chunk)
        phiinvs = batch_phiinv(self.rn_sigs, samples)
        phiinvs = [p[None, :] if p.dim() == 1 else p for p in phiinvs]
        D = phiinvs[0].shape[0]
        F = engine.freqs.shape[0]
        if assemble == "device":
            from fastfp_amd import ops

            _require_hip_engine(engine)
            ant_d = _antenna_table(self.fe.pos, sky, engine.device)
            out = np.empty((D, len(sky), F))
            for lo in range(0, D, draw_chunk):
                hi = min(lo + draw_chunk, D)
                prods = self._products(
                    engine, [p[lo:hi] for p in phiinvs], compress,
                    hip=True)  # (P, Dc, 5, F)
                out[lo:hi] = ops.fe_assemble(prods, ant_d).cpu().numpy()
            return out
        ant = [gw_antenna_pattern(self.fe.pos, th, ph) for th, ph in sky]
        out = np.empty((D, len(sky), F))
        for lo in range(0, D, draw_chunk):
            hi = min(lo + draw_chunk, D)
            prods = self._products(
                engine, [p[lo:hi] for p in phiinvs], compress, hip=False
            ).cpu().numpy()  # (P, Dc, 5, F)
            for k, (fplus, fcross) in enumerate(ant):
                out[lo:hi, k, :] = _assemble_fe_draws(prods, fplus, fcross)
        return out

    def sweep_max(
        self,
        freqs,
        sky,
        samples: dict,
        Nvecs,
        Ts,
        device: str = None,
        draw_chunk: int = 128,
        engine: FpEngine = None,
        compress: bool = False,
        amplitudes: bool = False,
    ):
        """Fe maximised over ``sky`` for every (draw, frequency).

        Returns ``(femax (D, F), argmax (D, F))``; ``argmax`` indexes
        into ``sky``.  The (D, nsky, F) cube is never formed: on a HIP
        engine each draw chunk goes products (HIP solve) ->
        ``fe_skymax`` kernel and only (Dc, F)-sized results leave the
        device; on a CPU engine each chunk is assembled on the host and
        reduced with ``np.nanmax`` / ``np.nanargmax`` (the reference
        implementation).  ``compress``: as in :meth:`sweep`.

        ``amplitudes``: return ``(femax, argmax, amps (D, F, 4))`` with
        the maximum-likelihood amplitudes at each maximum, as in
        :meth:`FastFe.sweep_max`.
        """
        from fastfp_amd.noise import batch_phiinv

        if device is None:
            device = "cuda" if torch.cuda.is_available() else "cpu"
        engine = self._engine(engine, freqs, samples, Nvecs, Ts, device,
                              compress)
        phiinvs = batch_phiinv(self.rn_sigs, samples)
        phiinvs = [p[None, :] if p.dim() == 1 else p for p in phiinvs]
        D = phiinvs[0].shape[0]
        F = engine.freqs.shape[0]
        femax = np.empty((D, F))
        argmax = np.empty((D, F), dtype=np.int64)
        amps = np.empty((D, F, 4)) if amplitudes else None
        if engine._use_hip:
            from fastfp_amd import ops

            ant_d = _antenna_table(self.fe.pos, sky, engine.device)
        else:
            ant = _antenna_table(self.fe.pos, sky)
        for lo in range(0, D, draw_chunk):
            hi = min(lo + draw_chunk, D)
            chunk = [p[lo:hi] for p in phiinvs]
            if engine._use_hip:
                prods = self._products(engine, chunk, compress,
                                       hip=True)  # (P, Dc, 5, F)
                fm, am, _ = ops.fe_skymax(prods, ant_d)
                femax[lo:hi] = fm.cpu().numpy()
                argmax[lo:hi] = am.cpu().numpy()
                if amplitudes:
                    amps[lo:hi] = ops.fe_amplitudes(
                        prods, ant_d, am)[0].cpu().numpy()
            elif amplitudes:
                prods = self._products(engine, chunk, compress,
                                       hip=False).cpu().numpy()
                femax[lo:hi], argmax[lo:hi], amps[lo:hi] = \
                    _host_max_amplitudes(
                        _assemble_fe_draws, prods,
                        [(ant[k, :, 0], ant[k, :, 1])
                         for k in range(len(sky))])
            else:
                prods = self._products(engine, chunk, compress,
                                       hip=False).cpu().numpy()
                cube = np.stack([
                    _assemble_fe_draws(prods, ant[k, :, 0], ant[k, :, 1])
                    for k in range(len(sky))
                ])  # (nsky, Dc, F)
                femax[lo:hi] = np.nanmax(cube, axis=0)
                argmax[lo:hi] = np.nanargmax(cube, axis=0)
        if amplitudes:
            return femax, argmax, amps
        return femax, argmax

    def null_max(
        self,
        freqs,
        sky,
        samples: dict,
        Nvecs,
        Ts,
        nreal: int,
        seed: int = 0,
        draw_chunk: int = 8,
        real_chunk: int = 128,
        engine: FpEngine = None,
        compress: bool = False,
        device: str = None,
    ) -> np.ndarray:
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
        :meth:`FastFe.null_max`."""
        from fastfp_amd.noise import batch_phiinv

        if device is None:
            device = "cuda" if torch.cuda.is_available() else "cpu"
        engine = self._engine(engine, freqs, samples, Nvecs, Ts, device,
                              compress)
        phiinvs = batch_phiinv(self.rn_sigs, samples)
        phiinvs = [p[None, :] if p.dim() == 1 else p for p in phiinvs]
        D = phiinvs[0].shape[0]
        F = engine.freqs.shape[0]
        hip = engine._use_hip
        ant = _antenna_table(self.fe.pos, sky, engine.device if hip else None)
        gen = torch.Generator(device=engine.device)
        gen.manual_seed(int(seed))
        out = np.empty((int(nreal), D, F))
        for lo in range(0, D, draw_chunk):
            hi = min(lo + draw_chunk, D)
            prods = self._products(engine, [p[lo:hi] for p in phiinvs],
                                   compress, hip=hip)  # (P, Dc, 5, F)
            if not hip:
                prods = prods.cpu().numpy()
            out[:, lo:hi] = _null_chunks(prods, ant, nreal, seed, real_chunk,
                                         None, engine.device, hip, gen=gen)
        return out
