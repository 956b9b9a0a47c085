"""HIP kernel op layer for the MI355X (gfx950).

Loads the in-tree extension ``_fastfp_hip`` built by ``setup.py
build_ext --inplace`` (or ``__graft_entry__.build()``).  On a GPU box
the HIP path is mandatory: :func:`require_hip` raises if the extension
is missing so eager fallback can never silently absorb GPU runs.
Set ``FASTFP_ALLOW_EAGER_GPU=1`` only for debugging comparisons.
"""

from __future__ import annotations

import os

import torch

_ext = None
_load_err = None


def _try_load():
    global _ext, _load_err
    if _ext is not None:
        return _ext
    try:
        from fastfp_amd.ops import _fastfp_hip as ext  # built in-tree

        _ext = ext
    except ImportError as e:  # pragma: no cover - exercised on GPU boxes
        _load_err = e
        _ext = None
    return _ext


def hip_available() -> bool:
    return _try_load() is not None


def require_hip() -> None:
    if os.environ.get("FASTFP_ALLOW_EAGER_GPU") == "1":
        return
    if _try_load() is None:
        raise RuntimeError(
            "fastfp_amd HIP extension (_fastfp_hip) is not built but a GPU "
            "run was requested. Build it in-tree with "
            "`python setup.py build_ext --inplace` (PYTORCH_ROCM_ARCH=gfx950) "
            f"or set FASTFP_ALLOW_EAGER_GPU=1 to debug with eager torch. "
            f"Original import error: {_load_err}"
        )


MAX_MP_CHOL = 128  # LDS-resident limit of the chol_batch kernel
MAX_MP = 256  # solve limit: trsm W registers (NBT*4 f64/lane at NBT=16)


def pad16(m: int) -> int:
    return max(16, (m + 15) // 16 * 16)


def check_m(m: int) -> int:
    """Solve-dimension check.  Up to mp=128 the batched Cholesky runs
    in the LDS-resident chol_batch kernel; 128 < mp <= 256 factors via
    batched rocSOLVER Cholesky + the diag_inv kernel and solves in the
    same register-resident trsm (W = NBT*4 doubles per lane).  Beyond
    256 use the Schur-compressed path (per-draw dimension = variable
    bins) or the CPU engine."""
    mp = pad16(m)
    if mp > MAX_MP:
        raise NotImplementedError(
            f"the direct per-draw solve supports m <= {MAX_MP} (got m={m}); "
            "use the Schur-compressed path (NMFp.sweep compress=True, on by "
            "default) whose per-draw dimension is the variable-bin count, "
            "or the CPU engine"
        )
    return mp


# ----------------------------------------------------------------------
# op wrappers (thin; shapes documented in the kernels)
# ----------------------------------------------------------------------
def _basis_rhs(A, weights, toas, TNr, freqs):
    """RHS (mp, 2F+1) = [A^T diag(weights) S | TNr] through the fused
    signal-basis MFMA DGEMM (sbgemm), rows zero-padded to mp."""
    ext = _try_load()
    F = int(freqs.shape[0])
    ntoa, m = A.shape
    mp = pad16(m)  # sbgemm is M-tiled: no 128 cap on the basis size
    RHS = torch.zeros((mp, 2 * F + 1), dtype=torch.float64, device=A.device)
    F2 = 2 * F
    ctiles = max(1, (F2 + 63) // 64)  # F = 0: sbgemm returns at once
    # split K to fill the 256-CU chip when the frequency grid is small;
    # partial planes + a deterministic torch reduction keep fp64
    # bitwise-reproducible (no atomics)
    ksplit = max(1, min(8, (512 + ctiles - 1) // ctiles, (ntoa + 255) // 256))
    if ksplit == 1:
        ext.sbgemm(A, toas, weights, freqs, RHS, 0, 2 * F + 1, mp, 1)
    else:
        part = torch.empty((ksplit, mp, F2), dtype=torch.float64,
                           device=A.device)
        ext.sbgemm(A, toas, weights, freqs, part, mp * F2, F2, mp, ksplit)
        RHS[:, :F2] = part.sum(dim=0)
    RHS[:m, -1] = TNr
    return RHS


def freq_precompute(toas, Nvec, r, T, TNr, freqs):
    """GPU frequency precompute for one pulsar.

    Returns (RHS (mp, 2F+1), sNs (3, F), sNr (2, F)).  The fused
    sigdots kernel computes the diagonal-weighted sin/cos dots; the
    fused signal-basis MFMA DGEMM (sbgemm) computes B = T^T (N^-1 S)
    with the S panel generated in LDS — NS is never materialized.
    RHS rows are zero-padded to mp (multiple of 16).

    Unlike the eager path there is no ``freq_chunk`` knob: the sin/cos
    S panel is generated tile-by-tile in LDS inside the kernels and no
    (F, ntoa) intermediate ever exists to bound.
    """
    ext = _try_load()
    Ninv = (1.0 / Nvec).contiguous()
    Nr = (r / Nvec).contiguous()
    freqs = freqs.contiguous()
    sNs, sNr = ext.sigdots(toas.contiguous(), Ninv, Nr, freqs)
    return _basis_rhs(T, Ninv, toas, TNr, freqs), sNs, sNr


def freq_precompute_block(toas, block_noise, Nr, V, TNr, freqs):
    """Block-diagonal-N (EcorrKernelNoise) frequency precompute.

    ``B = T^T N^-1 S = V^T S`` reuses the sbgemm kernel with V in place
    of T and unit weights; the per-frequency quadratics go through the
    sigdots_block kernel, which applies the exact Sherman–Morrison
    rank-1 correction per epoch block (any epoch size — no cap; the
    per-epoch blocks are diagonal + rank-1, see fastfp_amd.blocknoise).
    """
    ext = _try_load()
    freqs = freqs.contiguous()
    bt = block_noise.tensors(V.device)
    sNs, sNr = ext.sigdots_block(
        toas.contiguous(), bt["uvec"].contiguous(), Nr.contiguous(), freqs,
        bt["beta"].contiguous(), bt["offsets"], bt["sizes"],
    )
    ones = torch.ones(V.shape[0], dtype=torch.float64, device=V.device)
    return _basis_rhs(V, ones, toas, TNr, freqs), sNs, sNr


def chol_factor(TNT, phiinv, ext=None):
    """Batched Cholesky of Sigma = TNT + diag(phiinv) as the solve
    kernels take it: ``(L (P*D, mp, mp), invd (P*D, mp/16, 16, 16))``
    for TNT (m, m) / (P, m, m) and phiinv (D, m) / (P, D, m).

    mp <= 128: LDS-resident chol_batch kernel.  128 < mp <= 256
    (GP-ECORR direct path): Sigma no longer fits LDS — factor through
    batched rocSOLVER Cholesky (substitution-based, accurate; the
    rocBLAS accuracy caveat of docs/TUNING_NOTES.md concerns its
    inversion-based trsm, not potrf) + the diag_inv kernel.

    ``ext``: the extension to launch through (the engine passes its
    own); the loaded one by default."""
    if ext is None:
        ext = _try_load()
    m = TNT.shape[-1]
    mp = check_m(m)
    if mp <= MAX_MP_CHOL:
        L, invd = ext.chol_batch(TNT.contiguous(), phiinv.contiguous(), mp)
    else:
        batched = TNT.dim() == 3
        TNTb = TNT if batched else TNT.unsqueeze(0)  # (P, m, m)
        pib = phiinv if batched else phiinv.unsqueeze(0)  # (P, D, m)
        P, D = pib.shape[0], pib.shape[1]
        sigma = TNTb[:, None, :, :] + torch.diag_embed(pib)  # (P, D, m, m)
        Lt = torch.linalg.cholesky(sigma.reshape(P * D, m, m))
        L = torch.zeros((P * D, mp, mp), dtype=TNT.dtype, device=TNT.device)
        L[:, :m, :m] = Lt
        # identity padding: pad rows of RHS are zero, so results are
        # unchanged (same convention as chol_batch)
        idx = torch.arange(m, mp, device=TNT.device)
        L[:, idx, idx] = 1.0
        invd = ext.diag_inv(L.contiguous())
    return L, invd


def _grid_widths(cont):
    """``cont.Ffreqs`` contiguous and its pairwise bin widths, kept on the
    container while ``Ffreqs`` is the same unmodified tensor (the grid
    of a container is fixed; ``to(device)`` rebinds it)."""
    from fastfp_amd.noise import _bin_widths

    Ff = cont.Ffreqs
    key = (Ff.data_ptr(), Ff._version, Ff.device, tuple(Ff.shape))
    cached = getattr(cont, "_grid_widths", None)
    if cached is None or cached[0] != key:
        Fc = Ff.contiguous()
        cached = (key, Fc, _bin_widths(Fc).contiguous())
        cont._grid_widths = cached
    return cached[1], cached[2]


def phi_inv_batch(c0, gam, lgA, pars, tm_inv):
    """The homogeneous prior phi^-1 of ``noise.batch_phiinv`` in ONE
    kernel on the current stream: ``(P, D, ntm + nf)`` for the (P, D)
    device tensors ``gam``/``lgA`` of red-noise containers like ``c0``
    (with ``c0``'s common process from ``pars``), the timing-model
    columns set to ``tm_inv``.  Nothing but the output is allocated, so
    the call captures into a hipGraph.

    Returns None — the caller runs its torch chain — when the extension
    is not built or the common process's parameters are neither scalars
    nor one per draw."""
    ext = _try_load()
    if ext is None:
        return None
    import numpy as np

    from fastfp_amd.constants import fyr
    from fastfp_amd.noise import _as_tensor

    dev = gam.device
    P, D = gam.shape
    Ff, dff = _grid_widths(c0)
    if Ff.device != dev or Ff.numel() % 2:
        return None
    common = (None, None, None, None)
    if c0.add_curn:
        cc = c0.curn_container
        gc = _as_tensor(pars[cc.rn_gam_name], dev).reshape(-1).contiguous()
        lc = _as_tensor(pars[cc.rn_A_name], dev).reshape(-1).contiguous()
        Fc, dfc = _grid_widths(cc)
        if (gc.numel() != lc.numel() or gc.numel() not in (1, D)
                or Fc.device != dev or Fc.numel() > Ff.numel()):
            return None
        common = (gc, lc, Fc, dfc)
    ntm = c0.tm_weights.shape[0]
    out = torch.empty((P, D, ntm + Ff.numel()), dtype=torch.float64,
                      device=dev)
    # x / 12.0 and x / pi**2 of the torch chain are multiplications by
    # the rounded reciprocal of the scalar: the kernel takes those
    ext.phi_inv_batch(gam.contiguous(), lgA.contiguous(), common[0],
                      common[1], Ff, dff, common[2], common[3], ntm,
                      float(fyr), 1.0 / 12.0, 1.0 / np.pi**2, float(tm_inv),
                      out)
    return out


def chol_trsm_fp_accum(TNT, phiinv, RHS, sNs, sNr, fp_out, gsign=1.0):
    """:func:`chol_factor`, then the fused triangular solve of RHS
    (mp, 2F+1) + 2x2 Fp reduction, accumulating into fp_out (D, F).

    ``gsign``: +1 direct path (M = sNs - W.W); -1 Schur-compressed draw
    path (M = M0 + W.W) — docs/DESIGN.md §draw compression."""
    L, invd = chol_factor(TNT, phiinv)
    _try_load().trsm_fp_accum(L, invd, RHS, sNs, sNr, fp_out, gsign)


# ----------------------------------------------------------------------
# Fe sky assembly (fe_kernels.hip)
# ----------------------------------------------------------------------
def _fe_ext():
    require_hip()
    ext = _try_load()
    if ext is None:
        raise RuntimeError(
            "the Fe sky-assembly kernels need the HIP extension "
            f"(_fastfp_hip); import error: {_load_err}"
        )
    return ext


def _host_columns(prods, d_idx, f_idx, z=None):
    """The (d, f) columns ``d_idx, f_idx`` of the device product set
    ``prods`` (P, D, 5, F) as a host product set (P, ncols, 5, 1), for the
    host assembly of ``festat``; with ``z`` (D, F, P, 2, R) also its
    columns as (ncols, 1, P, 2, R)."""
    sub = prods[:, d_idx, :, f_idx].permute(1, 0, 2).unsqueeze(-1)
    if z is None:
        return sub.cpu().numpy()
    return sub.cpu().numpy(), z[d_idx, f_idx].unsqueeze(1).cpu().numpy()


def fe_assemble(prods, ant, repair: bool = True):
    """Fe over (draw, sky, frequency) on the device.

    ``prods`` (P, D, 5, F) = [ss, cc, sc, sr, cr] and ``ant``
    (nsky, P, 2) = [F+, Fx], both fp64 device tensors.  Returns the
    (D, nsky, F) device tensor.

    The kernel solves each point's 4x4 system by Cholesky in registers
    and writes NaN where a pivot is degenerate (``s_j <= 1e-12 M_jj``
    or non-finite).  With ``repair`` those entries are recomputed on the
    host through ``festat._assemble_fe_draws`` (pseudo-inverse branch);
    the common path costs one ``.any()`` sync.
    """
    ext = _fe_ext()
    fe = ext.fe_assemble(prods.contiguous(), ant.contiguous())
    if not repair:
        return fe
    bad = torch.isnan(fe)
    if bool(bad.any()):
        from fastfp_amd.festat import _assemble_fe_draws

        prods_h = prods.cpu().numpy()
        ant_h = ant.cpu().numpy()
        for k in torch.nonzero(bad.any(dim=2).any(dim=0)).flatten().tolist():
            full = torch.as_tensor(
                _assemble_fe_draws(prods_h, ant_h[k, :, 0], ant_h[k, :, 1]),
                dtype=fe.dtype,
            ).to(fe.device)  # (D, F)
            fe[:, k, :] = torch.where(bad[:, k, :], full, fe[:, k, :])
    return fe


def fe_skymax(prods, ant, repair: bool = True):
    """Fe maximised over the sky, fused in the kernel: nothing of size
    nsky x D x F is written.

    Returns ``(femax (D, F) f64, argmax (D, F) int32, nskip (D, F)
    int32)`` device tensors; ``argmax`` indexes the rows of ``ant`` (the
    lowest index on ties) and ``nskip`` counts the degenerate points the
    kernel left out of the maximum.  With ``repair`` every (d, f) column
    with ``nskip > 0`` is recomputed on the host over ALL sky points
    through ``festat._assemble_fe_draws`` (rare; the common path costs
    one ``.any()`` sync).  ``nskip`` keeps the kernel's counts.
    """
    ext = _fe_ext()
    femax, argmax, nskip = ext.fe_skymax(prods.contiguous(), ant.contiguous())
    if not repair:
        return femax, argmax, nskip
    bad = nskip > 0
    if bool(bad.any()):
        import numpy as np

        from fastfp_amd.festat import _assemble_fe_draws

        d_idx, f_idx = torch.nonzero(bad, as_tuple=True)
        sub_h = _host_columns(prods, d_idx, f_idx)
        ant_h = ant.cpu().numpy()
        vals = np.stack([
            _assemble_fe_draws(sub_h, ant_h[k, :, 0], ant_h[k, :, 1])[:, 0]
            for k in range(ant_h.shape[0])
        ])  # (nsky, ncols)
        femax[d_idx, f_idx] = torch.as_tensor(
            np.nanmax(vals, axis=0), dtype=femax.dtype).to(femax.device)
        argmax[d_idx, f_idx] = torch.as_tensor(
            np.nanargmax(vals, axis=0), dtype=argmax.dtype).to(argmax.device)
    return femax, argmax, nskip


def fe_amplitudes(prods, ant, idx, repair: bool = True):
    """Maximum-likelihood Fe amplitudes ``a = M^-1 N`` at one sky index
    per (draw, frequency) column, on the device: the products and the
    antenna table stay where ``fe_skymax`` read them.

    ``prods`` (P, D, 5, F) and ``ant`` (nsky, P, 2) as in
    :func:`fe_assemble` (any P >= 1: this kernel keeps no LDS tile);
    ``idx`` (D, F) integer rows of ``ant``, e.g. the ``argmax`` of
    :func:`fe_skymax`.  Returns ``(amps (D, F, 4) f64, fe (D, F) f64,
    status (D, F) int32)`` device tensors.  ``status`` 0: solved; 1: a
    degenerate or non-finite Cholesky pivot (the rule of the sky
    kernels); 2: ``idx`` outside ``[0, nsky)``.  ``amps`` and ``fe`` are
    NaN where ``status`` is not 0.

    With ``repair`` the status-1 columns are recomputed on the host
    through ``festat._assemble_fe_draws`` (pseudo-inverse branch) and
    come back finite; ``status`` keeps the kernel's values.  The common
    path costs one ``.any()`` sync.
    """
    ext = _fe_ext()
    idx = idx.to(device=prods.device, dtype=torch.int32).contiguous()
    amps, fe, status = ext.fe_amplitudes(
        prods.contiguous(), ant.contiguous(), idx)
    if not repair:
        return amps, fe, status
    bad = status == 1
    if bool(bad.any()):
        from fastfp_amd.festat import _assemble_fe_draws

        d_idx, f_idx = torch.nonzero(bad, as_tuple=True)
        rows = idx[d_idx, f_idx]
        for k in torch.unique(rows).tolist():
            sel = rows == k
            dk, fk = d_idx[sel], f_idx[sel]  # this sky row's bad columns
            ant_h = ant[k].cpu().numpy()
            fe_h, a_h = _assemble_fe_draws(
                _host_columns(prods, dk, fk), ant_h[:, 0], ant_h[:, 1],
                amplitudes=True)
            fe[dk, fk] = torch.as_tensor(
                fe_h[:, 0], dtype=fe.dtype).to(fe.device)
            amps[dk, fk] = torch.as_tensor(
                a_h[:, 0], dtype=amps.dtype).to(amps.device)
    return amps, fe, status


def fe_max_pulsars() -> int:
    """Largest pulsar count of the Fe sky kernels (``fe_assemble``,
    ``fe_skymax``, ``fe_null_skymax``)."""
    return int(_fe_ext().fe_max_pulsars())


def _null_lfac(prods):
    """(D, F, P, 3) = [l00, l10, l11], the Cholesky factors of the
    per-pulsar blocks [[ss, sc], [sc, cc]] of ``prods`` (P, D, 5, F):
    ``festat._null_factors`` in elementwise torch ops, its ``ValueError``
    for a block that is not positive definite included — one ``.all()``
    sync."""
    from fastfp_amd.festat import _null_factors

    return torch.stack(_null_factors(prods, torch),
                       dim=-1).permute(1, 2, 0, 3).contiguous()


def fe_null_data(white, rhs, X, out=None):
    """Joint null data of the Fe statistic on the device (docs/DESIGN.md
    section 14): ``n[d, f, p, c, r] = white[p, r, 2f+c] - sum_k rhs[p, k,
    2f+c] X[p, d, k, r]``, one fp64 MFMA GEMM per (pulsar, draw).

    ``white`` (P, Rp, ldw), ``Rp >= R`` and ``ldw >= 2F``, as ``sbgemm``
    writes it (the kernel transposes it); ``rhs`` (P, mp, 2F+1), the
    engine's stacked RHS, last column not read, ``mp`` a multiple of 16
    up to 256; ``X`` (P, D, mp, R) with zero padding rows.  Returns the
    contiguous (D, F, P, 2, R) tensor ``fe_null_skymax`` takes as
    ``z``, written into ``out`` when given."""
    ext = _fe_ext()
    P, D, R = X.shape[0], X.shape[1], X.shape[3]
    F = (rhs.shape[2] - 1) // 2
    if out is None:
        out = torch.empty((D, F, P, 2, R), dtype=torch.float64,
                          device=X.device)
    ext.fe_null_data(white, rhs, X, out)
    return out


def fe_null_data_torch(white, rhs, X):
    """What :func:`fe_null_data` computes, in torch ops: ``baddbmm`` per
    draw and a permuting copy into (D, F, P, 2, R).  The comparison arm
    of the measurement in docs/PERFORMANCE.md ("Fe joint null")."""
    P, D, R = X.shape[0], X.shape[1], X.shape[3]
    F = (rhs.shape[2] - 1) // 2
    wt = white[:, :R, :2 * F].transpose(1, 2)  # (P, 2F, R)
    Bt = rhs[:, :, :2 * F].transpose(1, 2)  # (P, 2F, mp)
    out = torch.empty((D, F, P, 2, R), dtype=torch.float64, device=X.device)
    for d in range(D):
        nd = torch.baddbmm(wt, Bt, X[:, d], alpha=-1.0)  # (P, 2F, R)
        out[d] = nd.reshape(P, F, 2, R).permute(1, 0, 2, 3)
    return out


def fe_null_skymax(prods, ant, z, repair: bool = True, rtiles: int = 0,
                   data: bool = False):
    """The sky maximum of Fe for ``R`` noise-only realisations per (draw,
    frequency) column, on the device (docs/DESIGN.md section 13).

    ``prods`` (P, D, 5, F) and ``ant`` (nsky, P, 2) as in
    :func:`fe_skymax` (only the planes ss, cc, sc are read); ``z``
    (D, F, P, 2, R) contiguous fp64 standard normals.  Realisation ``r``
    of pulsar ``p`` has the data products ``n = L_p z_p[r]`` with ``L_p``
    the Cholesky factor of ``[[ss, sc], [sc, cc]]_p``, which is how
    ``(sr, cr)_p`` is distributed under noise alone.  A block that is not
    positive definite raises ``ValueError`` naming its (pulsar, draw,
    frequency).

    Returns ``(femax (R, D, F) f64, argmax (R, D, F) int32, nskip (D, F)
    int32)`` device tensors, the first two as permuted views of the
    kernel's (D, F, R) output.  ``nskip`` counts the degenerate sky points
    of a column (bitwise those of :func:`fe_skymax`: they do not depend
    on the realisation).  With ``repair`` every column with ``nskip > 0``
    is recomputed on the host over ALL sky points through
    ``festat._null_max_host`` (pseudo-inverse at the degenerate points);
    ``nskip`` keeps the kernel's counts.  ``rtiles``: realisation tiles
    per workgroup (a tuning knob; no result depends on it).

    ``data``: ``z`` holds the data products ``n`` themselves, ``z[d, f, p]
    = (n_s, n_c)`` (the joint null of ``FpEngine.null_data``, section 14).
    The same kernel runs with the factor ``(1, 0, 1)``, under which ``n_s
    = 1 * z0`` and ``n_c = fma(0, z0, 1 * z1)`` are exact; the blocks are
    not factored and so not checked for positive definiteness.
    """
    ext = _fe_ext()
    if prods.dim() != 4 or prods.shape[2] != 5:
        raise RuntimeError("prods must be (P, D, 5, F)")
    prods = prods.contiguous()
    ant = ant.contiguous()
    if data:
        P, D, F = prods.shape[0], prods.shape[1], prods.shape[3]
        lfac = prods.new_tensor([1.0, 0.0, 1.0]).expand(D, F, P, 3).contiguous()
    else:
        lfac = _null_lfac(prods)
    femax, argmax, nskip = ext.fe_null_skymax(prods, ant, lfac, z, rtiles)
    if repair:
        bad = nskip > 0
        if bool(bad.any()):
            from fastfp_amd.festat import _null_max_host

            d_idx, f_idx = torch.nonzero(bad, as_tuple=True)
            sub_h, z_h = _host_columns(prods, d_idx, f_idx, z)
            fm, am = _null_max_host(sub_h, ant.cpu().numpy(),
                                    **{"n" if data else "z": z_h}
                                    )  # (R, ncols, 1)
            femax[d_idx, f_idx] = torch.as_tensor(
                fm[:, :, 0].T.copy(), dtype=femax.dtype).to(femax.device)
            argmax[d_idx, f_idx] = torch.as_tensor(
                am[:, :, 0].T.copy(), dtype=argmax.dtype).to(argmax.device)
    return femax.permute(2, 0, 1), argmax.permute(2, 0, 1), nskip
