"""The Fp-statistic compute engine (restructured math, device-aware).

The reference evaluates, for every (frequency, draw, pulsar), six
independent Woodbury products ``x^T C^-1 y`` each re-solving the same
Sigma (``/root/reference/fastfp/fastfp.py:81-88``,
``/root/reference/fastfp/utils.py:49-54``) and relies on XLA CSE.  This
engine restructures the computation around what is invariant along each
batch axis:

per pulsar (fixed):
    ``TNT = T^T N^-1 T``, ``TNr = T^T N^-1 r``
per (pulsar, frequency) (fixed across draws):
    ``B = T^T N^-1 [s, c]`` for the whole frequency grid at once — one
    GEMM — plus the diagonal-weighted dots ``sNs`` (3 per f) and ``sNr``
    (2 per f).  The common amplitude ``f^-1/3`` of the reference's filter
    (``/root/reference/fastfp/fastfp.py:78-79``) cancels exactly in
    ``N^T M^-1 N`` and is omitted here (proved in docs/DESIGN.md,
    verified against the oracle).
per (pulsar, draw):
    one Cholesky ``L L^T = Sigma = TNT + diag(phi^-1)`` and one
    triangular solve ``W = L^-1 [B | TNr]``; then for every frequency
    the 2x2 system is closed-form:

    ``M = sNs - W_s/c^T W_s/c``, ``N = sNr - W_s/c^T w_u``,
    ``Fp += 1/2 N^T M^-1 N``.

This turns 6*F*D*P Woodbury solves into P GEMMs + D*P Cholesky/TRSMs —
the MFMA-DGEMM-shaped form the MI355X wants.  On CPU the engine runs
vectorized torch eager (the unit-test oracle path); on a ROCm GPU the
hot ops are hand-written fp64 HIP kernels (fastfp_amd.ops), and falling
back silently to eager on GPU is an error.
"""

from __future__ import annotations

import contextlib
import math
import os
from typing import NamedTuple

import numpy as np
import torch

from fastfp_amd import ops


@contextlib.contextmanager
def _roctx(name: str):
    """Optional roctx ranges (shown in rocprof timelines) around the
    engine phases; enable with FASTFP_ROCTX=1."""
    if os.environ.get("FASTFP_ROCTX") == "1" and torch.cuda.is_available():
        torch.cuda.nvtx.range_push(name)
        try:
            yield
        finally:
            torch.cuda.nvtx.range_pop()
    else:
        yield


def _t64(x, device):
    if isinstance(x, torch.Tensor):
        return x.to(device=device, dtype=torch.float64)
    return torch.as_tensor(np.asarray(x, dtype=np.float64), device=device)


class SolveSystem(NamedTuple):
    """One per-draw solve as the kernels take it: Cholesky of
    ``A + diag(d)``, forward solve of ``RHS``, and the per-frequency
    2x2 closure ``M = S - gsign * W.W``, ``N = R - gsign * W.wu``.

    direct:      ``(TNT, RHS, sNs, sNr, +1)``, ``d = phiinv``
    compressed:  ``(G, K, M0, N0, -1)``,
                 ``d = 1 / (phiinv[var] - delta0)``  (docs/DESIGN.md)

    The same description serves one pulsar (``A`` (m, m), ``var`` a
    slice) and the pulsar stack (``A`` (P, m, m), ``var`` one slice per
    pulsar).

    ``lead`` (stacked compressed system only): ``A`` and ``RHS`` carry
    the padding of the solve dimension to a multiple of 16 themselves,
    in FRONT — ``A = blockdiag(I_lead, G)``, ``lead`` zero rows on top
    of ``RHS`` — and ``diag`` left-pads with zeros, so the padded Sigma
    has an exact identity block.  ``var`` and ``delta0`` keep the
    unpadded dimension."""

    A: torch.Tensor
    RHS: torch.Tensor
    S: torch.Tensor
    R: torch.Tensor
    gsign: float
    var: object = slice(None)  # columns of phiinv the diagonal is built from
    delta0: torch.Tensor = None  # compressed only: the reference prior
    lead: int = 0  # leading identity rows of A (zero rows of RHS)

    def diag(self, pinv):
        """phiinv rows (..., D, m), already cut to ``var``, -> the
        diagonal added to ``A``."""
        if self.delta0 is None:
            return pinv
        d = 1.0 / (pinv - self.delta0[..., None, :])
        if self.lead:
            d = torch.nn.functional.pad(d, (self.lead, 0))
        return d


def _close_2x2(prods, fp_out):
    """fp_out += 1/2 N^T M^-1 N from the five products (closed form)."""
    M11, M22, M12, N1, N2 = prods
    det = M11 * M22 - M12 * M12
    fp_out += 0.5 * (N1 * N1 * M22 - 2.0 * N1 * N2 * M12 + N2 * N2 * M11) / det


def _eager_products(system: SolveSystem, sigma):
    """Eager Cholesky + TRSM of the (D, m, m) ``sigma``, reduced to the
    five (D, F) products [ss, cc, sc, sr, cr] of ``system``."""
    D, m = sigma.shape[0], sigma.shape[-1]
    L = torch.linalg.cholesky(sigma)  # (D, m, m)
    W = torch.linalg.solve_triangular(
        L, system.RHS[:m, :][None].expand(D, -1, -1), upper=False
    )  # (D, m, 2F+1)
    wu = W[:, :, -1]  # (D, m)
    Ws, Wc = W[:, :, 0:-1:2], W[:, :, 1:-1:2]  # (D, m, F)
    g, S, R = system.gsign, system.S, system.R
    return (
        S[0][None] - g * (Ws * Ws).sum(1),
        S[1][None] - g * (Wc * Wc).sum(1),
        S[2][None] - g * (Ws * Wc).sum(1),
        R[0][None] - g * torch.einsum("dmf,dm->df", Ws, wu),
        R[1][None] - g * torch.einsum("dmf,dm->df", Wc, wu),
    )


def _per_column(A, X):
    """``A @ X`` for ``A`` (a, k) and ``X`` (k, R), as R independent
    matrix-vector products (one batch entry each): column r of the result
    is bitwise the same whatever other columns ``X`` holds, which a
    single GEMM does not promise."""
    R = X.shape[1]
    xt = X.transpose(0, 1).contiguous()[:, :, None]  # (R, k, 1)
    return torch.bmm(A.expand(R, *A.shape), xt)[:, :, 0].transpose(0, 1)


class PulsarBlock:
    """Per-pulsar device tensors + fixed precompute.

    ``Nvec`` may be a per-TOA variance vector (diagonal N) or a
    :class:`fastfp_amd.blocknoise.BlockNoise` (block-diagonal N, the
    EcorrKernelNoise case).  For block N the TOAs are re-ordered by the
    BlockNoise permutation (a pure relabeling — every inner product is
    permutation-invariant) and the engine precomputes ``V = N^{-1} T``
    so the frequency GEMM is unchanged: ``T^T N^{-1} S = V^T S``.
    """

    def __init__(self, toas, resid, Nvec, T, device):
        from fastfp_amd.blocknoise import BlockNoise

        toas = np.asarray(toas, dtype=np.float64)
        resid = np.asarray(resid, dtype=np.float64)
        T = np.asarray(T, dtype=np.float64)
        self.block_noise = Nvec if isinstance(Nvec, BlockNoise) else None
        if self.block_noise is not None:
            perm = self.block_noise.perm
            toas, resid, T = toas[perm], resid[perm], T[perm, :]
        self.toas = _t64(toas, device)
        self.r = _t64(resid, device)
        self.T = _t64(T, device).contiguous()
        self.ntoa, self.m = self.T.shape

        if self.block_noise is None:
            self.Nvec = _t64(Nvec, device)
            TN = self.T / self.Nvec[:, None]  # N^-1 T  (ntoa, m)
            self.Nr = self.r / self.Nvec
        else:
            self.Nvec = None
            TN = _t64(self.block_noise.solve(T), device)  # V = N^-1 T
            self.Nr = _t64(self.block_noise.solve(resid), device)
        self.V = TN.contiguous()
        self.TNT = self.T.transpose(0, 1) @ TN
        self.TNr = TN.transpose(0, 1) @ self.r

        # filled by freq precompute:
        self.RHS = None  # (m, 2F+1): interleaved [s_f, c_f] columns + TNr
        self.sNs = None  # (3, F): ss, cc, sc
        self.sNr = None  # (2, F): s.r, c.r
        self.direct = None  # SolveSystem(TNT, RHS, sNs, sNr, +1)
        # filled by enable_draw_compression (docs/DESIGN.md):
        self.comp = None  # SolveSystem(G, K, M0, N0, -1, var, delta0)


# Smallest compression margin (FpEngine.compression_margin: phiinv_d /
# delta0) at which a draw still runs the Schur-compressed system; below
# it callers take the exact direct path.
COMPRESSION_MARGIN_GUARD = 1.5


class FpEngine:
    """Restructured Fp/NM-Fp compute over a list of pulsars.

    Parameters
    ----------
    psrs : list of PulsarData (or anything with .toas/.residuals)
    Nvecs, Ts : per-pulsar white-noise diagonals and basis matrices
        (the ``get_mats_*`` outputs, keeping the reference's data flow).
    device : torch device ("cpu" or "cuda:N").
    """

    def __init__(self, psrs, Nvecs, Ts, device="cpu", force_eager=False):
        self.device = torch.device(device)
        self.blocks = [
            PulsarBlock(p.toas, p.residuals, nv, T, self.device)
            for p, nv, T in zip(psrs, Nvecs, Ts)
        ]
        self.names = [str(getattr(p, "name", i)) for i, p in enumerate(psrs)]
        self.freqs = None
        self._use_hip = False
        self._ext = None  # the HIP extension module, HIP engines only
        self._side_stream = None
        self._direct_stack = None  # stacked SolveSystems, None = not formed
        self._comp_stack = None
        self._pipe_bufs = None
        if self.device.type == "cuda" and not force_eager:
            ops.require_hip()  # fail loudly if the extension is missing
            self._ext = ops._try_load()
            self._use_hip = True
            # second stream: per-pulsar chol->trsm chains are independent,
            # so alternating pulsars across two streams overlaps each
            # pulsar's Cholesky with the previous pulsar's solve
            self._side_stream = torch.cuda.Stream(device=self.device)

    # ------------------------------------------------------------------
    # frequency precompute
    # ------------------------------------------------------------------
    def precompute(self, freqs, freq_chunk: int = 2048):
        """Compute B, sNs, sNr for all pulsars on the engine's frequency
        grid.  Chunked over frequencies to bound the (Fc, ntoa) sin/cos
        intermediate."""
        freqs = _t64(freqs, self.device).reshape(-1)
        self.freqs = freqs
        F = freqs.shape[0]
        # any existing compression state was built against the OLD
        # frequency grid; callers re-enable after re-precomputing
        self.disable_draw_compression()
        with _roctx("fastfp:freq_precompute"):
            for blk in self.blocks:
                if self._use_hip:
                    self._precompute_hip(blk, freqs)
                else:
                    self._precompute_eager(blk, freqs, freq_chunk)
                blk.direct = SolveSystem(blk.TNT, blk.RHS, blk.sNs, blk.sNr, 1.0)
        self._stack_direct()
        return self

    def _precompute_eager(self, blk: PulsarBlock, freqs, freq_chunk):
        F = freqs.shape[0]
        m = blk.m
        RHS = torch.empty((m, 2 * F + 1), dtype=torch.float64, device=self.device)
        sNs = torch.empty((3, F), dtype=torch.float64, device=self.device)
        sNr = torch.empty((2, F), dtype=torch.float64, device=self.device)
        for lo in range(0, F, freq_chunk):
            hi = min(lo + freq_chunk, F)
            arg = 2.0 * math.pi * freqs[lo:hi, None] * blk.toas[None, :]  # (Fc, ntoa)
            S = torch.sin(arg)
            C = torch.cos(arg)
            if blk.block_noise is None:
                NS = S / blk.Nvec[None, :]
                NC = C / blk.Nvec[None, :]
            else:
                NS = blk.block_noise.solve(S.transpose(0, 1)).transpose(0, 1)
                NC = blk.block_noise.solve(C.transpose(0, 1)).transpose(0, 1)
            # B columns: interleaved sin,cos  (B = S N^-1 T = S V)
            Bs = S @ blk.V  # (Fc, m)
            Bc = C @ blk.V
            RHS[:, 2 * lo : 2 * hi : 2] = Bs.transpose(0, 1)
            RHS[:, 2 * lo + 1 : 2 * hi : 2] = Bc.transpose(0, 1)
            sNs[0, lo:hi] = (S * NS).sum(dim=1)
            sNs[1, lo:hi] = (C * NC).sum(dim=1)
            sNs[2, lo:hi] = (S * NC).sum(dim=1)
            sNr[0, lo:hi] = S @ blk.Nr
            sNr[1, lo:hi] = C @ blk.Nr
        RHS[:, -1] = blk.TNr
        blk.RHS, blk.sNs, blk.sNr = RHS, sNs, sNr

    def _precompute_hip(self, blk: PulsarBlock, freqs):
        if blk.block_noise is None:
            # no freq_chunk: the HIP kernels generate the S panel in
            # LDS and need no chunking (ops.freq_precompute docstring)
            blk.RHS, blk.sNs, blk.sNr = ops.freq_precompute(
                blk.toas, blk.Nvec, blk.r, blk.T, blk.TNr, freqs
            )
        else:
            blk.RHS, blk.sNs, blk.sNr = ops.freq_precompute_block(
                blk.toas, blk.block_noise, blk.Nr, blk.V, blk.TNr, freqs
            )

    # ------------------------------------------------------------------
    # Schur draw-compression
    # ------------------------------------------------------------------
    def enable_draw_compression(self, var_slices, phiinv_fixed,
                                jitter_rel: float = 1e-8):
        """Compress the per-draw solve to the VARIABLE prior bins.

        The draw-dependent part of ``Sigma(theta) = TNT + diag(phi^-1)``
        lives only on the bins whose prior varies (the red-noise(+CURN)
        Fourier bins); the timing-model 1e-40 and fixed GP-ECORR bins
        never change.  With ``Sigma_0 = TNT + diag(phiinv_fixed)``
        (variable bins zeroed) and Woodbury,

          B^T Sigma_d^-1 B = B^T Sigma_0^-1 B - K^T C_d^-1 K,
          C_d = diag(phi_d[var]) + G,  K = (Sigma_0^-1 [B|TNr])[var],
          G = (Sigma_0^-1)[var, var],

        so the per-draw Cholesky/TRSM run at dimension m_v = |var bins|
        instead of m — 4x fewer TRSM flops at the benchmark shape
        (m=120, m_v=60).  The per-frequency baseline M0/N0 replaces
        sNs/sNr, and the fused reduction flips sign (M = M0 + W.W).

        ``var_slices``: per-pulsar slice of variable basis columns;
        ``phiinv_fixed``: per-pulsar (m,) fixed phi^-1 (values on the
        variable bins are ignored/zeroed).
        """
        assert self.freqs is not None, "call precompute(freqs) first"
        # The K/M0/N0/G setup runs on CPU LAPACK even for GPU engines:
        # rocBLAS trsm is inversion-based rather than backward-stable
        # substitution and measured ~50x less accurate here (1e-4 vs
        # 2e-6 of spectrum scale at the benchmark conditioning) — a
        # one-time ~2 MB/pulsar round trip buys LAPACK accuracy.
        wdev = torch.device("cpu")
        for blk, sl, pf in zip(self.blocks, var_slices, phiinv_fixed):
            m = blk.m
            pf = _t64(pf, wdev).clone()
            # Sigma_0 must be SPD even when timing-model columns are
            # (nearly) degenerate with red-noise Fourier columns, so the
            # variable bins keep a TINY reference prior delta_i
            # proportional to the Sigma diagonal; the per-draw
            # correction then uses Delta_d = phiinv_d - delta, valid
            # while phiinv_d >> delta (checked by compression_margin).
            # delta_i trades conditioning against margin EXACTLY (the
            # split is algebraically exact; only round-off depends on
            # it): the compression error scales ~ cond(Sigma_0)*eps ~
            # eps/jitter_rel, so 1e-8 keeps errors ~1e-9..1e-7 of the
            # spectrum scale (measured: 100x better than the r01
            # 1e-10, which left 6/67 bench pulsars over the probe tol).
            # The margin guard (compression_margin) falls back to the
            # direct path below COMPRESSION_MARGIN_GUARD.
            # rank-deficient TNT (basis larger than the TOA count)
            # leaves Sigma_0 supported only by the jitter along its
            # null space — keep such pulsars on the exact direct path
            # (checked BEFORE factoring: their Sigma_0 may not even be
            # numerically PD).  Near-degeneracy SHORT of deficiency is
            # handled by the empirical probe below: Cholesky-pivot
            # heuristics measured uncorrelated with the actual error.
            if blk.ntoa < m:
                blk.comp = None
                continue
            TNTc = blk.TNT.to(wdev)
            delta0 = jitter_rel * torch.diagonal(TNTc)[sl].abs()
            pf[sl] = delta0
            sigma0 = TNTc + torch.diag(pf)
            try:
                L0 = torch.linalg.cholesky(sigma0)
            except torch.linalg.LinAlgError:
                blk.comp = None  # fail safe to the exact direct path
                continue
            RHSe = blk.RHS[:m, :].to(wdev)  # (m, 2F+1)
            ncols = RHSe.shape[1]
            mv = len(range(*sl.indices(m)))
            sNs_c = blk.sNs.to(wdev)
            sNr_c = blk.sNr.to(wdev)
            # column-chunked solves (bounds LAPACK workspace/temporaries
            # at the 2e5-frequency SKA shape)
            K = torch.empty((mv, ncols), dtype=torch.float64)
            M0 = torch.empty((3, ncols // 2), dtype=torch.float64)
            N0 = torch.empty((2, ncols // 2), dtype=torch.float64)
            CH = 16384  # even: chunks stay aligned to sin/cos pairs
            # first pass: the u column (last), needed by every chunk
            wcol = torch.linalg.solve_triangular(
                L0, RHSe[:, -1:], upper=False
            )
            for lo in range(0, ncols, CH):
                hi = min(lo + CH, ncols)
                W0c = torch.linalg.solve_triangular(
                    L0, RHSe[:, lo:hi], upper=False
                )
                # frequency-column bookkeeping: chunks are aligned to
                # even columns (CH is even), so cols lo..hi-1 pair up;
                # the final chunk also carries the (already solved) u col
                fs, fe = lo // 2, (hi - (1 if hi == ncols else 0)) // 2
                Ws = W0c[:, 0 : 2 * (fe - fs) : 2]
                Wc = W0c[:, 1 : 2 * (fe - fs) : 2]
                wu = wcol[:, 0]
                M0[0, fs:fe] = sNs_c[0, fs:fe] - (Ws * Ws).sum(0)
                M0[1, fs:fe] = sNs_c[1, fs:fe] - (Wc * Wc).sum(0)
                M0[2, fs:fe] = sNs_c[2, fs:fe] - (Ws * Wc).sum(0)
                N0[0, fs:fe] = sNr_c[0, fs:fe] - Ws.T @ wu
                N0[1, fs:fe] = sNr_c[1, fs:fe] - Wc.T @ wu
                S0c = torch.linalg.solve_triangular(
                    L0.transpose(0, 1), W0c, upper=True
                )
                K[:, lo:hi] = S0c[sl, :]
            S0inv = torch.cholesky_inverse(L0)
            G = S0inv[sl, sl]
            if self._use_hip:
                mvp = ops.check_m(mv)
                Kp = torch.zeros((mvp, K.shape[1]), dtype=torch.float64)
                Kp[:mv] = K
                K = Kp
            blk.comp = SolveSystem(
                G.to(self.device).contiguous(),
                K.to(self.device).contiguous(),
                M0.to(self.device).contiguous(),
                N0.to(self.device).contiguous(),
                -1.0,
                var=sl,
                delta0=delta0.to(self.device),
            )
        self._probe_compression(phiinv_fixed)
        self._stack_compression()
        return self

    def _probe_compression(self, phiinv_fixed, tol: float = 1e-6):
        """Empirical accuracy guard: evaluate one probe draw per pulsar
        through BOTH the compressed and the direct path and drop
        compression where they disagree beyond ``tol`` — conditioning
        heuristics (Cholesky pivot ratios vs the jitter) measured
        uncorrelated with the real error, so measure instead.

        tol 1e-6 (10x tighter than round 1): with jitter_rel=1e-8 the
        measured bench-shape errors are 1e-8..7e-8 of the spectrum
        scale, so healthy pulsars pass with two orders of margin."""
        F = self.freqs.shape[0]
        for blk, pf in zip(self.blocks, phiinv_fixed):
            if blk.comp is None:
                continue
            pinv = _t64(pf, self.device).reshape(1, -1)
            ref = blk.direct
            if self._use_hip and blk.m > 128:
                # above m=128 the GPU direct factor routes through
                # rocSOLVER; for the probe's REFERENCE arm prefer
                # the CPU LAPACK eager path on this one draw
                # (compression precompute is already pinned to CPU,
                # so this adds one more small host round trip at
                # setup time only)
                ref = SolveSystem(*(t.cpu() for t in ref[:4]), ref.gsign)
            fpA = torch.zeros((1, F), dtype=torch.float64, device=self.device)
            fpB = torch.zeros((1, F), dtype=torch.float64, device=ref.A.device)
            try:
                for system, out in ((blk.comp, fpA), (ref, fpB)):
                    p = pinv.to(out.device)
                    self._accumulate(
                        system, system.diag(p[:, system.var]).contiguous(), out
                    )
            except torch.linalg.LinAlgError:
                blk.comp = None  # pathological probe (e.g. phi < jitter)
                continue
            fpB = fpB.to(self.device)
            # error against the SPECTRUM scale: per-frequency relative
            # error is meaningless at cancellation-dominated frequencies
            # (docs/DESIGN.md §8) and mis-flags healthy models
            scale = fpB.abs().max().clamp_min(1e-30)
            err = (fpA - fpB).abs().max() / scale
            blk.probe_err = float(err)  # kept for diagnostics
            # NaN-safe: a non-finite probe (GPU kernels don't raise) or
            # a too-large error both disqualify the compressed path
            if not bool(torch.isfinite(err)) or float(err) > tol:
                blk.comp = None

    def _stack(self, systems):
        """Stack per-pulsar systems of one shape into a single
        ``(P, ...)`` system, so a whole sweep is ONE chol launch + ONE
        trsm launch per draw chunk (grid.z = pulsar) — no per-pulsar
        launch gaps or tail quantization.  Per-pulsar Fp planes are
        summed deterministically by torch.  None when the stack does
        not form (eager engine, a missing system, ragged shapes, or a
        dimension beyond the solve kernels)."""
        if not self._use_hip or any(s is None for s in systems):
            return None
        shapes = {(tuple(s.A.shape), tuple(s.RHS.shape)) for s in systems}
        if len(shapes) != 1 or systems[0].A.shape[-1] > ops.MAX_MP:
            return None
        A, RHS, S, R = (
            torch.stack(ts).contiguous()
            for ts in zip(*(s[:4] for s in systems))
        )
        delta0, lead = None, 0
        if systems[0].delta0 is not None:
            delta0 = torch.stack([s.delta0 for s in systems]).contiguous()
            # Compressed stack within the draw-looping solve: pad the
            # solve dimension in FRONT.  Sigma then starts with an exact
            # identity block over zero RHS rows, L[lead:, :lead] and the
            # first `lead` rows of W are exact zeros, and trsm_fp_store
            # leaves out the MFMAs that would multiply them.
            mv = A.shape[-1]
            mp = ops.pad16(mv)
            if mp <= self.DRAW_LOOP_MAX_MP and mp > mv:
                lead = mp - mv
                Ap = A.new_zeros((A.shape[0], mp, mp))
                Ap[:, :lead, :lead] = torch.eye(lead, dtype=A.dtype,
                                                device=A.device)
                Ap[:, lead:, lead:] = A
                Kp = RHS.new_zeros((RHS.shape[0], mp, RHS.shape[2]))
                Kp[:, lead:] = RHS[:, :mv]
                A, RHS = Ap, Kp
        return SolveSystem(A, RHS, S, R, systems[0].gsign,
                           var=[s.var for s in systems], delta0=delta0,
                           lead=lead)

    def _stack_direct(self):
        """Stacked DIRECT system (same dimensions across pulsars; used
        by the plain-Fp phiinv path, the compression-margin fallback
        and the Fe products)."""
        self._direct_stack = self._stack([blk.direct for blk in self.blocks])

    def _stack_compression(self):
        """Stacked COMPRESSED system: forms when every pulsar
        compresses to the same variable dimension."""
        self._comp_stack = self._stack([blk.comp for blk in self.blocks])

    def _rows(self, phiinvs):
        """Per-pulsar phiinvs, each (m,) or (D, m) -> (list of (D, m)
        device tensors, whether the input was draw-batched)."""
        rows = [_t64(p, self.device) for p in phiinvs]
        batched = rows[0].dim() == 2
        return [p[None, :] if p.dim() == 1 else p for p in rows], batched

    def compression_margin_per_draw(self, phiinvs) -> torch.Tensor:
        """Per-draw compression margin: (D,) tensor of
        min over pulsars/bins of phiinv_d / delta0.  Basis of the
        per-draw hybrid split (NMFp.sweep): draws above the guard run
        compressed, the (rare) prior-corner draws run the exact direct
        path — one extreme draw no longer forces a whole batch off the
        fast path.  Returns +inf per draw when nothing is compressed.

        No device sync: per-pulsar mins are stacked and reduced on
        device.  When every pulsar compresses with the same variable
        slice (the stacked homogeneous case), the whole check is one
        stack, one divide and one min."""
        st = self._comp_stack
        if (
            st is not None
            and all(sl == st.var[0] for sl in st.var)
            and all(
                isinstance(p, torch.Tensor)
                and p.device == self.device
                and p.dim() == 2
                for p in phiinvs
            )
        ):
            pall = torch.stack(list(phiinvs))  # (P, D, m)
            ratio = pall[:, :, st.var[0]] / st.delta0[:, None, :]
            return ratio.amin(dim=(0, 2))
        rows, _ = self._rows(phiinvs)
        mins = [
            (p[:, blk.comp.var] / blk.comp.delta0[None, :]).min(dim=1).values
            for blk, p in zip(self.blocks, rows)
            if blk.comp is not None
        ]
        if not mins:
            return torch.full((rows[0].shape[0],), float("inf"),
                              dtype=torch.float64, device=self.device)
        return torch.stack(mins).min(dim=0).values

    def compression_margin(self, phiinvs) -> float:
        """min over pulsars/draws/bins of phiinv_d / delta_0.  The
        compressed path is numerically safe above
        ``COMPRESSION_MARGIN_GUARD`` (the split is algebraically exact;
        precision of the Delta = phiinv - delta0 subtraction degrades
        as eps/(1 - 1/margin) and Delta <= 0 is the NaN cliff —
        measured 2e-10 error at margin 1.7).  Callers fall back to the
        exact direct path below the guard.

        One device sync total (a per-pulsar ``float()`` cost 67 syncs
        per draw batch in the CLI hot loop)."""
        return float(self.compression_margin_per_draw(phiinvs).min())

    def margin_split(self, phiinvs, compressed, direct, dim: int = 0):
        """The per-draw hybrid: ``compressed(rows)`` on the draws whose
        compression margin reaches ``COMPRESSION_MARGIN_GUARD``,
        ``direct(rows)`` on the (rare) prior-corner draws below it —
        ``rows`` being ``phiinvs`` cut to those draws — and the two
        results scattered back in draw order along ``dim``.  One
        extreme draw does not take a whole batch off the fast path."""
        bad = (self.compression_margin_per_draw(phiinvs)
               < COMPRESSION_MARGIN_GUARD)
        if not bool(bad.any()):
            return compressed(phiinvs)
        out = None
        for idx, run in ((torch.nonzero(~bad).reshape(-1), compressed),
                         (torch.nonzero(bad).reshape(-1), direct)):
            if not len(idx):
                continue
            part = run([p[idx.to(p.device)] for p in phiinvs])
            if out is None:
                shape = list(part.shape)
                shape[dim] = bad.shape[0]
                out = part.new_empty(shape)
            out.index_copy_(dim, idx.to(out.device), part)
        return out

    def compress_around_first_draw(self, rn_sigs, samples):
        """:meth:`enable_draw_compression` for the phi containers
        ``rn_sigs``, with the fixed phi^-1 taken at the first draw of
        ``samples`` (any parameter point serves: the variable bins are
        zeroed inside)."""
        probe = {k: (v[0] if np.ndim(v) else v) for k, v in samples.items()}
        return self.enable_draw_compression(
            [sig.var_slice for sig in rn_sigs],
            [sig.get_phiinv(probe) for sig in rn_sigs],
        )

    def disable_draw_compression(self):
        for blk in self.blocks:
            blk.comp = None
        self._comp_stack = None  # the stacked path must also fall back
        return self

    # ------------------------------------------------------------------
    # sweeps
    # ------------------------------------------------------------------
    def _accumulate(self, system: SolveSystem, diag, fp_out, sigma=None):
        """fp_out (D, F) += Fp of ``system`` with the (D, m) ``diag``
        on its A: the HIP kernels on a HIP engine, eager torch (the
        unit-test oracle path) otherwise and for host-resident systems.
        ``sigma``: a caller-supplied dense A + diag(d) for the eager
        path (the ``get_mats_fp`` contract)."""
        if self._use_hip and diag.is_cuda:
            L, invd = ops.chol_factor(system.A, diag, ext=self._ext)
            self._solve(system, L, invd, fp_out, accumulate=True)
            return
        if sigma is None:
            sigma = system.A[None, :, :] + torch.diag_embed(diag)
        _close_2x2(_eager_products(system, sigma), fp_out)

    def sweep(
        self,
        phiinvs=None,
        sigmas=None,
        draw_chunk: int = 32,
        accumulate_to=None,
        force_direct: bool = False,
    ) -> torch.Tensor:
        """Run the Fp sweep over the precomputed frequency grid.

        ``phiinvs``: per-pulsar diagonal phi^-1, shape (m,) for the plain
        Fp path or (D, m) for D noise draws.  Alternatively pass dense
        ``sigmas`` (m, m) / (D, m, m) directly (the ``get_mats_fp``
        contract).  Returns Fp of shape (F,) or (D, F).

        ``force_direct``: bypass the Schur compression for THIS call
        (used by the per-draw hybrid for prior-corner draws whose
        margin is below the guard).
        """
        assert self.freqs is not None, "call precompute(freqs) first"
        F = self.freqs.shape[0]
        rows = None
        if phiinvs is not None:
            rows, batched = self._rows(phiinvs)
            D = rows[0].shape[0]
        else:
            first = _t64(sigmas[0], self.device)
            batched = first.dim() == 3
            D = first.shape[0] if batched else 1

        fp = accumulate_to
        if fp is None:
            fp = torch.zeros((D, F), dtype=torch.float64, device=self.device)

        stack = None
        if rows is not None and not force_direct:
            stack = self._comp_stack
        if stack is None and rows is not None and (
            force_direct or all(blk.comp is None for blk in self.blocks)
        ):
            stack = self._direct_stack
        if stack is not None:
            # one chol + one trsm launch per draw chunk across ALL pulsars
            self._solve_chunks(stack, rows, draw_chunk, fp, pipeline=True)
            return fp[0] if not batched else fp

        fp_side = None
        main_stream = None
        if self._use_hip:
            main_stream = torch.cuda.current_stream(self.device)
            fp_side = torch.zeros_like(fp)
            ev = torch.cuda.Event()
            ev.record(main_stream)
            self._side_stream.wait_event(ev)

        for lo in range(0, D, draw_chunk):
            hi = min(lo + draw_chunk, D)
            for i, blk in enumerate(self.blocks):
                side = self._use_hip and (i & 1) == 1
                stream_ctx = (
                    torch.cuda.stream(self._side_stream)
                    if side
                    else contextlib.nullcontext()
                )
                fp_tgt = (fp_side if side else fp)[lo:hi]
                direct = force_direct or blk.comp is None
                system = blk.direct if direct else blk.comp
                with stream_ctx:
                    if rows is not None:
                        pinv = rows[i][lo:hi]
                        sigma = None
                    else:
                        sg = _t64(sigmas[i], self.device)
                        sigma = sg[None, :, :] if sg.dim() == 2 else sg[lo:hi]
                        # get_mats_fp contract: sigma = TNT + diag(phi^-1)
                        pinv = (
                            torch.diagonal(sigma, dim1=-2, dim2=-1)
                            - torch.diagonal(blk.TNT)[None, :]
                        )
                    self._accumulate(
                        system,
                        system.diag(pinv[:, system.var]).contiguous(),
                        fp_tgt,
                        sigma=sigma if direct else None,
                    )

        if self._use_hip:
            ev2 = torch.cuda.Event()
            ev2.record(self._side_stream)
            main_stream.wait_event(ev2)
            fp += fp_side

        return fp[0] if not batched else fp

    # Fewest draws in a chunk for which a sweep solves with the
    # draw-looping kernel (trsm_fp_store / trsm_prods_store, mp <= 64);
    # below it the one-draw-per-workgroup kernel runs.
    # docs/TUNING_NOTES.md has the measurement behind the value.
    DRAW_LOOP_MIN_DRAWS = 16
    DRAW_LOOP_MAX_MP = 64

    def _draw_loop_solve(self, sy: SolveSystem, ndraws: int,
                         prods: bool = False) -> bool:
        """Whether ``ndraws`` draws of ``sy`` solve with the
        draw-looping kernel."""
        # unmeasured: the stacked DIRECT products never take the draw
        # loop, the per-pulsar direct ones do (docs/ROADMAP.md)
        if prods and sy.A.dim() == 3 and sy.delta0 is None:
            return False
        return (ops.pad16(sy.A.shape[-1]) <= self.DRAW_LOOP_MAX_MP
                and ndraws >= self.DRAW_LOOP_MIN_DRAWS)

    def _solve(self, sy: SolveSystem, L, invd, out, prods=False,
               accumulate=False):
        """Solve ``sy`` on its factor ``L``/``invd`` into the contiguous
        ``out``: Fp ((P,) D, F), or with ``prods`` the five products
        ((P,) D, 5, F).  Every entry of ``out`` is overwritten, unless
        ``accumulate`` asks to add Fp to what ``out`` holds.  The one
        place that chooses among the four solve kernels."""
        ext = self._ext
        args = (L, invd, sy.RHS, sy.S, sy.R, out, sy.gsign)
        ndraws = out.shape[sy.A.dim() - 2]
        if not accumulate and self._draw_loop_solve(sy, ndraws, prods):
            op = ext.trsm_prods_store if prods else ext.trsm_fp_store
            # the solve skips whole 4-row k-steps of the leading pad
            op(*args, lead=sy.lead - sy.lead % 4)
        elif prods:
            ext.trsm_prods(*args)
        else:
            if not accumulate:
                out.zero_()
            ext.trsm_fp_accum(*args)

    def _rows_in_place(self, sy: SolveSystem, rows):
        """``(row0, pstride, var0)`` when the factor of the stacked
        ``sy`` can read its diagonal from ``rows`` where they lie
        (``chol_rows_into``), None otherwise.

        That takes the per-pulsar (D, m) ``rows`` to be regular views of
        ONE device tensor — same storage, same shape and strides, unit
        column stride, pulsar p's view ``p * pstride`` elements behind
        pulsar 0's ``row0``, which is what ``noise.batch_phiinv``
        returns — every pulsar's ``var`` to be the same contiguous
        column range of them (``var0`` its first column), and the
        system to factor in the LDS-resident kernel.  Host-side pointer
        and stride comparisons only: no sync, nothing launched."""
        if (sy.A.dim() != 3 or not isinstance(rows, (list, tuple))
                or len(rows) != sy.A.shape[0]
                or ops.pad16(sy.A.shape[-1]) > ops.MAX_MP_CHOL):
            return None
        r0 = rows[0]
        if (not r0.is_cuda or r0.dtype != torch.float64 or r0.dim() != 2
                or (r0.shape[1] > 1 and r0.stride(1) != 1)):
            return None
        D, width = r0.shape
        if not all(isinstance(v, slice) for v in sy.var):
            return None
        spans = {v.indices(width) for v in sy.var}
        if len(spans) != 1:
            return None
        (var0, stop, step), = spans
        if step != 1 or stop - var0 != sy.A.shape[-1] - sy.lead:
            return None
        base = r0.untyped_storage().data_ptr()
        pstride = 0
        for i, r in enumerate(rows[1:], 1):
            if (r.dtype != r0.dtype or r.shape != r0.shape
                    or r.untyped_storage().data_ptr() != base
                    or (width > 1 and r.stride(1) != 1)
                    or (D > 1 and r.stride(0) != r0.stride(0))):
                return None
            off = r.storage_offset() - r0.storage_offset()
            if i == 1:
                pstride = off
            if pstride < 0 or off != i * pstride:
                return None
        return r0, pstride, var0

    def _pipeline_chunks(self, sy: SolveSystem, factor_into, chunks):
        """``(lo, hi, L, invd)`` per draw chunk of a stacked system
        within ``MAX_MP_CHOL``, from a factor/solve software pipeline
        with PING-PONG factor buffers and two-way event fencing;
        ``factor_into(lo, hi, L, invd)`` launches the factor of the
        draws [lo, hi) into the buffers.

        Chunk k+1's factor (side stream, buffer (k+1)&1) overlaps chunk
        k's solve, which the consumer queues on the main stream before
        it asks for the next chunk; before overwriting a buffer, the
        side stream waits on the event recorded after the solve that
        last read it.  Explicit reusable buffers instead of per-chunk
        allocations + record_stream: the latter defers caching-
        allocator reuse across streams and measured as multi-GB
        allocator churn (2.2 s/step) on the 9.5 GB direct-path chunks.
        The structure is hipGraph-capturable (events + two streams
        forked from the capture stream)."""
        dev = self.device
        P, mp = sy.A.shape[0], ops.pad16(sy.A.shape[-1])
        nmax = P * (chunks[0][1] - chunks[0][0])
        key = ("pipebuf", nmax, mp)
        bufs = self._pipe_bufs
        if bufs is None or bufs[0] != key:
            L0 = torch.empty((nmax, mp, mp), dtype=torch.float64, device=dev)
            L1 = torch.empty_like(L0)
            i0 = torch.empty((nmax, mp // 16, 16, 16), dtype=torch.float64,
                             device=dev)
            i1 = torch.empty_like(i0)
            bufs = (key, (L0, L1), (i0, i1))
            self._pipe_bufs = bufs
        _, Lb, Ib = bufs

        main = torch.cuda.current_stream(dev)
        side = self._side_stream
        side.wait_stream(main)  # inputs visible to side
        solve_done = [None, None]  # event after the solve reading buf b

        def factor(i, lo, hi):
            b, n = i & 1, P * (hi - lo)
            with torch.cuda.stream(side):
                if solve_done[b] is not None:
                    side.wait_event(solve_done[b])
                factor_into(lo, hi, Lb[b][:n], Ib[b][:n])
                ev = torch.cuda.Event()
                ev.record(side)
            return ev

        pending = factor(0, *chunks[0])
        for i, (lo, hi) in enumerate(chunks):
            ev = pending
            if i + 1 < len(chunks):
                pending = factor(i + 1, *chunks[i + 1])
            main.wait_event(ev)
            b, n = i & 1, P * (hi - lo)
            yield lo, hi, Lb[b][:n], Ib[b][:n]
            # resumed once the consumer has queued its solve of buffer b
            ev2 = torch.cuda.Event()
            ev2.record(main)
            solve_done[b] = ev2

    def _solve_chunks(self, sy: SolveSystem, rows, draw_chunk, out,
                      prods=False, pipeline=False):
        """The one driver of the HIP sweeps: walk the draws of ``rows``
        (the (D, m) phiinv rows of one pulsar, or the list of them for a
        stack) in chunks — diagonal, factor, solve into a contiguous
        per-chunk buffer.  With ``prods`` the products land in ``out``
        ((P,) D, 5, F); otherwise (stacked only) the chunk's per-pulsar
        Fp planes are summed, deterministically by torch, into ``out``
        (D, F)."""
        mp = ops.pad16(sy.A.shape[-1])
        inrows = self._rows_in_place(sy, rows)
        if inrows is not None:
            # the factor reads the prior rows where they lie: no gathered
            # copy, no diagonal kernels in front of a factor launch
            row0, pstride, var0 = inrows
            lead_dims, D = (sy.A.shape[0],), row0.shape[0]

            def factor_into(lo, hi, L, invd):
                self._ext.chol_rows_into(sy.A, row0, pstride, lo, hi - lo,
                                         var0, sy.delta0, sy.lead, mp, L,
                                         invd)

            def factor(lo, hi):
                n = sy.A.shape[0] * (hi - lo)
                L = torch.empty((n, mp, mp), dtype=torch.float64,
                                device=self.device)
                invd = torch.empty((n, mp // 16, 16, 16),
                                   dtype=torch.float64, device=self.device)
                factor_into(lo, hi, L, invd)
                return L, invd
        else:
            if sy.A.dim() == 3:  # gathered and stacked once: (P, D, m_var)
                pinv = torch.stack([p[:, v] for p, v in zip(rows, sy.var)])
            else:
                pinv = rows[:, sy.var]
            lead_dims, D = tuple(pinv.shape[:-2]), pinv.shape[-2]

            def diag(lo, hi):
                return sy.diag(pinv[..., lo:hi, :]).contiguous()

            def factor_into(lo, hi, L, invd):
                self._ext.chol_batch_into(sy.A, diag(lo, hi), mp, L, invd)

            def factor(lo, hi):
                return ops.chol_factor(sy.A, diag(lo, hi), ext=self._ext)

        chunks = [(lo, min(lo + draw_chunk, D))
                  for lo in range(0, D, draw_chunk)]
        if not chunks:
            return

        def empty(n):  # what the solve writes for n draws
            return torch.empty(
                lead_dims + (n,) + out.shape[-2 if prods else -1:],
                dtype=torch.float64, device=self.device)

        # SOFTWARE PIPELINE across the chunks of a stacked Fp sweep:
        # chunk k+1's factor runs on a side stream beside chunk k's
        # solve.  The solve kernels fill the register file (4 waves/SIMD
        # at 128 VGPR), so a CU that takes factor workgroups gives up
        # solve workgroups for as long as they live: measured, the step
        # pays about 0.8 of the factor's stand-alone time per chunk, and
        # the pipeline hides the other fifth (docs/TUNING_NOTES.md).
        # Above MAX_MP_CHOL the factor is rocSOLVER's, which does not
        # write into caller buffers.
        if pipeline and len(chunks) > 1 and mp <= ops.MAX_MP_CHOL:
            factors = self._pipeline_chunks(sy, factor_into, chunks)
        else:
            factors = ((lo, hi, *factor(lo, hi)) for lo, hi in chunks)
        n0 = chunks[0][1]
        # products go straight into `out` where its draw slices are
        # contiguous (one pulsar, or a single chunk); otherwise through
        # one full-size buffer, and a tail chunk through its own
        inplace = prods and out[..., :n0, :, :].is_contiguous()
        full = None if inplace else empty(n0)
        for lo, hi, L, invd in factors:
            if inplace:
                buf = out[..., lo:hi, :, :]
            else:
                buf = full if hi - lo == n0 else empty(hi - lo)
            self._solve(sy, L, invd, buf, prods)
            if not prods:
                out[lo:hi] += buf.sum(dim=0)
            elif not inplace:
                out[..., lo:hi, :, :] = buf

    def sweep_products(self, sigmas=None, phiinvs=None,
                       compressed: bool = False) -> torch.Tensor:
        """Per-pulsar corrected inner products
        [s|s, c|c, s|c, s|r, c|r], each ``(x|y) = x^T C_p^{-1} y``
        over the precomputed frequency grid.

        Fixed noise ((m,) phiinvs / (m, m) sigmas): returns (P, 5, F).
        Draw-batched ((D, m) phiinvs / (D, m, m) sigmas): returns
        (P, D, 5, F) — the noise-marginalized Fe input.

        These are exactly the quantities the Fp reduction consumes
        before its per-pulsar 2x2 solve; exposing them lets sky-
        coherent statistics (the Fe assembly, ``fastfp_amd.festat``)
        reuse the engine's precompute + one m-dim solve per (pulsar,
        draw) and pay only O(P) per additional sky location.  Runs on
        the engine's device (torch batched Cholesky/solve — setup-
        scale work, not the draw-batched Fp hot path).

        ``compressed`` (``phiinvs`` only): take each pulsar's products
        from its Schur-compressed system where it has one
        (:meth:`enable_draw_compression`), from the direct system
        otherwise.  The per-draw margin is the caller's business, as in
        :meth:`sweep`."""
        assert self.freqs is not None, "call precompute(freqs) first"
        if compressed and sigmas is not None:
            raise ValueError("compressed=True takes phiinvs, not sigmas")
        if sigmas is not None:
            dense = [_t64(s, self.device) for s in sigmas]
            batched = dense[0].dim() == 3
            dense = [s[None] if s.dim() == 2 else s for s in dense]
            systems = [blk.direct for blk in self.blocks]
        else:
            rows, batched = self._rows(phiinvs)
            systems = [
                blk.comp if compressed and blk.comp is not None
                else blk.direct
                for blk in self.blocks
            ]
            dense = [self._dense(sy, p) for sy, p in zip(systems, rows)]
        out = torch.stack([
            torch.stack(_eager_products(sy, sigma), dim=1)
            for sy, sigma in zip(systems, dense)
        ])  # (P, D, 5, F)
        return out[:, 0] if not batched else out

    # ------------------------------------------------------------------
    # joint null across frequencies (docs/DESIGN.md section 14)
    # ------------------------------------------------------------------
    def null_normals(self, nreal: int, gen):
        """``(w, u)``: per-pulsar standard normals ``w_p (ntoa_p, nreal)``
        and ``u_p (m_p, nreal)`` from the ``torch.Generator`` ``gen`` on
        the engine's device, in pulsar order (w_0, u_0, w_1, ...)."""
        w, u = [], []
        for blk in self.blocks:
            for rows, out in ((blk.ntoa, w), (blk.m, u)):
                out.append(torch.randn((rows, int(nreal)), generator=gen,
                                       dtype=torch.float64,
                                       device=self.device))
        return w, u

    def _null_kernel_path(self) -> bool:
        """Whether the joint null runs white term and combine in the HIP
        kernels: a HIP engine whose direct systems stack."""
        return self._use_hip and self._direct_stack is not None

    def _null_white(self, w, freq_chunk: int = 2048):
        """The part of the joint null data that no noise draw changes:
        ``(white, Tw)`` with ``white_p = w_p^T N^-1/2 S`` and ``Tw_p = T^T
        N^-1/2 w_p`` (m, R).  Kernel path: ``white`` (P, Rp, 2F+1) as
        ``sbgemm`` writes it (row r, column 2f+c) and ``Tw`` (P, m, R);
        otherwise lists of (2F, R) and (m, R) tensors."""
        assert self.freqs is not None, "call precompute(freqs) first"
        F = self.freqs.shape[0]
        white, Tw = [], []
        for i, (blk, wp) in enumerate(zip(self.blocks, w)):
            if blk.block_noise is not None:
                raise NotImplementedError(
                    f"pulsar {self.names[i]} (index {i}) has block-diagonal "
                    "white noise (BlockNoise): "
                    "the joint null needs N^-1/2, implemented for diagonal "
                    "Nvec only")
            wp = _t64(wp, self.device)
            if wp.dim() != 2 or wp.shape[0] != blk.ntoa:
                raise ValueError(f"w[{i}] must be (ntoa, R) = ({blk.ntoa}, R),"
                                 f" got {tuple(wp.shape)}")
            nis = torch.rsqrt(blk.Nvec)
            nw = nis[:, None] * wp  # (ntoa, R)
            R = wp.shape[1]
            if self._null_kernel_path():
                Tw.append(blk.T.transpose(0, 1) @ nw)
                zero = torch.zeros(R, dtype=torch.float64, device=self.device)
                white.append(ops._basis_rhs(wp.contiguous(), nis, blk.toas,
                                            zero, self.freqs))
                continue
            wh = torch.empty((2 * F, R), dtype=torch.float64,
                             device=self.device)
            # R independent products: a realisation's value does not
            # depend on its chunk
            Tw.append(_per_column(blk.T.transpose(0, 1), nw))
            for lo in range(0, F, freq_chunk):
                hi = min(lo + freq_chunk, F)
                arg = 2.0 * math.pi * self.freqs[lo:hi, None] * blk.toas[None, :]
                wh[2 * lo:2 * hi:2] = _per_column(torch.sin(arg), nw)
                wh[2 * lo + 1:2 * hi:2] = _per_column(torch.cos(arg), nw)
            white.append(wh)
        if self._null_kernel_path():
            return torch.stack(white), torch.stack(Tw)
        return white, Tw

    def _null_combine(self, white_Tw, phiinvs, u):
        """Joint null data (D, F, P, 2, R) from :meth:`_null_white`'s pair,
        per-pulsar (D, m) or (m,) ``phiinvs`` and normals ``u_p (m, R)``:
        ``n = white - B^T Sigma_d^-1 (Tw - phi_d^-1/2 u)``.  Entries of
        ``phiinvs`` at or below zero (an improper prior, or its rounding
        when the prior comes back from a dense sigma) count as zero."""
        white, Tw = white_Tw
        rows, _ = self._rows(phiinvs)
        u = [_t64(x, self.device) for x in u]
        for i, (blk, up) in enumerate(zip(self.blocks, u)):
            if tuple(up.shape) != (blk.m, Tw[i].shape[1]):
                raise ValueError(
                    f"u[{i}] must be (m, R) = ({blk.m}, {Tw[i].shape[1]}), "
                    f"got {tuple(up.shape)}")
        P, D, F = len(rows), rows[0].shape[0], self.freqs.shape[0]
        if self._null_kernel_path():
            st = self._direct_stack
            m, R = Tw.shape[1], Tw.shape[2]
            pinv = torch.stack(rows).contiguous()  # (P, D, m)
            L, _ = ops.chol_factor(st.A, pinv, ext=self._ext)
            mp = L.shape[-1]
            U = torch.zeros((P, D, mp, R), dtype=torch.float64,
                            device=self.device)
            U[:, :, :m] = Tw[:, None] - (
                pinv.clamp_min(0.0).sqrt()[..., None] * torch.stack(u)[:, None])
            # the solver returns its own (column-major) layout
            X = torch.cholesky_solve(U.view(P * D, mp, R), L).contiguous()
            return ops.fe_null_data(white, st.RHS, X.view(P, D, mp, R))
        R_ = Tw[0].shape[1]
        n = torch.empty((D, F, P, 2, R_), dtype=torch.float64,
                        device=self.device)
        for i, (blk, pinv) in enumerate(zip(self.blocks, rows)):
            m = blk.m
            U = Tw[i][None] - pinv.clamp_min(0.0).sqrt()[..., None] * u[i][None]
            Lc = torch.linalg.cholesky(blk.TNT[None] + torch.diag_embed(pinv))
            # one solve and one product per realisation, so that a
            # realisation's value does not depend on its chunk
            X = torch.cat([torch.cholesky_solve(U[:, :, r:r + 1].contiguous(),
                                                Lc) for r in range(R_)],
                          dim=2)  # (D, m, R)
            Bt = blk.RHS[:m, :2 * F].transpose(0, 1)  # (2F, m)
            BX = _per_column(Bt, X.permute(1, 0, 2).reshape(m, D * R_))
            nd = white[i][None] - BX.reshape(2 * F, D, R_).permute(1, 0, 2)
            n[:, :, i] = nd.reshape(D, F, 2, R_)
        return n

    def null_data(self, phiinvs, nreal: int, seed: int = 0, w=None, u=None):
        """Noise-only data products of all frequencies from ONE noise
        realisation per pulsar: ``n (D, F, P, 2, R)`` with ``n[d, f, p] =
        (s_f | r)_p, (c_f | r)_p`` for ``r ~ N(0, C_{p,d})``, correlated
        across frequencies as the data are (docs/DESIGN.md section 14);
        the layout ``ops.fe_null_skymax`` takes.

        For ``r = N^1/2 w + T phi^1/2 u`` with standard normals ``w``
        (ntoa) and ``u`` (m),

            n = S^T N^-1/2 w - B^T Sigma^-1 (T^T N^-1/2 w - phi^-1/2 u),

        the engine's own data path on the direct system; ``phi^1/2`` never
        appears, so an improper prior (``phi^-1 = 0``) contributes exactly
        nothing.  ``phiinvs``: per-pulsar (m,) or (D, m) prior rows; the
        SAME ``(w, u)`` serve every draw and every frequency.

        ``w`` / ``u``: lists of (ntoa_p, R) / (m_p, R) normals that
        bypass the generator; otherwise :meth:`null_normals` draws them
        from a ``torch.Generator`` of ``seed`` on the engine's device
        (reproducible per ``(seed, nreal, device type)``).  Diagonal white
        noise only: a ``BlockNoise`` pulsar raises ``NotImplementedError``.
        On a HIP engine whose direct systems stack, the white term is the
        ``sbgemm`` kernel and the combine ``ops.fe_null_data``; otherwise
        both are torch ops on the engine's device."""
        assert self.freqs is not None, "call precompute(freqs) first"
        if (w is None) != (u is None):
            raise ValueError("give both w and u, or neither")
        if w is None:
            gen = torch.Generator(device=self.device)
            gen.manual_seed(int(seed))
            w, u = self.null_normals(nreal, gen)
        elif any(x.shape[1] != int(nreal) for x in list(w) + list(u)):
            raise ValueError(f"w and u must hold nreal = {nreal} columns")
        return self._null_combine(self._null_white(w), phiinvs, u)

    @staticmethod
    def _dense(system: SolveSystem, pinv):
        """(D, m, m) ``A + diag(d)`` of one pulsar's system for the
        (D, m) phiinv rows ``pinv``."""
        return system.A[None] + torch.diag_embed(
            system.diag(pinv[:, system.var]))

    def sweep_products_hip(self, phiinvs, draw_chunk: int = 32,
                           compressed: bool = False) -> torch.Tensor:
        """:meth:`sweep_products` on the HIP solve: the same five
        corrected products, stored un-collapsed by the products mode of
        the trsm kernels.

        ``phiinvs``: per-pulsar (m,) or (D, m) diagonal phi^-1; returns
        the (P, 5, F) / (P, D, 5, F) device tensor.  When every pulsar
        shares one basis size with ``pad16(m) <= 128`` this is ONE
        ``chol_batch`` and ONE ``trsm_prods`` launch per draw chunk
        across all pulsars, on the direct (uncompressed) system.
        Otherwise (CPU/eager engine, ragged bases, larger m) it returns
        ``self.sweep_products(phiinvs=...)``.

        ``compressed``: solve the Schur-compressed systems instead
        (:meth:`enable_draw_compression`), at the variable dimension:

        * stacked compression: one ``chol_batch`` per draw chunk on the
          stacked system, then ``trsm_prods_store`` (the draw-looping
          kernel) where :meth:`_draw_loop_solve` holds and
          ``trsm_prods`` on the same padded system otherwise;
        * no stack (ragged variable dimensions, or pulsars that lost
          compression): per pulsar, its compressed system where it has
          one and its direct system otherwise, on the HIP kernels while
          that system's padded dimension is within ``MAX_MP_CHOL`` and
          eager beyond;
        * nothing compressed: the same as ``compressed=False``.

        No limit on ``m`` and no common basis size is needed.  The
        per-draw margin is the caller's business, as in :meth:`sweep`."""
        assert self.freqs is not None, "call precompute(freqs) first"
        if compressed and not self._use_hip:
            return self.sweep_products(phiinvs=phiinvs, compressed=True)
        compressed = compressed and any(
            blk.comp is not None for blk in self.blocks)
        st = self._comp_stack if compressed else self._direct_stack
        if st is None:  # the compressed systems also solve one by one
            eager = not compressed
        else:
            eager = ops.pad16(st.A.shape[-1]) > ops.MAX_MP_CHOL
        if eager:
            return self.sweep_products(phiinvs=phiinvs, compressed=compressed)
        rows, batched = self._rows(phiinvs)
        out = torch.empty(
            (len(rows), rows[0].shape[0], 5, self.freqs.shape[0]),
            dtype=torch.float64, device=self.device)
        if st is not None:
            # one factor and one solve launch per draw chunk
            self._solve_chunks(st, rows, draw_chunk, out, prods=True)
            return out if batched else out[:, 0]
        # compressed without a stack: per pulsar, each on its own system
        for i, (blk, p) in enumerate(zip(self.blocks, rows)):
            sy = blk.comp if blk.comp is not None else blk.direct
            if ops.pad16(sy.A.shape[-1]) > ops.MAX_MP_CHOL:
                out[i] = torch.stack(
                    _eager_products(sy, self._dense(sy, p)), dim=1)
            else:
                self._solve_chunks(sy, p, draw_chunk, out[i], prods=True)
        return out if batched else out[:, 0]
