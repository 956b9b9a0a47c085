"""GPU kernel numerics: every HIP kernel vs a plain PyTorch fp64
reference on-device, plus end-to-end HIP-vs-eager and
bitwise-determinism checks."""

import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def _ext():
    from fastfp_amd import ops

    ops.require_hip()
    from fastfp_amd.ops import _fastfp_hip

    return _fastfp_hip


def _rand_problem(seed=0, ntoa=333, m=37, F=29, D=5):
    rng = np.random.default_rng(seed)
    toas = torch.as_tensor(
        np.sort(rng.uniform(0, 4e8, ntoa)), dtype=torch.float64, device=DEV
    )
    nvec = torch.as_tensor(
        rng.uniform(0.5, 2.0, ntoa) * 1e-12, dtype=torch.float64, device=DEV
    )
    r = torch.as_tensor(
        rng.normal(0, 1e-6, ntoa), dtype=torch.float64, device=DEV
    )
    T = torch.as_tensor(
        rng.normal(size=(ntoa, m)), dtype=torch.float64, device=DEV
    )
    freqs = torch.as_tensor(
        np.linspace(3e-9, 5e-8, F), dtype=torch.float64, device=DEV
    )
    phiinv = torch.as_tensor(
        rng.uniform(0.5, 2.0, (D, m)) * 1e10, dtype=torch.float64, device=DEV
    )
    return toas, nvec, r, T, freqs, phiinv


def test_sigdots_vs_torch():
    ext = _ext()
    toas, nvec, r, T, freqs, _ = _rand_problem()
    ninv = 1.0 / nvec
    nr = r / nvec
    sNs, sNr = ext.sigdots(toas, ninv.contiguous(), nr.contiguous(), freqs)
    arg = 2 * math.pi * freqs[:, None] * toas[None, :]
    S, C = torch.sin(arg), torch.cos(arg)
    torch.testing.assert_close(sNs[0], (S * S * ninv).sum(1), rtol=1e-12, atol=1e-6)
    torch.testing.assert_close(sNs[1], (C * C * ninv).sum(1), rtol=1e-12, atol=1e-6)
    torch.testing.assert_close(sNs[2], (S * C * ninv).sum(1), rtol=1e-10, atol=1e-4)
    torch.testing.assert_close(sNr[0], S @ nr, rtol=1e-10, atol=1e-8)
    torch.testing.assert_close(sNr[1], C @ nr, rtol=1e-10, atol=1e-8)


@pytest.mark.parametrize("F,ntoa,m", [(29, 333, 37), (70, 150, 37),
                                      (200, 2000, 37), (40, 500, 300)])
def test_sbgemm_vs_torch(F, ntoa, m):
    from fastfp_amd import ops

    toas, nvec, r, T, freqs, _ = _rand_problem(F=F, ntoa=ntoa, m=m)
    ninv = 1.0 / nvec
    TNr = (T / nvec[:, None]).T @ r
    RHS, sNs, sNr = ops.freq_precompute(toas, nvec, r, T, TNr, freqs)
    m = T.shape[1]
    mp = RHS.shape[0]
    assert mp % 16 == 0
    arg = 2 * math.pi * freqs[:, None] * toas[None, :]
    S = torch.sin(arg) * ninv[None, :]
    C = torch.cos(arg) * ninv[None, :]
    want_s = S @ T  # (F, m)
    want_c = C @ T
    # fixed-order kernel sum vs torch matmul order: fp64 roundoff-level
    torch.testing.assert_close(RHS[:m, 0:-1:2], want_s.T, rtol=1e-9, atol=1e-9)
    torch.testing.assert_close(RHS[:m, 1:-1:2], want_c.T, rtol=1e-9, atol=1e-9)
    assert (RHS[m:, :] == 0).all()
    torch.testing.assert_close(RHS[:m, -1], TNr, rtol=1e-12, atol=0.0)


@pytest.mark.parametrize("m,mp", [(37, 48), (100, 112), (120, 128)])
def test_chol_batch_vs_torch(m, mp):
    ext = _ext()
    toas, nvec, r, T, freqs, phiinv = _rand_problem(m=m)
    TN = T / nvec[:, None]
    TNT = (T.T @ TN).contiguous()
    L, invd = ext.chol_batch(TNT, phiinv, mp)
    D = phiinv.shape[0]
    sigma = TNT[None] + torch.diag_embed(phiinv)
    want = torch.linalg.cholesky(sigma)
    got = torch.tril(L[:, :m, :m])
    torch.testing.assert_close(got, want, rtol=1e-9, atol=1e-9)
    # pad block identity
    assert (torch.tril(L[:, m:, m:]) == torch.eye(mp - m, device=DEV)).all()
    # inverted diagonal blocks
    nb = mp // 16
    for kb in range(nb):
        blk = torch.tril(L[:, kb * 16 : kb * 16 + 16, kb * 16 : kb * 16 + 16])
        inv = torch.linalg.solve_triangular(
            blk, torch.eye(16, dtype=torch.float64, device=DEV)[None].expand(D, 16, 16),
            upper=False,
        )
        torch.testing.assert_close(
            torch.tril(invd[:, kb]), torch.tril(inv), rtol=1e-8, atol=1e-8
        )


@pytest.mark.parametrize("m", [37, 120])  # NBT=3 and NBT=8 (only DPG=1 exists)
def test_trsm_fp_accum_vs_eager(m):
    from fastfp_amd import ops

    toas, nvec, r, T, freqs, phiinv = _rand_problem(F=100, D=7, m=m)
    m = T.shape[1]
    F = freqs.shape[0]
    D = phiinv.shape[0]
    TN = T / nvec[:, None]
    TNT = (T.T @ TN).contiguous()
    TNr = TN.T @ r
    RHS, sNs, sNr = ops.freq_precompute(toas, nvec, r, T, TNr, freqs)

    fp = torch.zeros((D, F), dtype=torch.float64, device=DEV)
    ops.chol_trsm_fp_accum(TNT, phiinv, RHS, sNs, sNr, fp)

    # eager reference (same restructured math, torch linalg)
    sigma = TNT[None] + torch.diag_embed(phiinv)
    Lr = torch.linalg.cholesky(sigma)
    RHSe = torch.cat([RHS[:m, :-1], TNr[:, None]], dim=1)
    W = torch.linalg.solve_triangular(
        Lr, RHSe[None].expand(D, -1, -1), upper=False
    )
    wu = W[:, :, -1]
    Ws, Wc = W[:, :, 0:-1:2], W[:, :, 1:-1:2]
    M11 = sNs[0][None] - (Ws * Ws).sum(1)
    M22 = sNs[1][None] - (Wc * Wc).sum(1)
    M12 = sNs[2][None] - (Ws * Wc).sum(1)
    N1 = sNr[0][None] - torch.einsum("dmf,dm->df", Ws, wu)
    N2 = sNr[1][None] - torch.einsum("dmf,dm->df", Wc, wu)
    det = M11 * M22 - M12 * M12
    want = 0.5 * (N1 * N1 * M22 - 2 * N1 * N2 * M12 + N2 * N2 * M11) / det
    torch.testing.assert_close(fp, want, rtol=1e-7, atol=1e-9)

    # accumulation: second call doubles
    fp2 = fp.clone()
    ops.chol_trsm_fp_accum(TNT, phiinv, RHS, sNs, sNr, fp2)
    torch.testing.assert_close(fp2, 2 * fp, rtol=1e-12, atol=0.0)


def test_engine_gpu_matches_cpu_eager():
    from fastfp_amd import FpEngine, get_mats_nmfp, initialize_pta, make_synthetic_pta
    from fastfp_amd.nmfp import NMFp

    psrs = make_synthetic_pta(npsr=3, ntoa=500, ntm=5, seed=3)
    noise = {"gw_gamma": 13.0 / 3.0, "gw_log10_A": float(np.log10(2e-15))}
    for p in psrs:
        noise[f"{p.name}_red_noise_gamma"] = 4.0
        noise[f"{p.name}_red_noise_log10_A"] = -14.5
    pta = initialize_pta(psrs, noise, inc_cp=True, rn_comps=6, gwb_comps=6)
    TNTs, Nvecs, Ts = get_mats_nmfp(pta, noise)
    D = 4
    rng = np.random.default_rng(7)
    samples = {}
    for name in pta.params:
        samples[name] = (
            rng.uniform(2, 6, D) if name.endswith("gamma") else rng.uniform(-16, -14, D)
        )
    nm = NMFp(psrs, pta.rn_containers)
    freqs = np.linspace(4e-9, 6e-8, 33)
    cpu = nm.sweep(freqs, samples, Nvecs, Ts, device="cpu")
    for c in pta.rn_containers:
        c.to(DEV)
    gpu = nm.sweep(freqs, samples, Nvecs, Ts, device=DEV)
    np.testing.assert_allclose(gpu, cpu, rtol=1e-8)


def test_gpu_determinism_bitwise():
    from fastfp_amd import ops

    toas, nvec, r, T, freqs, phiinv = _rand_problem(F=65, D=6)
    TN = T / nvec[:, None]
    TNT = (T.T @ TN).contiguous()
    TNr = TN.T @ r
    outs = []
    for _ in range(2):
        RHS, sNs, sNr = ops.freq_precompute(toas, nvec, r, T, TNr, freqs)
        fp = torch.zeros((phiinv.shape[0], freqs.shape[0]), dtype=torch.float64, device=DEV)
        ops.chol_trsm_fp_accum(TNT, phiinv, RHS, sNs, sNr, fp)
        outs.append(fp.cpu().numpy())
    np.testing.assert_array_equal(outs[0], outs[1])


def test_native_extension_is_loaded():
    """Guard against silent eager fallback on GPU boxes."""
    from fastfp_amd import ops

    assert ops.hip_available(), "HIP extension must be importable on a GPU box"
    from fastfp_amd.ops import _fastfp_hip

    assert "fastfp_amd" in _fastfp_hip.__file__


def test_sigdots_block_kernel_vs_eager():
    """Sherman–Morrison block-N dots kernel vs the CPU eager precompute
    — on a PTA with LARGE epochs (>32 TOAs/epoch, beyond the round-1
    block-Cholesky cap)."""
    from fastfp_amd import make_synthetic_pta
    from fastfp_amd.blocknoise import BlockNoise
    from fastfp_amd.engine import FpEngine

    # dense-in-time TOAs -> day-buckets of ~40 TOAs
    psrs = make_synthetic_pta(npsr=1, ntoa=300, tspan_yr=0.02, ntm=3, seed=11)
    psr = psrs[0]
    noise = {}
    for b in np.unique(psr.backend_flags):
        noise[f"{psr.name}_basis_ecorr_{b}_log10_ecorr"] = -6.4
    bn = BlockNoise(psr, noise)
    assert bn.max_block > 32, "test needs an epoch beyond the old cap"
    freqs = np.linspace(4e-9, 6e-8, 11)
    T = np.asarray(psr.Mmat, dtype=np.float64)
    eng_gpu = FpEngine([psr], [bn], [T], device=DEV)
    eng_gpu.precompute(freqs)
    eng_cpu = FpEngine([psr], [bn], [T], device="cpu")
    eng_cpu.precompute(freqs)
    for attr in ("sNs", "sNr", "RHS"):
        got = getattr(eng_gpu.blocks[0], attr).cpu().numpy()
        want = getattr(eng_cpu.blocks[0], attr).numpy()
        got = got[: want.shape[0]]  # GPU RHS rows padded to mp
        np.testing.assert_allclose(got, want, rtol=1e-9, atol=1e-24,
                                   err_msg=attr)


def test_engine_blocknoise_gpu_matches_cpu():
    from fastfp_amd import FastFp, get_mats_fp, initialize_pta, make_synthetic_pta

    psrs = make_synthetic_pta(npsr=2, ntoa=400, ntm=4, seed=12)
    noise = {}
    for p in psrs:
        noise[f"{p.name}_red_noise_gamma"] = 4.0
        noise[f"{p.name}_red_noise_log10_A"] = -14.5
        for b in np.unique(p.backend_flags):
            noise[f"{p.name}_basis_ecorr_{b}_log10_ecorr"] = -6.5
    pta = initialize_pta(psrs, noise, inc_cp=False, rn_comps=5,
                         ecorr_kernel=True)
    Nvecs, Ts, sigmas = get_mats_fp(pta, noise)
    freqs = np.linspace(4e-9, 6e-8, 17)
    fp_obj = FastFp(psrs)
    cpu = fp_obj.sweep(freqs, Nvecs, Ts, sigmas, device="cpu")
    gpu = fp_obj.sweep(freqs, Nvecs, Ts, sigmas, device=DEV)
    np.testing.assert_allclose(gpu, cpu, rtol=1e-8)


def test_nmfp_large_m_ecorr_gpu_compressed():
    """GP-ECORR model with basis size m > 128: precompute is M-tiled,
    the per-draw solve runs compressed at the variable-bin dimension."""
    from fastfp_amd import get_mats_nmfp, initialize_pta, make_synthetic_pta
    from fastfp_amd.nmfp import NMFp

    psrs = make_synthetic_pta(npsr=2, ntoa=700, ntm=5, seed=21)
    noise = {}
    for p in psrs:
        noise[f"{p.name}_red_noise_gamma"] = 4.0
        noise[f"{p.name}_red_noise_log10_A"] = -14.5
        for b in np.unique(p.backend_flags):
            noise[f"{p.name}_basis_ecorr_{b}_log10_ecorr"] = -6.5
            noise[f"{p.name}_{b}_efac"] = 1.0
    pta = initialize_pta(psrs, noise, inc_cp=False, rn_comps=6,
                         simple_wn=True, inc_ecorr=True)
    TNTs, Nvecs, Ts = get_mats_nmfp(pta, noise)
    assert max(T.shape[1] for T in Ts) > 128, "test needs m > 128"
    D = 3
    rng = np.random.default_rng(5)
    samples = {
        n: (rng.uniform(2, 6, D) if n.endswith("gamma")
            else rng.uniform(-16, -14, D))
        for n in pta.params
    }
    nm = NMFp(psrs, pta.rn_containers)
    freqs = np.linspace(4e-9, 5e-8, 9)
    cpu = nm.sweep(freqs, samples, Nvecs, Ts, device="cpu")
    for c in pta.rn_containers:
        c.to(DEV)
    gpu = nm.sweep(freqs, samples, Nvecs, Ts, device=DEV)
    np.testing.assert_allclose(gpu, cpu, rtol=1e-7)


def test_chol_full_dynamic_range_gpu():
    """Sigma with the production prior spread: 1e-40 tm bins against
    ~1e12-1e18 red-noise phi^-1."""
    ext = _ext()
    rng = np.random.default_rng(31)
    ntoa, m, D = 400, 24, 6
    T = torch.as_tensor(rng.normal(size=(ntoa, m)), dtype=torch.float64, device=DEV)
    nvec = torch.full((ntoa,), 1e-12, dtype=torch.float64, device=DEV)
    TNT = (T.T @ (T / nvec[:, None])).contiguous()
    phiinv = torch.empty((D, m), dtype=torch.float64, device=DEV)
    phiinv[:, :8] = 1e-40  # improper-flat timing-model prior
    phiinv[:, 8:] = torch.as_tensor(
        10.0 ** rng.uniform(12, 18, (D, m - 8)), device=DEV
    )
    mp = 32
    L, invd = ext.chol_batch(TNT, phiinv, mp)
    want = torch.linalg.cholesky(TNT[None] + torch.diag_embed(phiinv))
    torch.testing.assert_close(
        torch.tril(L[:, :m, :m]), want, rtol=1e-9, atol=0.0
    )


def test_fastfp_sweep_large_m_gpu():
    """Plain Fp sweep with m > 128 (GP-ECORR) on GPU auto-routes
    through the compressed path."""
    from fastfp_amd import FastFp, get_mats_fp, initialize_pta, make_synthetic_pta

    psrs = make_synthetic_pta(npsr=2, ntoa=700, ntm=5, seed=22)
    noise = {}
    for p in psrs:
        noise[f"{p.name}_red_noise_gamma"] = 4.0
        noise[f"{p.name}_red_noise_log10_A"] = -14.5
        for b in np.unique(p.backend_flags):
            noise[f"{p.name}_basis_ecorr_{b}_log10_ecorr"] = -6.5
    pta = initialize_pta(psrs, noise, inc_cp=False, rn_comps=6, inc_ecorr=True)
    Nvecs, Ts, sigmas = get_mats_fp(pta, noise)
    assert max(T.shape[1] for T in Ts) > 128
    freqs = np.linspace(4e-9, 5e-8, 11)
    fp_obj = FastFp(psrs, pta)
    cpu = fp_obj.sweep(freqs, Nvecs, Ts, sigmas, device="cpu")
    gpu = fp_obj.sweep(freqs, Nvecs, Ts, sigmas, device=DEV)
    np.testing.assert_allclose(gpu, cpu, rtol=1e-6)


def test_engine_direct_stacked_gpu_matches_cpu():
    """Direct (uncompressed) pulsar-stacked sweep on GPU vs CPU eager."""
    from fastfp_amd import FpEngine, get_mats_nmfp, initialize_pta, make_synthetic_pta

    psrs = make_synthetic_pta(npsr=3, ntoa=400, ntm=4, seed=33, ragged=False)
    noise = {"gw_gamma": 13.0 / 3.0, "gw_log10_A": float(np.log10(2e-15))}
    for p in psrs:
        noise[f"{p.name}_red_noise_gamma"] = 4.0
        noise[f"{p.name}_red_noise_log10_A"] = -14.5
    pta = initialize_pta(psrs, noise, inc_cp=True, rn_comps=6, gwb_comps=6)
    TNTs, Nvecs, Ts = get_mats_nmfp(pta, noise)
    D = 5
    rng = np.random.default_rng(3)
    pars = {
        n: (rng.uniform(2, 6, D) if n.endswith("gamma")
            else rng.uniform(-16, -14, D))
        for n in pta.params
    }
    phiinvs = [c.get_phiinv(pars).numpy() for c in pta.rn_containers]
    freqs = np.linspace(4e-9, 6e-8, 21)

    eng_c = FpEngine(psrs, Nvecs, Ts, device="cpu").precompute(freqs)
    want = eng_c.sweep(phiinvs=phiinvs).numpy()

    eng_g = FpEngine(psrs, Nvecs, Ts, device=DEV).precompute(freqs)
    assert eng_g._direct_stack is not None, "stack should engage (same m)"
    got = eng_g.sweep(phiinvs=phiinvs).cpu().numpy()
    np.testing.assert_allclose(got, want, rtol=1e-8)
    # draw_chunk=2 over D=5: the factor/solve pipeline with ping-pong
    # buffers, ending in a one-draw tail chunk
    got = eng_g.sweep(phiinvs=phiinvs, draw_chunk=2).cpu().numpy()
    np.testing.assert_allclose(got, want, rtol=1e-8)


def test_compressed_stacked_large_mv_multichunk_gpu():
    """Compressed stacked sweep whose variable dimension exceeds the
    LDS-resident Cholesky (mv = 140 > 128) over more than one draw
    chunk: it must take the un-pipelined rocSOLVER-factored loop, not
    the chol_batch pipeline.  Compared with the CPU engine's compressed
    sweep of the same draws."""
    from fastfp_amd import FpEngine, get_mats_nmfp, initialize_pta, \
        make_synthetic_pta

    psrs = make_synthetic_pta(npsr=2, ntoa=500, ntm=10, seed=51,
                              ragged=False)
    noise = {"gw_gamma": 13.0 / 3.0, "gw_log10_A": float(np.log10(2e-15))}
    for p in psrs:
        noise[f"{p.name}_red_noise_gamma"] = 4.0
        noise[f"{p.name}_red_noise_log10_A"] = -14.5
    # ntm 10 + 2*70 rn = 150 columns, 140 of them variable
    pta = initialize_pta(psrs, noise, inc_cp=True, rn_comps=70,
                         gwb_comps=10)
    TNTs, Nvecs, Ts = get_mats_nmfp(pta, noise)
    D = 3
    rng = np.random.default_rng(5)
    pars = {
        n: (rng.uniform(2, 6, D) if n.endswith("gamma")
            else rng.uniform(-16, -14, D))
        for n in pta.params
    }
    phiinvs = [c.get_phiinv(pars).numpy() for c in pta.rn_containers]
    freqs = np.linspace(4e-9, 6e-8, 13)
    var_slices = [c.var_slice for c in pta.rn_containers]
    fixed = [c.get_phiinv(noise) for c in pta.rn_containers]

    results = {}
    for dev in ("cpu", DEV):
        eng = FpEngine(psrs, Nvecs, Ts, device=dev).precompute(freqs)
        eng.enable_draw_compression(var_slices, fixed)
        print(dev, "probe errors",
              [getattr(b, "probe_err", None) for b in eng.blocks])
        assert all(blk.comp is not None for blk in eng.blocks)
        assert all(blk.comp.A.shape[0] == 140 for blk in eng.blocks)
        results[dev] = eng.sweep(phiinvs=phiinvs, draw_chunk=2).cpu().numpy()
    assert eng._comp_stack is not None
    cpu, gpu = results["cpu"], results[DEV]
    err = np.abs(gpu - cpu).max() / np.abs(cpu).max()
    print("max|gpu - cpu| / max|cpu| =", err)
    assert err < 1e-6


def test_low_margin_draws_compressed_gpu_vs_direct():
    """Uniform-prior tail draws (margin just above the 1.5 guard) on
    the GPU compressed kernels vs the GPU direct path — the accuracy
    that justifies the r02 margin-threshold change."""
    from fastfp_amd import FpEngine, get_mats_nmfp, initialize_pta, \
        make_synthetic_pta
    from fastfp_amd.noise import batch_phiinv

    psrs = make_synthetic_pta(npsr=3, ntoa=1500, ntm=10, seed=61)
    noise = {"gw_gamma": 13.0 / 3.0, "gw_log10_A": float(np.log10(2e-15))}
    for p in psrs:
        noise[f"{p.name}_red_noise_gamma"] = 13.0 / 3.0
        noise[f"{p.name}_red_noise_log10_A"] = -14.5
    pta = initialize_pta(psrs, noise, inc_cp=True, rn_comps=20, gwb_comps=20)
    TNTs, Nvecs, Ts = get_mats_nmfp(pta, noise)
    for c in pta.rn_containers:
        c.to(DEV)
    D = 4
    samples = {
        n: (np.array([6.5, 6.0, 5.0, 13 / 3]) if n.endswith("gamma")
            else np.array([-13.5, -13.8, -14.0, -14.5]))
        for n in pta.params
    }
    freqs = np.linspace(3e-9, 5e-8, 40)
    eng = FpEngine(psrs, Nvecs, Ts, device=DEV)
    eng.precompute(freqs)
    eng.enable_draw_compression(
        [c.var_slice for c in pta.rn_containers],
        [c.get_phiinv(noise).to(DEV) for c in pta.rn_containers],
    )
    assert all(blk.comp is not None for blk in eng.blocks)
    piv = [p if p.dim() == 2 else p[None]
           for p in batch_phiinv(pta.rn_containers, samples)]
    margin = eng.compression_margin(piv)
    assert margin > 1.5, margin
    comp = eng.sweep(phiinvs=piv).cpu().numpy()
    eng.disable_draw_compression()
    eng._stack_direct()
    direct = eng.sweep(phiinvs=piv).cpu().numpy()
    scale = np.abs(direct).max()
    assert np.isfinite(comp).all()
    assert np.abs(comp - direct).max() / scale < 1e-6


def test_direct_sweep_large_m_gpu():
    """DIRECT (uncompressed) GPU sweep at basis size 128 < m <= 256:
    the rocSOLVER-factored + diag_inv + register-resident trsm path
    (round-1 cap lifted).  Validated against the CPU eager engine."""
    from fastfp_amd import FpEngine, get_mats_nmfp, initialize_pta, \
        make_synthetic_pta

    psrs = make_synthetic_pta(npsr=2, ntoa=500, ntm=10, seed=51,
                              ragged=False)
    noise = {"gw_gamma": 13.0 / 3.0, "gw_log10_A": float(np.log10(2e-15))}
    for p in psrs:
        noise[f"{p.name}_red_noise_gamma"] = 4.0
        noise[f"{p.name}_red_noise_log10_A"] = -14.5
    # ntm 10 + 2*80 rn + 2*10 gwb = 190 columns
    pta = initialize_pta(psrs, noise, inc_cp=True, rn_comps=80,
                         gwb_comps=10)
    TNTs, Nvecs, Ts = get_mats_nmfp(pta, noise)
    assert 128 < max(T.shape[1] for T in Ts) <= 256
    D = 4
    rng = np.random.default_rng(5)
    pars = {
        n: (rng.uniform(2, 6, D) if n.endswith("gamma")
            else rng.uniform(-16, -14, D))
        for n in pta.params
    }
    phiinvs = [c.get_phiinv(pars).numpy() for c in pta.rn_containers]
    freqs = np.linspace(4e-9, 6e-8, 13)

    eng_c = FpEngine(psrs, Nvecs, Ts, device="cpu").precompute(freqs)
    want = eng_c.sweep(phiinvs=phiinvs).numpy()
    eng_g = FpEngine(psrs, Nvecs, Ts, device=DEV).precompute(freqs)
    got = eng_g.sweep(phiinvs=phiinvs).cpu().numpy()
    np.testing.assert_allclose(got, want, rtol=1e-7)

    # plain-Fp entry point (sigmas contract) through the same path
    from fastfp_amd import FastFp, get_mats_fp

    noise1 = dict(noise)
    for p in psrs:
        noise1[f"{p.name}_red_noise_gamma"] = 4.2
        noise1[f"{p.name}_red_noise_log10_A"] = -14.2
    Nv2, Ts2, sigmas = get_mats_fp(pta, noise1)
    fp_obj = FastFp(psrs, pta)
    cpu = fp_obj.sweep(freqs, Nv2, Ts2, sigmas, device="cpu")
    gpu = fp_obj.sweep(freqs, Nv2, Ts2, sigmas, device=DEV)
    np.testing.assert_allclose(gpu, cpu, rtol=1e-7)


def test_graphed_nmfp_sweep_matches_eager(monkeypatch):
    """The CLI's hipGraph-replayed batch sweep (NMFp._sweep_graphed)
    must reproduce the eager sweep bitwise, including across repeated
    replays with different draw batches, and must recompute
    prior-corner draws through the direct path."""
    from fastfp_amd import FpEngine, get_mats_nmfp, initialize_pta, \
        make_synthetic_pta
    from fastfp_amd.nmfp import NMFp

    psrs = make_synthetic_pta(npsr=3, ntoa=800, ntm=8, seed=71)
    noise = {"gw_gamma": 13.0 / 3.0, "gw_log10_A": float(np.log10(2e-15))}
    for p in psrs:
        noise[f"{p.name}_red_noise_gamma"] = 13.0 / 3.0
        noise[f"{p.name}_red_noise_log10_A"] = -14.5
    pta = initialize_pta(psrs, noise, inc_cp=True, rn_comps=12, gwb_comps=12)
    TNTs, Nvecs, Ts = get_mats_nmfp(pta, noise)
    for c in pta.rn_containers:
        c.to(DEV)
    eng = FpEngine(psrs, Nvecs, Ts, device=DEV)
    freqs = np.linspace(3e-9, 5e-8, 30)
    eng.precompute(freqs)
    eng.enable_draw_compression(
        [c.var_slice for c in pta.rn_containers],
        [c.get_phiinv(noise).to(DEV) for c in pta.rn_containers],
    )
    assert eng._comp_stack is not None
    nm = NMFp(psrs, pta.rn_containers)
    rng = np.random.default_rng(9)
    D = 16
    batches = []
    for _ in range(3):
        batches.append({
            n: (rng.uniform(2, 6, D) if n.endswith("gamma")
                else rng.uniform(-16, -14, D))
            for n in pta.params
        })
    # one batch includes a prior-corner draw (direct-path overwrite)
    for n in pta.params:
        batches[2][n][3] = 9.0 if n.endswith("gamma") else -12.5

    monkeypatch.setenv("FASTFP_NO_GRAPH", "1")
    eager = [nm.sweep(freqs, b, Nvecs, Ts, engine=eng) for b in batches]
    monkeypatch.delenv("FASTFP_NO_GRAPH")
    graphed = [nm.sweep(freqs, b, Nvecs, Ts, engine=eng) for b in batches]
    assert nm._graphs, "graph path should have engaged"
    for a, b in zip(eager, graphed):
        np.testing.assert_array_equal(a, b)


def test_graph_captured_sweep_bitwise_equals_eager():
    """A hipGraph-captured sweep (the bench's step structure) must
    reproduce the eager sweep BITWISE on replay."""
    from fastfp_amd import FpEngine, get_mats_nmfp, initialize_pta, make_synthetic_pta
    from fastfp_amd.noise import batch_phiinv, check_batch_homogeneous

    psrs = make_synthetic_pta(npsr=3, ntoa=400, ntm=5, seed=41)
    noise = {"gw_gamma": 13.0 / 3.0, "gw_log10_A": float(np.log10(2e-15))}
    for p in psrs:
        noise[f"{p.name}_red_noise_gamma"] = 4.0
        noise[f"{p.name}_red_noise_log10_A"] = -14.5
    pta = initialize_pta(psrs, noise, inc_cp=True, rn_comps=5, gwb_comps=5)
    TNTs, Nvecs, Ts = get_mats_nmfp(pta, noise)
    for c in pta.rn_containers:
        c.to(DEV)
    eng = FpEngine(psrs, Nvecs, Ts, device=DEV)
    freqs = np.linspace(4e-9, 6e-8, 40)
    eng.precompute(freqs)
    eng.enable_draw_compression(
        [c.var_slice for c in pta.rn_containers],
        [c.get_phiinv(noise) for c in pta.rn_containers],
    )
    D = 12
    rng = np.random.default_rng(1)
    pool = {
        n: torch.as_tensor(
            rng.uniform(2, 6, D) if n.endswith("gamma")
            else rng.uniform(-16, -14, D),
            dtype=torch.float64, device=DEV,
        )
        for n in pta.params
    }
    homog = check_batch_homogeneous(pta.rn_containers)
    fp_accum = torch.zeros((D, 40), dtype=torch.float64, device=DEV)

    def step():
        phiinvs = batch_phiinv(pta.rn_containers, pool, homogeneous=homog)
        fp_accum.zero_()
        eng.sweep(phiinvs=phiinvs, draw_chunk=8, accumulate_to=fp_accum)

    step()
    torch.cuda.synchronize()
    eager = fp_accum.cpu().numpy().copy()

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step()
    torch.cuda.current_stream().wait_stream(side)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        step()
    g.replay()
    torch.cuda.synchronize()
    np.testing.assert_array_equal(fp_accum.cpu().numpy(), eager)


def test_probe_keeps_compression_at_bench_conditioning():
    """GPU regression guard for the compression-precompute accuracy:
    at the benchmark's conditioning (rn 30 + gwb 14 components, dense
    TOA coverage) the enable-time probe must keep EVERY pulsar on the
    compressed path.  This failed when the K/M0/N0/G setup ran through
    rocBLAS solve_triangular (inversion-based, ~1e-4 spectrum-scale
    error) instead of CPU LAPACK — docs/TUNING_NOTES.md."""
    from fastfp_amd import FpEngine, get_mats_nmfp, initialize_pta, \
        make_synthetic_pta

    # the EXACT bench pulsars that failed the probe in round 2 with the
    # old jitter_rel=1e-10 (probe errors 1.0-1.8e-5 > tol, conditioning
    # cond(Sigma_0)*eps — fixed by jitter_rel=1e-8), plus two that
    # always passed
    psrs_all = make_synthetic_pta(npsr=67, ntoa=5000, tspan_yr=15.0,
                                  ntm=60, seed=1234, ragged=True)
    keep = [0, 1, 10, 13, 20, 26, 66]
    noise = {"gw_gamma": 13.0 / 3.0, "gw_log10_A": float(np.log10(2e-15))}
    for p in psrs_all:
        noise[f"{p.name}_red_noise_gamma"] = 13.0 / 3.0
        noise[f"{p.name}_red_noise_log10_A"] = -14.5
    pta = initialize_pta(psrs_all, noise, inc_cp=True, rn_comps=30,
                         gwb_comps=30)
    TNTs, Nvecs, Ts = get_mats_nmfp(pta, noise)
    psrs = [psrs_all[i] for i in keep]
    conts = [pta.rn_containers[i] for i in keep]
    eng = FpEngine(psrs, [Nvecs[i] for i in keep], [Ts[i] for i in keep],
                   device=DEV)
    eng.precompute(np.arange(1, 1001) / pta.Tspan)
    probe = {k: v for k, v in noise.items() if k in pta.params}
    eng.enable_draw_compression(
        [c.var_slice for c in conts],
        [c.get_phiinv(probe).to(DEV) for c in conts],
    )
    errs = [getattr(b, "probe_err", float("nan")) for b in eng.blocks]
    kept_n = sum(blk.comp is not None for blk in eng.blocks)
    assert kept_n == len(eng.blocks), \
        f"probe disabled compression on {len(eng.blocks) - kept_n} pulsars " \
        f"(errors {['%.1e' % e for e in errs]})"
    assert eng._comp_stack is not None, "stacked compressed path must form"
    # the jitter_rel=1e-8 conditioning fix should leave a wide margin
    # below the 1e-5 tol, not a marginal pass
    assert max(errs) < 2e-6, f"probe errors regressed: {errs}"
