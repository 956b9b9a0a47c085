"""Isolated micro-benchmarks of the hot HIP kernels on one MI355X.

Usage (GPU box): python tools/kernel_bench.py
Prints per-kernel wall time and fp64 TFLOP/s at the NMFp bench shape.

    python tools/kernel_bench.py fe [P D F nsky m]

    python tools/kernel_bench.py stacked [P D F m]

times the two solve kernels of the stacked compressed sweep
(trsm_fp_accum, trsm_fp_store); defaults P=67, D=1024, F=1000, m=60.
Where m is short of mp by 4 or more it also times trsm_fp_store on the
same system padded in front, with lead = 0 and with the skipped k-steps.

    python tools/kernel_bench.py factor [P D m]

times the factor kernel alone (chol_batch_into) at the stacked shape;
defaults P=67, D=1024, m=60 (mp = 64).

times the Fe-on-device kernels (trsm_prods, fe_assemble, fe_skymax,
fe_amplitudes at the argmax);
defaults P=67, D=256, F=200, nsky=768, m=120.  It also times the
products solve at the compressed shape (m / 2 variable columns padded in
front to mp, gsign = -1): trsm_prods and trsm_prods_store on the same
padded system.  Last it times the null sky maximum (fe_null_skymax, D = 1,
R = 1024 realisations, with 1, 2 and 4 realisation tiles per workgroup,
and its factor pass fe_mfactor alone) in rounds alternated with the route
that needs no new kernel: fe_skymax on products replicated to (P, R, 5, F)
with the realisations in the planes sr, cr.

    python tools/kernel_bench.py nulldata [P D F R m]

times the joint-null combine (fe_null_data) in rounds alternated with
the torch route to the same array (baddbmm + permuting copy); defaults
P=67, D=1, F=200, R=1024, m=120.

    python tools/kernel_bench.py nulljoint [npsr ntoa F nsky R]

times FastFe.null_max with joint=True and joint=False in alternated
rounds on the synthetic bench array (m = 120), and the phases of one
joint chunk (normals, white-term sbgemm, factor + solve, fe_null_data,
sky kernel); defaults npsr=67, ntoa=5000, F=200, nsky=768, R=1024.
"""

import sys

import numpy as np
import torch

sys.path.insert(0, __import__("os").path.abspath(
    __import__("os").path.join(__import__("os").path.dirname(__file__), "..")))
from fastfp_amd.ops import _fastfp_hip as ext  # noqa: E402

DEV = "cuda:0"


def timeit(fn, iters=20, warmup=5):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    start = torch.cuda.Event(enable_timing=True)
    end = torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(iters):
        fn()
    end.record()
    torch.cuda.synchronize()
    return start.elapsed_time(end) / iters * 1e-3  # seconds


def main():
    m, mp = 120, 128
    F = 1000
    ntoa = 5000
    rng = np.random.default_rng(0)

    T = torch.as_tensor(rng.normal(size=(ntoa, m)), dtype=torch.float64, device=DEV)
    nvec = torch.full((ntoa,), 1e-12, dtype=torch.float64, device=DEV)
    TNT = (T.T @ (T / nvec[:, None])).contiguous()
    toas = torch.as_tensor(
        np.sort(rng.uniform(0, 4.7e8, ntoa)), dtype=torch.float64, device=DEV
    )
    ninv = (1.0 / nvec).contiguous()
    freqs = torch.as_tensor(
        np.arange(1, F + 1) / 4.7e8, dtype=torch.float64, device=DEV
    )
    RHS = torch.zeros((mp, 2 * F + 1), dtype=torch.float64, device=DEV)
    sNs = torch.ones((3, F), dtype=torch.float64, device=DEV) * 1e13
    sNr = torch.ones((2, F), dtype=torch.float64, device=DEV)

    for D in (128, 256, 512, 1024):
        phiinv = torch.as_tensor(
            rng.uniform(0.5, 2.0, (D, m)) * 1e10, dtype=torch.float64, device=DEV
        )
        t = timeit(lambda: ext.chol_batch(TNT, phiinv, mp))
        # flops: assemble+factor: m^3/3 chol + panel/trailing MFMA work
        flops = D * (mp**3 / 3 + mp**3 / 6) * 2
        print(f"chol  D={D:5d}: {t*1e6:9.1f} us  {flops/t/1e12:6.2f} TF/s"
              f"  ({t/D*1e6:6.2f} us/matrix)")

        L, invd = ext.chol_batch(TNT, phiinv, mp)
        fp = torch.zeros((D, F), dtype=torch.float64, device=DEV)
        t = timeit(lambda: ext.trsm_fp_accum(L, invd, RHS, sNs, sNr, fp, 1.0))
        flops = D * (mp * mp / 2) * (2 * F + 2) * 2  # TRSM MACs*2
        print(f"trsm  D={D:5d}: {t*1e6:9.1f} us  {flops/t/1e12:6.2f} TF/s"
              f"  ({flops:.3g} flops)")

    main_stacked()

    # sbgemm at the two headline shapes
    for Fs in (1000, 10000):
        fr = torch.as_tensor(
            np.arange(1, Fs + 1) / 4.7e8, dtype=torch.float64, device=DEV
        )
        out = torch.zeros((mp, 2 * Fs + 1), dtype=torch.float64, device=DEV)
        ctiles = (2 * Fs + 63) // 64
        ks = max(1, min(8, (512 + ctiles - 1) // ctiles, (ntoa + 255) // 256))
        if ks == 1:
            fn = lambda: ext.sbgemm(T, toas, ninv, fr, out, 0, 2 * Fs + 1, mp, 1)  # noqa: E731
        else:
            part = torch.empty((ks, mp, 2 * Fs), dtype=torch.float64, device=DEV)
            fn = lambda: ext.sbgemm(T, toas, ninv, fr, part, mp * 2 * Fs, 2 * Fs, mp, ks)  # noqa: E731
        t = timeit(fn, iters=10)
        flops = 2.0 * mp * 2 * Fs * ntoa
        print(f"sbgemm F={Fs:6d} ks={ks}: {t*1e6:9.1f} us  {flops/t/1e12:6.2f} TF/s")


def main_stacked(P=67, D=1024, F=1000, m=60):
    """The two solve kernels of the stacked compressed sweep, isolated,
    at the flagship shape (67 pulsars, one 1024-draw chunk, mp = 64):
    trsm_fp_accum (one draw per workgroup, accumulates) against
    trsm_fp_store (draw loop, plain stores).  Device events; the factor
    is real, the outputs are checked bitwise equal."""
    mp = (m + 15) // 16 * 16
    ntoa = 2000
    rng = np.random.default_rng(0)
    T = torch.as_tensor(rng.normal(size=(P, ntoa, m)), dtype=torch.float64,
                        device=DEV)
    TNT = (T.transpose(1, 2) @ T * 1e12).contiguous()  # (P, m, m)
    del T
    phiinv = torch.as_tensor(rng.uniform(0.5, 2.0, (P, D, m)) * 1e10,
                             dtype=torch.float64, device=DEV)
    RHS = torch.as_tensor(rng.normal(size=(P, mp, 2 * F + 1)) * 1e6,
                          dtype=torch.float64, device=DEV)
    RHS[:, m:] = 0.0
    sNs = torch.ones((P, 3, F), dtype=torch.float64, device=DEV) * 1e13
    sNr = torch.ones((P, 2, F), dtype=torch.float64, device=DEV)
    L, invd = ext.chol_batch(TNT, phiinv, mp)
    flops = P * D * (mp * mp / 2) * (2 * F + 2) * 2
    acc = torch.zeros((P, D, F), dtype=torch.float64, device=DEV)
    out = torch.full((P, D, F), float("nan"), dtype=torch.float64,
                     device=DEV)
    ext.trsm_fp_accum(L, invd, RHS, sNs, sNr, acc, -1.0)
    ext.trsm_fp_store(L, invd, RHS, sNs, sNr, out, -1.0)
    assert torch.equal(acc, out), "trsm_fp_store != trsm_fp_accum into zeros"
    iters = 20 if D >= 256 else 100
    t = timeit(lambda: ext.trsm_fp_accum(L, invd, RHS, sNs, sNr, acc, -1.0),
               iters=iters)
    print(f"trsm_fp_accum P={P} D={D} F={F} mp={mp}: {t*1e3:9.3f} ms"
          f"  {flops/t/1e12:6.2f} TF/s")
    t = timeit(lambda: ext.trsm_fp_store(L, invd, RHS, sNs, sNr, out, -1.0),
               iters=iters)
    print(f"trsm_fp_store P={P} D={D} F={F} mp={mp}: {t*1e3:9.3f} ms"
          f"  {flops/t/1e12:6.2f} TF/s")

    # lead arm: the same system with the pad in FRONT (identity block,
    # zero RHS rows on top, as the engine's compressed stack presents
    # it), solved with and without the skipped k-steps
    lead = mp - m
    skip = lead - lead % 4
    if skip == 0:
        return
    A = torch.zeros((P, mp, mp), dtype=torch.float64, device=DEV)
    A[:, :lead, :lead] = torch.eye(lead, dtype=torch.float64, device=DEV)
    A[:, lead:, lead:] = TNT
    pad = torch.nn.functional.pad(phiinv, (lead, 0))
    RHSl = torch.zeros_like(RHS)
    RHSl[:, lead:] = RHS[:, :m]
    L, invd = ext.chol_batch(A, pad, mp)
    ref = torch.full_like(out, float("nan"))
    ext.trsm_fp_store(L, invd, RHSl, sNs, sNr, ref, -1.0, lead=0)
    ext.trsm_fp_store(L, invd, RHSl, sNs, sNr, out, -1.0, lead=skip)
    assert torch.equal(ref, out), "trsm_fp_store lead != lead=0"
    for ld in (0, skip):
        t = timeit(lambda: ext.trsm_fp_store(L, invd, RHSl, sNs, sNr, out,
                                             -1.0, lead=ld), iters=iters)
        print(f"trsm_fp_store P={P} D={D} F={F} mp={mp} front pad, lead={ld}:"
              f" {t*1e3:9.3f} ms  {flops/t/1e12:6.2f} TF/s")


def main_factor(P=67, D=1024, m=60):
    """The factor of one stacked draw chunk, isolated (67 pulsars, 1024
    draws, mp = 64): chol_batch_into caller-owned buffers, as the
    sweep's pipeline calls it.  Device events.  In the step this kernel
    runs beside the solve on a side stream and costs the step about 0.8
    of this figure (docs/TUNING_NOTES.md)."""
    mp = (m + 15) // 16 * 16
    ntoa = 2000
    rng = np.random.default_rng(0)
    T = torch.as_tensor(rng.normal(size=(P, ntoa, m)), dtype=torch.float64,
                        device=DEV)
    TNT = (T.transpose(1, 2) @ T * 1e12).contiguous()  # (P, m, m)
    del T
    phiinv = torch.as_tensor(rng.uniform(0.5, 2.0, (P, D, m)) * 1e10,
                             dtype=torch.float64, device=DEV)
    L = torch.empty((P * D, mp, mp), dtype=torch.float64, device=DEV)
    invd = torch.empty((P * D, mp // 16, 16, 16), dtype=torch.float64,
                       device=DEV)
    t = timeit(lambda: ext.chol_batch_into(TNT, phiinv, mp, L, invd),
               iters=50, warmup=5)
    print(f"chol_batch_into P={P} D={D} mp={mp}: {t*1e3:9.3f} ms"
          f"  ({t/(P*D)*1e9:7.1f} ns/matrix,"
          f" {P*D*(mp*mp+mp*16)*8/t/1e9:7.1f} GB/s written)")
    # the sweep's form: the lead-padded system, the diagonal read from
    # the prior rows in place (1 / (rows - delta0) behind the lead)
    lead = mp - m
    A = torch.zeros((P, mp, mp), dtype=torch.float64, device=DEV)
    A[:, :lead, :lead] = torch.eye(lead, dtype=torch.float64, device=DEV)
    A[:, lead:, lead:] = TNT
    delta0 = torch.full((P, m), 1e-3, dtype=torch.float64, device=DEV)
    rows = 1.0 / phiinv + delta0[:, None, :]
    t = timeit(lambda: ext.chol_rows_into(A, rows[0], rows.stride(0), 0, D,
                                          0, delta0, lead, mp, L, invd),
               iters=50, warmup=5)
    print(f"chol_rows_into  P={P} D={D} mp={mp} lead={lead}: {t*1e3:9.3f} ms")


def main_fe(P=67, D=256, F=200, nsky=768, m=120):
    """Fe on device: products mode of the solve + the two sky kernels.

    Synthetic but well-posed inputs: the timed solve runs on a real
    batched Cholesky factor; the sky kernels run on positive-definite
    per-pulsar 2x2 product blocks so every 4x4 M is non-degenerate
    (nskip is checked to be zero — a skipped point would shorten the
    epilogue)."""
    mp = (m + 15) // 16 * 16
    ntoa = 2000
    rng = np.random.default_rng(0)
    T = torch.as_tensor(rng.normal(size=(P, ntoa, m)), dtype=torch.float64,
                        device=DEV)
    TNT = (T.transpose(1, 2) @ T * 1e12).contiguous()  # (P, m, m)
    del T
    phiinv = torch.as_tensor(rng.uniform(0.5, 2.0, (P, D, m)) * 1e10,
                             dtype=torch.float64, device=DEV)
    RHS = torch.zeros((P, mp, 2 * F + 1), dtype=torch.float64, device=DEV)
    sNs = torch.ones((P, 3, F), dtype=torch.float64, device=DEV) * 1e13
    sNr = torch.ones((P, 2, F), dtype=torch.float64, device=DEV)
    L, invd = ext.chol_batch(TNT, phiinv, mp)
    out = torch.empty((P, D, 5, F), dtype=torch.float64, device=DEV)
    t = timeit(lambda: ext.trsm_prods(L, invd, RHS, sNs, sNr, out, 1.0),
               iters=30, warmup=3)
    flops = P * D * (mp * mp / 2) * (2 * F + 2) * 2
    print(f"trsm_prods  P={P} D={D} F={F} mp={mp}: {t*1e3:9.3f} ms"
          f"  {flops/t/1e12:6.2f} TF/s")
    del L, invd

    # the compressed shape: m_v = m / 2 variable columns, padded in
    # FRONT to mp_v as the engine's compressed stack presents it
    # (identity block, zero RHS rows on top), gsign = -1.  trsm_prods
    # and trsm_prods_store on the SAME padded system: the first against
    # the line above is the dimension change, the second against the
    # first the draw loop.
    mv = m // 2
    mpv = (mv + 15) // 16 * 16
    lead = mpv - mv
    skip = lead - lead % 4
    A = torch.zeros((P, mpv, mpv), dtype=torch.float64, device=DEV)
    A[:, :lead, :lead] = torch.eye(lead, dtype=torch.float64, device=DEV)
    A[:, lead:, lead:] = TNT[:, :mv, :mv]
    pad = torch.nn.functional.pad(phiinv[:, :, :mv], (lead, 0)).contiguous()
    RHSv = torch.zeros((P, mpv, 2 * F + 1), dtype=torch.float64, device=DEV)
    RHSv[:, lead:] = torch.as_tensor(
        rng.normal(size=(P, mv, 2 * F + 1)) * 1e6, device=DEV)
    L, invd = ext.chol_batch(A, pad, mpv)
    ref = torch.full_like(out, float("nan"))
    out.fill_(float("nan"))
    ext.trsm_prods(L, invd, RHSv, sNs, sNr, ref, -1.0)
    ext.trsm_prods_store(L, invd, RHSv, sNs, sNr, out, -1.0, lead=skip)
    assert torch.equal(ref, out), "trsm_prods_store != trsm_prods"
    flops = P * D * (mpv * mpv / 2) * (2 * F + 2) * 2
    # alternate the two arms; the spread over rounds is the run-to-run
    # spread that the comparison has to clear
    ts = {"trsm_prods": [], "trsm_prods_store": []}
    for _ in range(5):
        ts["trsm_prods"].append(timeit(
            lambda: ext.trsm_prods(L, invd, RHSv, sNs, sNr, ref, -1.0),
            iters=30, warmup=3))
        ts["trsm_prods_store"].append(timeit(
            lambda: ext.trsm_prods_store(L, invd, RHSv, sNs, sNr, out, -1.0,
                                         lead=skip), iters=30, warmup=3))
    for name, v in ts.items():
        t = float(np.median(v))
        tag = f"{name} P={P} D={D} F={F} mp={mpv} lead={skip}"
        print(f"{tag}: {t*1e3:9.3f} ms  {flops/t/1e12:6.2f} TF/s"
              f"  (5 rounds: min {min(v)*1e3:.3f}, max {max(v)*1e3:.3f})")
    del L, invd, out, ref, TNT, phiinv, A, pad, RHSv

    prods = np.empty((P, D, 5, F))
    prods[:, :, 0] = rng.uniform(1.0, 2.0, (P, D, F))
    prods[:, :, 1] = rng.uniform(1.0, 2.0, (P, D, F))
    prods[:, :, 2] = 0.1 * rng.normal(size=(P, D, F))
    prods[:, :, 3:] = rng.normal(size=(P, D, 2, F))
    prods = torch.as_tensor(prods, device=DEV)
    ant = torch.as_tensor(rng.normal(size=(nsky, P, 2)), device=DEV)
    points = float(nsky) * D * F
    flops = points * 13 * 2 * P  # the pulsar sums; the 4x4 solve is extra
    t = timeit(lambda: ext.fe_assemble(prods, ant), iters=50, warmup=5)
    print(f"fe_assemble nsky={nsky}: {t*1e3:9.3f} ms  {flops/t/1e12:6.2f} TF/s"
          f"  ({points*8/t/1e9:7.1f} GB/s map write)")
    t = timeit(lambda: ext.fe_skymax(prods, ant), iters=50, warmup=5)
    print(f"fe_skymax   nsky={nsky}: {t*1e3:9.3f} ms  {flops/t/1e12:6.2f} TF/s"
          f"  ({flops:.3g} flops = 13*2*P per point)")
    femax, argmax, nskip = ext.fe_skymax(prods, ant)
    fmap = ext.fe_assemble(prods, ant)
    assert int(nskip.sum()) == 0, "bench inputs must be non-degenerate"
    assert torch.equal(femax, fmap.max(dim=1).values)
    print(f"check: nskip=0, skymax == max(map) bitwise; "
          f"femax range [{float(femax.min()):.3g}, {float(femax.max()):.3g}]")
    # the amplitudes at the maximum: one sky row per column, 1/nsky of
    # the sky pass; reads all of prods once
    t = timeit(lambda: ext.fe_amplitudes(prods, ant, argmax), iters=50,
               warmup=5)
    nbytes = prods.numel() * 8
    print(f"fe_amplitudes D*F={D*F}: {t*1e3:9.3f} ms"
          f"  ({nbytes/t/1e9:7.1f} GB/s product read)")
    amps, fe_a, status = ext.fe_amplitudes(prods, ant, argmax)
    assert int(status.sum()) == 0, "bench inputs must be non-degenerate"
    rel = float(((fe_a - femax).abs() / femax).max())
    print(f"check: status=0, fe at argmax vs femax max rel diff {rel:.2e}")
    del prods, fmap, femax, argmax, nskip, amps, fe_a, status
    main_fe_null(P, F, nsky, ant, rng)


def main_fe_null(P, F, nsky, ant, rng, R=1024, rounds=5):
    """Null sky maximum at D = 1: the new kernel against fe_skymax on
    replicated products (what the parent of the kernel offers).  Only the
    fe_skymax call of that route is timed: building its (P, R, 5, F)
    input is left out, in its favour."""
    prods = np.empty((P, 1, 5, F))
    prods[:, :, 0:2] = rng.uniform(1.0, 2.0, (P, 1, 2, F))
    prods[:, :, 2] = 0.1 * rng.normal(size=(P, 1, F))
    prods[:, :, 3:] = 0.0
    prods = torch.as_tensor(prods, device=DEV)
    z = torch.as_tensor(rng.standard_normal((1, F, P, 2, R)), device=DEV)
    ss, cc, sc = prods[:, :, 0], prods[:, :, 1], prods[:, :, 2]  # (P, 1, F)
    l00 = torch.sqrt(ss)
    l10 = sc / l00
    l11 = torch.sqrt(cc - l10 * l10)
    lfac = torch.stack([l00, l10, l11], dim=-1).permute(1, 2, 0, 3).contiguous()
    # the replicated route's input: draw r = realisation r
    zt = z[0].permute(1, 2, 3, 0)  # (P, 2, R, F)
    rep = prods.expand(P, R, 5, F).clone()
    rep[:, :, 3] = l00 * zt[:, 0]
    rep[:, :, 4] = l10 * zt[:, 0] + l11 * zt[:, 1]
    wmax, warg, wskip = ext.fe_skymax(rep, ant)
    femax, argmax, nskip = ext.fe_null_skymax(prods, ant, lfac, z)
    assert int(wskip.sum()) == 0 and int(nskip.sum()) == 0
    got = femax[0].t()  # (R, F)
    rel = float(((got - wmax).abs() / wmax).max())
    same = float((argmax[0].t() == warg).double().mean())
    print(f"check: fe_null_skymax vs replicated fe_skymax max rel diff "
          f"{rel:.2e}, argmax equal at {same:.6f} of the points")
    assert rel < 1e-9
    arms = {
        "fe_skymax replicated": lambda: ext.fe_skymax(rep, ant),
        "fe_null_skymax rtiles=1": lambda: ext.fe_null_skymax(
            prods, ant, lfac, z, 1),
        "fe_null_skymax rtiles=2": lambda: ext.fe_null_skymax(
            prods, ant, lfac, z, 2),
        "fe_null_skymax rtiles=4": lambda: ext.fe_null_skymax(
            prods, ant, lfac, z, 4),
        "fe_null_skymax default": lambda: ext.fe_null_skymax(
            prods, ant, lfac, z),
        "fe_mfactor alone": lambda: ext.fe_mfactor(prods, ant),
    }
    ts = {k: [] for k in arms}
    for _ in range(rounds):
        for k, fn in arms.items():
            ts[k].append(timeit(fn, iters=20, warmup=3))
    points = float(nsky) * R * F
    for k, v in ts.items():
        t = float(np.median(v))
        nsum = 13 if "replicated" in k else 4
        tf = "" if "mfactor" in k else \
            f"  {points * nsum * 2 * P / t / 1e12:6.2f} TF/s ({nsum} sums)"
        print(f"{k:26s} P={P} F={F} nsky={nsky} R={R}: {t*1e3:9.3f} ms{tf}"
              f"  ({rounds} rounds: min {min(v)*1e3:.3f}, "
              f"max {max(v)*1e3:.3f})")


def _rounds(arms, rounds, iters, warmup=2):
    """Alternated rounds of ``arms`` (name -> callable): name -> list of
    per-call seconds, one entry per round."""
    ts = {k: [] for k in arms}
    for _ in range(rounds):
        for k, fn in arms.items():
            ts[k].append(timeit(fn, iters=iters, warmup=warmup))
    return ts


def _report(tag, v, extra=""):
    print(f"{tag}: median {float(np.median(v))*1e3:9.3f} ms  ({len(v)} "
          f"rounds: min {min(v)*1e3:.3f}, max {max(v)*1e3:.3f}){extra}")


def main_null_data(P=67, D=1, F=200, R=1024, m=120, rounds=5):
    """fe_null_data against baddbmm + permuting copy, same inputs, same
    output array."""
    from fastfp_amd import ops

    rng = np.random.default_rng(0)
    mp = ops.pad16(m)
    Rp = ops.pad16(R)
    white = torch.as_tensor(rng.normal(size=(P, Rp, 2 * F + 1)), device=DEV)
    rhs = torch.as_tensor(rng.normal(size=(P, mp, 2 * F + 1)), device=DEV)
    X = torch.zeros((P, D, mp, R), dtype=torch.float64, device=DEV)
    X[:, :, :m] = torch.as_tensor(rng.normal(size=(P, D, m, R)), device=DEV)
    out = torch.empty((D, F, P, 2, R), dtype=torch.float64, device=DEV)
    a = ops.fe_null_data(white, rhs, X, out=out)
    b = ops.fe_null_data_torch(white, rhs, X)
    rel = float(((a - b).abs().max() / b.abs().max()))
    print(f"check: fe_null_data vs torch max abs diff / max abs {rel:.2e}")
    assert rel < 1e-12
    del a, b
    ts = _rounds({
        "fe_null_data": lambda: ops.fe_null_data(white, rhs, X, out=out),
        "torch baddbmm+copy": lambda: ops.fe_null_data_torch(white, rhs, X),
    }, rounds, iters=300, warmup=10)
    nbytes = 2.0 * out.numel() * 8  # white read + n written
    flops = 2.0 * P * D * 2 * F * R * mp
    for k, v in ts.items():
        t = float(np.median(v))
        _report(f"{k:20s} P={P} D={D} F={F} R={R} mp={mp}", v,
                f"  {nbytes/t/1e9:7.1f} GB/s (white + n), "
                f"{flops/t/1e12:5.2f} TF/s")


def main_null_joint(npsr=67, ntoa=5000, F=200, nsky=768, R=1024, rounds=3):
    """null_max(joint=True) against null_max(joint=False), and the phases
    of one joint chunk, on the synthetic bench array."""
    import time

    from fastfp_amd import FastFe, FpEngine, initialize_pta, ops
    from fastfp_amd.cli.run_fe import fibonacci_sky
    from fastfp_amd.data import make_synthetic_pta
    from fastfp_amd.festat import _phiinvs_from_sigmas
    from fastfp_amd.model import get_mats_fp

    psrs = make_synthetic_pta(npsr=npsr, ntoa=ntoa, ntm=60, seed=0)
    noise = {"gw_gamma": 13.0 / 3.0, "gw_log10_A": float(np.log10(2e-15))}
    for p in psrs:
        noise[f"{p.name}_red_noise_gamma"] = 4.0
        noise[f"{p.name}_red_noise_log10_A"] = -14.5
    pta = initialize_pta(psrs, noise, inc_cp=True, rn_comps=30, gwb_comps=30)
    Nvecs, Ts, sigmas = get_mats_fp(pta, noise)
    freqs = np.linspace(2e-9, 3e-7, F)
    sky = fibonacci_sky(nsky)
    eng = FpEngine(psrs, Nvecs, Ts, device=DEV)
    eng.precompute(freqs)
    assert eng._null_kernel_path()
    fe = FastFe(psrs, pta)
    args = (freqs, sky, Nvecs, Ts, sigmas, R)

    def wall(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return time.perf_counter() - t0, out

    arms = {
        "null_max joint=False": lambda: fe.null_max(
            *args, seed=1, engine=eng, real_chunk=R),
        "null_max joint=True": lambda: fe.null_max(
            *args, seed=1, engine=eng, real_chunk=R, joint=True),
    }
    for fn in arms.values():
        fn()  # warm-up
    ts = {k: [] for k in arms}
    for _ in range(rounds):
        for k, fn in arms.items():
            ts[k].append(wall(fn)[0])
    for k, v in ts.items():
        _report(f"{k:22s} P={npsr} F={F} nsky={nsky} R={R}", v)

    # the phases of one joint chunk, each ended by a synchronise
    layer, prods = fe._setup(freqs, sky, Nvecs, Ts, sigmas, DEV, eng)
    phiinvs = _phiinvs_from_sigmas(eng, sigmas, improper=True)
    gen = torch.Generator(device=DEV)
    gen.manual_seed(1)
    st = eng._direct_stack
    ph = {k: [] for k in ("normals", "white sbgemm + Tw", "factor + solve",
                          "fe_null_data", "sky kernel")}
    for i in range(rounds + 1):
        t_n, (w, u) = wall(lambda: eng.null_normals(R, gen))
        t_w, (white, Tw) = wall(lambda: eng._null_white(w))

        def solve():
            pinv = torch.stack(eng._rows(phiinvs)[0]).contiguous()
            L, _ = ops.chol_factor(st.A, pinv, ext=eng._ext)
            mp, m = L.shape[-1], Tw.shape[1]
            U = torch.zeros((npsr, 1, mp, R), dtype=torch.float64, device=DEV)
            U[:, :, :m] = Tw[:, None] - (pinv.clamp_min(0.0).sqrt()[..., None]
                                         * torch.stack(u)[:, None])
            return torch.cholesky_solve(U.view(npsr, mp, R), L).contiguous()

        t_s, X = wall(solve)
        t_c, n = wall(lambda: ops.fe_null_data(
            white, st.RHS, X.view(npsr, 1, -1, R)))
        t_k, _ = wall(lambda: ops.fe_null_skymax(prods, layer.ant, n,
                                                 data=True))
        if i:  # the first pass warms up
            for k, t in zip(ph, (t_n, t_w, t_s, t_c, t_k)):
                ph[k].append(t)
        del w, u, white, Tw, X, n
    total = sum(float(np.median(v)) for v in ph.values())
    for k, v in ph.items():
        _report(f"phase {k:20s}", v,
                f"  {float(np.median(v)) / total * 100:5.1f} % of the phases")


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "nulldata":
        main_null_data(*[int(a) for a in sys.argv[2:]])
    elif len(sys.argv) > 1 and sys.argv[1] == "nulljoint":
        main_null_joint(*[int(a) for a in sys.argv[2:]])
    elif len(sys.argv) > 1 and sys.argv[1] == "fe":
        main_fe(*[int(a) for a in sys.argv[2:]])
    elif len(sys.argv) > 1 and sys.argv[1] == "factor":
        main_factor(*[int(a) for a in sys.argv[2:]])
    elif len(sys.argv) > 1 and sys.argv[1] == "stacked":
        main_stacked(*[int(a) for a in sys.argv[2:]])
    else:
        main()
