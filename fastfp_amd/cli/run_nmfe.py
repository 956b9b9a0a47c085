"""Noise-marginalized Fe CLI: sky-coherent CW search over MCMC draws.

Completes the CLI family (run_fp / run_nmfp / run_fe / run_nmfe); no
reference counterpart exists (the reference has neither Fe nor its
marginalized form).  Input contract mirrors ``run_nmfp`` (psrfile,
noisefile, chainfile, savefile; 25% burn-in, last 4 bookkeeping
columns stripped); the sky grid mirrors ``run_fe``.  Output:
``{outdir}/{savefile}.npy`` of shape (nsamples, nsky, nfreqs) plus
``{outdir}/{savefile}.meta.json`` with the freqs/sky axes.

``--skymax`` writes the sky-maximised statistic instead of the cube:
``{savefile}.max.npy`` (nsamples, nfreqs) and ``{savefile}.argmax.npy``
(indices into the meta JSON's ``sky`` list).  ``--assemble device``
runs the sky assembly of the cube in the HIP kernel (GPU only).
``--compress`` takes the per-pulsar products from the Schur-compressed
per-draw systems, as ``run_nmfp`` does for Fp.

``--amplitudes`` (with ``--skymax``) also writes the maximum-likelihood
amplitudes at each maximum, ``{savefile}.amps.npy`` (nsamples, nfreqs, 4)
in the filter order [F+ sin, F+ cos, Fx sin, Fx cos], and
``{savefile}.cwpar.npy`` of the same shape = [h0, cosi, psi, phi0].
"""

import argparse
import json
import logging
import os
import time

import numpy as np
import torch

from fastfp_amd.cli.run_fe import cwpar_array, fibonacci_sky
from fastfp_amd.data import get_tspan, load_pulsars
from fastfp_amd.engine import FpEngine
from fastfp_amd.festat import NMFe
from fastfp_amd.model import get_mats_nmfp, initialize_pta
from fastfp_amd.parallel import (
    all_gather_concat,
    cleanup,
    init_distributed,
    shard_slice,
)


def main(
    psrfile,
    noisefile,
    chainfile,
    savefile,
    inc_cp=False,
    nrncomps=30,
    ngwbcomps=30,
    ncwfreqs=100,
    nsamples=100,
    nsky=48,
    theta=None,
    phi=None,
    outdir="res",
    device=None,
    seed=0,
    batch_size=64,
    skymax=False,
    assemble="host",
    compress=False,
    amplitudes=False,
):
    if amplitudes and not skymax:
        raise ValueError("amplitudes=True needs skymax=True: the amplitudes "
                         "are those at the sky maximum")
    logging.basicConfig(format="%(levelname)s: %(message)s", level=logging.INFO)
    logger = logging.getLogger(__name__)

    rank, world, dev = init_distributed(
        device=torch.device(device) if device else None
    )
    if world > 1:
        torch.set_num_threads(max(1, (os.cpu_count() or world) // world))
    logger.info(f"fastfp_amd backend device {dev} (rank {rank}/{world})")

    psrs = load_pulsars(psrfile)
    with open(noisefile, "r") as f:
        noise = json.load(f)
    chain = np.loadtxt(chainfile)
    if chain.ndim == 1:
        chain = chain[None, :]
    burn = int(0.25 * chain.shape[0])

    noise["gw_gamma"] = 13 / 3
    noise["gw_log10_A"] = float(np.log10(2e-15))

    Tspan = get_tspan(psrs)
    pta = initialize_pta(
        psrs, noise, inc_cp=inc_cp, rn_comps=nrncomps, gwb_comps=ngwbcomps
    )

    t0 = time.perf_counter()
    TNTs, Nvecs, Ts = get_mats_nmfp(pta, noise)
    logger.info(f"Precompute matrix wall time: {time.perf_counter() - t0:.2f} s")

    freqs = np.arange(1, ncwfreqs + 1) / Tspan
    sky = (
        [(float(theta), float(phi))]
        if theta is not None and phi is not None
        else fibonacci_sky(nsky)
    )

    rng = np.random.default_rng(seed)
    n_avail = chain.shape[0] - burn
    idxs = rng.choice(np.arange(burn, chain.shape[0]), size=nsamples,
                      replace=nsamples > n_avail)
    rns_full = chain[idxs, :-4].T  # (nparams, nsamples)

    my = shard_slice(nsamples, rank, world)
    my_idx = np.arange(nsamples)[my]

    t0 = time.perf_counter()
    nm = NMFe(psrs, pta.rn_containers)
    # ONE engine for every batch: the frequency precompute does not
    # depend on the draws
    engine = None
    if len(my_idx):
        engine = FpEngine(psrs, Nvecs, Ts, device=dev)
        engine.precompute(freqs)
        if compress:
            # Schur draw compression: per-draw solves run at the
            # variable-bin dimension only (docs/DESIGN.md)
            engine.enable_draw_compression(
                [c.var_slice for c in pta.rn_containers],
                [c.get_phiinv(noise) for c in pta.rn_containers],
            )
    parts, parts_arg, parts_amp = [], [], []
    for lo in range(0, len(my_idx), batch_size):
        sel = my_idx[lo : lo + batch_size]
        samples = {
            p: rns_full[ct, sel] for ct, p in enumerate(pta.params)
        }
        if skymax:
            res = nm.sweep_max(freqs, sky, samples, Nvecs, Ts,
                               device=dev, engine=engine,
                               compress=compress, amplitudes=amplitudes)
            parts.append(res[0])
            parts_arg.append(res[1])
            if amplitudes:
                parts_amp.append(res[2])
        else:
            parts.append(nm.sweep(freqs, sky, samples, Nvecs, Ts, device=dev,
                                  engine=engine, assemble=assemble,
                                  compress=compress))
    tail = (ncwfreqs,) if skymax else (len(sky), ncwfreqs)
    local = np.concatenate(parts, axis=0) if parts else np.zeros((0,) + tail)
    t_local = torch.as_tensor(local, dtype=torch.float64)
    full = all_gather_concat(t_local, world, dim=0).numpy()
    if skymax:
        local_arg = (np.concatenate(parts_arg, axis=0) if parts_arg
                     else np.zeros((0, ncwfreqs), dtype=np.int64))
        full_arg = all_gather_concat(
            torch.as_tensor(local_arg, dtype=torch.int64), world, dim=0
        ).numpy()
    if amplitudes:
        local_amp = (np.concatenate(parts_amp, axis=0) if parts_amp
                     else np.zeros((0, ncwfreqs, 4)))
        full_amp = all_gather_concat(
            torch.as_tensor(local_amp, dtype=torch.float64), world, dim=0
        ).numpy()
    logger.info(
        "Noise marginalized Fe-statistic wall time: "
        f"{time.perf_counter() - t0:.2f} s"
    )

    if rank == 0:
        os.makedirs(outdir, exist_ok=True)
        if skymax:
            with open(os.path.join(outdir, f"{savefile}.max.npy"), "wb") as f:
                np.save(f, full)
            with open(os.path.join(outdir, f"{savefile}.argmax.npy"),
                      "wb") as f:
                np.save(f, full_arg)
            if amplitudes:
                with open(os.path.join(outdir, f"{savefile}.amps.npy"),
                          "wb") as f:
                    np.save(f, full_amp)
                with open(os.path.join(outdir, f"{savefile}.cwpar.npy"),
                          "wb") as f:
                    np.save(f, cwpar_array(full_amp, freqs))
        else:
            with open(os.path.join(outdir, f"{savefile}.npy"), "wb") as f:
                np.save(f, full)
        with open(os.path.join(outdir, f"{savefile}.meta.json"), "w") as f:
            json.dump({"freqs": [float(x) for x in freqs],
                       "sky": [[t, p] for t, p in sky]}, f)
    cleanup()
    return


def cli():
    parser = argparse.ArgumentParser(description=__doc__)
    parser.add_argument("psrfile", type=str, help="pulsars file (.pkl/.npz/dir)")
    parser.add_argument("noisefile", type=str, help="noise dictionary json")
    parser.add_argument("chainfile", type=str, help="MCMC chain text file")
    parser.add_argument("savefile", type=str, help="output .npy name (no ext)")
    parser.add_argument("--inc_cp", action="store_true", help="include CURN")
    parser.add_argument("--nrncomps", type=int, default=30)
    parser.add_argument("--ngwbcomps", type=int, default=30)
    parser.add_argument("--ncwfreqs", type=int, default=100)
    parser.add_argument("--nsamples", type=int, default=100)
    parser.add_argument("--nsky", type=int, default=48)
    parser.add_argument("--theta", type=float, default=None)
    parser.add_argument("--phi", type=float, default=None)
    parser.add_argument("--outdir", type=str, default="res")
    parser.add_argument("--device", type=str, default=None)
    parser.add_argument("--seed", type=int, default=0)
    parser.add_argument("--batch_size", type=int, default=64)
    parser.add_argument("--skymax", action="store_true",
                        help="write the sky-maximised Fe (.max.npy / "
                             ".argmax.npy) instead of the full cube")
    parser.add_argument("--assemble", choices=["host", "device"],
                        default="host",
                        help="where the sky assembly of the cube runs")
    parser.add_argument("--compress", action="store_true",
                        help="solve the Schur-compressed per-draw systems "
                             "(variable prior bins only), draw by draw where "
                             "the compression margin allows")
    parser.add_argument("--amplitudes", action="store_true",
                        help="with --skymax: also write the maximum-"
                             "likelihood amplitudes (.amps.npy) and source "
                             "parameters (.cwpar.npy) at each maximum")
    args = parser.parse_args()
    if args.amplitudes and not args.skymax:
        parser.error("--amplitudes requires --skymax")
    main(**vars(args))


if __name__ == "__main__":
    cli()
