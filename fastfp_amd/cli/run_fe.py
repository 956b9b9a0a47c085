"""Fe-statistic sweep CLI: sky-coherent Earth-term CW search.

Companion to ``run_fp`` for the Fe statistic (the reference's open
to-do, ``/root/reference/README.md:23`` — no reference counterpart
exists).  Same input contract as ``run_fp`` (psrfile, noisefile,
savefile; CURN parameters fixed as in the reference script); sweeps
the (frequency x sky) grid and writes ``{savefile}.json``:

    {"freqs": [...], "sky": [[theta, phi], ...],
     "fe": [[Fe(sky0, f0), ...], ...]}        # (nsky, nfreqs)

The sky grid is an equal-area-ish lattice of ``--nsky`` points
(Fibonacci sphere), or a single ``--theta/--phi`` location.  Pulsars
must carry sky positions (``PulsarData.pos``).

``--skymax`` writes the statistic maximised over the sky instead of the
map: ``{savefile}.max.npy`` (nfreqs,) and ``{savefile}.argmax.npy``
(indices into ``sky``); ``{savefile}.json`` then holds only the
``freqs`` and ``sky`` axes.  ``--assemble device`` runs the sky
assembly of the map in the HIP kernel (GPU only).

``--amplitudes`` (with ``--skymax``) also writes the maximum-likelihood
amplitudes at each maximum, ``{savefile}.amps.npy`` (nfreqs, 4) in the
filter order [F+ sin, F+ cos, Fx sin, Fx cos], and the source parameters
they imply, ``{savefile}.cwpar.npy`` (nfreqs, 4) = [h0, cosi, psi, phi0]
(``festat.cw_parameters``).

``--null R`` (with ``--skymax``) also draws ``R`` noise-only realisations
of the sky maximum per frequency (``FastFe.null_max``, seed
``--null_seed``) and writes ``{savefile}.null.npy`` (R, nfreqs) and the
false-alarm probability of each observed maximum,
``{savefile}.pfa.npy`` (nfreqs,) = (1 + #{null >= max}) / (1 + R).  The
normals do not depend on the sky, so under torchrun every rank draws the
same ones and takes the null maximum over its sky shard; the elementwise
maximum over ranks is the single-process null.

``--null_joint`` (with ``--null R``) draws the realisations jointly across
frequencies (``FastFe.null_max(joint=True)``: one noise realisation per
pulsar serves the whole grid), so ``{savefile}.null.npy`` and
``{savefile}.pfa.npy`` come from joint realisations, and also writes
``{savefile}.pfa_global.npy`` = [femax_global, f, pfa_global]
(``festat.global_false_alarm``): the loudest observed maximum, its
frequency index, and the probability that noise alone makes any frequency
that loud.  Under torchrun every rank draws the same ``(w, u)``.
"""

import argparse
import json
import logging
import time

import numpy as np
import torch

from fastfp_amd.data import load_pulsars
from fastfp_amd.engine import FpEngine
from fastfp_amd.festat import (
    FastFe,
    cw_parameters,
    false_alarm_probability,
    global_false_alarm,
)
from fastfp_amd.model import get_mats_fp, initialize_pta
from fastfp_amd.parallel import (
    all_gather_concat,
    cleanup,
    init_distributed,
    shard_slice,
)


def cwpar_array(amps, freqs) -> np.ndarray:
    """(..., F, 4) amplitudes -> (..., F, 4) = [h0, cosi, psi, phi0]."""
    par = cw_parameters(amps, f=np.asarray(freqs, dtype=np.float64))
    return np.stack([par[k] for k in ("h0", "cosi", "psi", "phi0")], axis=-1)


def fibonacci_sky(nsky: int) -> list:
    """~Equal-area sky lattice: (theta, phi) colatitude/longitude pairs
    on the Fibonacci sphere."""
    ga = np.pi * (3.0 - np.sqrt(5.0))
    k = np.arange(nsky)
    z = 1.0 - (2.0 * k + 1.0) / nsky
    theta = np.arccos(z)
    phi = np.mod(ga * k, 2.0 * np.pi)
    return [(float(t), float(p)) for t, p in zip(theta, phi)]


def main(
    psrfile,
    noisefile,
    savefile,
    nfreqs=200,
    fmin=2e-9,
    fmax=3e-7,
    nsky=48,
    theta=None,
    phi=None,
    device=None,
    rn_comps=30,
    gwb_comps=30,
    skymax=False,
    assemble="host",
    amplitudes=False,
    null=0,
    null_seed=0,
    null_joint=False,
):
    if null_joint and not null:
        raise ValueError("null_joint needs null > 0 realisations")
    if null and not skymax:
        raise ValueError("null needs skymax=True: the null distribution is "
                         "that of the sky maximum")
    if null < 0:
        raise ValueError("null must be a number of realisations >= 0")
    if amplitudes and not skymax:
        raise ValueError("amplitudes=True needs skymax=True: the amplitudes "
                         "are those at the sky maximum")
    logging.basicConfig(format="%(levelname)s: %(message)s", level=logging.INFO)
    logger = logging.getLogger(__name__)

    rank, world, dev = init_distributed(
        device=torch.device(device) if device else None
    )
    if world > 1:
        import os

        torch.set_num_threads(max(1, (os.cpu_count() or world) // world))
    logger.info(f"fastfp_amd backend device {dev} (rank {rank}/{world})")

    psrs = load_pulsars(psrfile)
    with open(noisefile, "r") as f:
        noise = json.load(f)
    noise["gw_gamma"] = 13 / 3
    noise["gw_log10_A"] = float(np.log10(2e-15))

    pta = initialize_pta(
        psrs, noise, inc_cp=True, rn_comps=rn_comps, gwb_comps=gwb_comps
    )

    t0 = time.perf_counter()
    Nvecs, Ts, sigmas = get_mats_fp(pta, noise)
    logger.info(f"Precompute matrix wall time: {time.perf_counter() - t0:.4f} s")

    freqs = np.linspace(fmin, fmax, nfreqs)
    sky = (
        [(float(theta), float(phi))]
        if theta is not None and phi is not None
        else fibonacci_sky(nsky)
    )
    # shard the SKY axis across ranks (the engine pass is per-rank;
    # each sky point is O(P) assembly on top of it)
    local_sky = sky[shard_slice(len(sky), rank, world)]

    t0 = time.perf_counter()
    fe = FastFe(psrs, pta)
    if skymax:
        # per-rank maximum over its sky shard, then the maximum over
        # ranks (shards are in sky order: the first maximum is the
        # lowest sky index)
        amp = np.full((nfreqs, 4), np.nan)
        engine = None
        if local_sky and null:
            # one precompute serves the observed pass and the null pass
            engine = FpEngine(psrs, Nvecs, Ts, device=dev)
            engine.precompute(freqs)
        if local_sky and amplitudes:
            fm, am, amp = fe.sweep_max(freqs, local_sky, Nvecs, Ts, sigmas,
                                       device=dev, engine=engine,
                                       amplitudes=True)
        elif local_sky:
            fm, am = fe.sweep_max(freqs, local_sky, Nvecs, Ts, sigmas,
                                  device=dev, engine=engine)
        else:
            fm = np.full(nfreqs, -np.inf)
            am = np.zeros(nfreqs, dtype=np.int64)
        am = am + (shard_slice(len(sky), rank, world).start or 0)
        fms = all_gather_concat(
            torch.as_tensor(fm[None], dtype=torch.float64), world, dim=0
        ).numpy()
        ams = all_gather_concat(
            torch.as_tensor(am[None], dtype=torch.int64), world, dim=0
        ).numpy()
        if amplitudes:
            # each rank's amplitudes at its local maximum; the rank that
            # holds the global maximum is picked below with ``best``
            amp_all = all_gather_concat(
                torch.as_tensor(amp[None], dtype=torch.float64), world, dim=0
            ).numpy()
        if null:
            # every rank draws the same normals (they do not depend on the
            # sky); the maximum over its shard, then over ranks
            nl = (fe.null_max(freqs, local_sky, Nvecs, Ts, sigmas, null,
                              seed=null_seed, engine=engine,
                              joint=null_joint)
                  if local_sky else np.full((null, nfreqs), -np.inf))
            nls = all_gather_concat(
                torch.as_tensor(nl[None], dtype=torch.float64), world, dim=0
            ).numpy().max(axis=0)
        logger.info(f"Fe-statistic wall time: {time.perf_counter() - t0:.4f} s")
        if rank == 0:
            best = np.argmax(fms, axis=0)
            cols = np.arange(nfreqs)
            np.save(f"{savefile}.max.npy", fms[best, cols])
            np.save(f"{savefile}.argmax.npy", ams[best, cols])
            if amplitudes:
                amps = amp_all[best, cols]
                np.save(f"{savefile}.amps.npy", amps)
                np.save(f"{savefile}.cwpar.npy", cwpar_array(amps, freqs))
            if null:
                np.save(f"{savefile}.null.npy", nls)
                np.save(f"{savefile}.pfa.npy",
                        false_alarm_probability(fms[best, cols], nls))
                if null_joint:
                    fg, fi, pg = global_false_alarm(fms[best, cols], nls)
                    np.save(f"{savefile}.pfa_global.npy",
                            np.array([fg, fi, pg], dtype=np.float64))
            with open(f"{savefile}.json", "w") as f:
                json.dump({"freqs": [float(x) for x in freqs],
                           "sky": [[t, p] for t, p in sky]}, f)
        cleanup()
        return
    local = fe.sweep(freqs, local_sky, Nvecs, Ts, sigmas, device=dev,
                     assemble=assemble) \
        if local_sky else np.zeros((0, nfreqs))
    t_local = torch.as_tensor(local, dtype=torch.float64)
    full = all_gather_concat(t_local, world, dim=0).numpy()
    logger.info(f"Fe-statistic wall time: {time.perf_counter() - t0:.4f} s")

    if rank == 0:
        out = {
            "freqs": [float(f) for f in freqs],
            "sky": [[t, p] for t, p in sky],
            "fe": full.tolist(),
        }
        with open(f"{savefile}.json", "w") as f:
            json.dump(out, f)
    cleanup()
    return


def cli():
    parser = argparse.ArgumentParser(description=__doc__)
    parser.add_argument("psrfile", type=str, help="pulsars file (.pkl/.npz/dir)")
    parser.add_argument("noisefile", type=str, help="noise dictionary json")
    parser.add_argument("savefile", type=str, help="output json path (no ext)")
    parser.add_argument("--nfreqs", type=int, default=200)
    parser.add_argument("--fmin", type=float, default=2e-9)
    parser.add_argument("--fmax", type=float, default=3e-7)
    parser.add_argument("--nsky", type=int, default=48,
                        help="Fibonacci-sphere sky points")
    parser.add_argument("--theta", type=float, default=None,
                        help="single-sky colatitude (with --phi)")
    parser.add_argument("--phi", type=float, default=None,
                        help="single-sky longitude (with --theta)")
    parser.add_argument("--device", type=str, default=None)
    parser.add_argument("--rn_comps", type=int, default=30)
    parser.add_argument("--gwb_comps", type=int, default=30)
    parser.add_argument("--skymax", action="store_true",
                        help="write the sky-maximised Fe (.max.npy / "
                             ".argmax.npy) instead of the (sky x freq) map")
    parser.add_argument("--assemble", choices=["host", "device"],
                        default="host",
                        help="where the sky assembly of the map runs")
    parser.add_argument("--amplitudes", action="store_true",
                        help="with --skymax: also write the maximum-"
                             "likelihood amplitudes (.amps.npy) and source "
                             "parameters (.cwpar.npy) at each maximum")
    parser.add_argument("--null", type=int, default=0, metavar="R",
                        help="with --skymax: also draw R noise-only "
                             "realisations of the sky maximum (.null.npy) "
                             "and write the false-alarm probability of each "
                             "observed maximum (.pfa.npy)")
    parser.add_argument("--null_seed", type=int, default=0,
                        help="seed of the --null realisations")
    parser.add_argument("--null_joint", action="store_true",
                        help="with --null: draw the realisations jointly "
                             "across frequencies and also write the search-"
                             "wide false-alarm probability (.pfa_global.npy)")
    args = parser.parse_args()
    if args.null_joint and not args.null:
        parser.error("--null_joint requires --null")
    if args.null and not args.skymax:
        parser.error("--null requires --skymax")
    if args.amplitudes and not args.skymax:
        parser.error("--amplitudes requires --skymax")
    main(**vars(args))


if __name__ == "__main__":
    cli()
