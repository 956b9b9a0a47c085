"""``run_fe --skymax --null`` on two gloo ranks: the sky axis is sharded,
every rank draws the same normals, and the elementwise maximum over the
ranks' null maxima is the single-process null — bit for bit."""

import json
import os

import numpy as np
import torch.multiprocessing as mp

from fastfp_amd import make_synthetic_pta

KW = dict(nfreqs=4, nsky=7, rn_comps=3, gwb_comps=3, device="cpu",
          skymax=True, null=16, null_seed=4)


def _inputs(tmp_path):
    from fastfp_amd.data import save_pulsars

    psrs = make_synthetic_pta(npsr=3, ntoa=60, ntm=3, seed=0)
    psrfile = str(tmp_path / "psrs.npz")
    save_pulsars(psrs, psrfile)
    noise = {}
    for p in psrs:
        noise[f"{p.name}_red_noise_gamma"] = 4.0
        noise[f"{p.name}_red_noise_log10_A"] = -14.5
    noisefile = str(tmp_path / "noise.json")
    with open(noisefile, "w") as f:
        json.dump(noise, f)
    return psrfile, noisefile


def _worker(rank, world, port, psrfile, noisefile, savefile):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    os.environ["RANK"] = str(rank)
    os.environ["WORLD_SIZE"] = str(world)
    os.environ["LOCAL_RANK"] = str(rank)
    from fastfp_amd.cli import run_fe

    run_fe.main(psrfile, noisefile, savefile, **KW)


def test_sky_sharded_null_matches_single(tmp_path):
    from fastfp_amd.cli import run_fe

    psrfile, noisefile = _inputs(tmp_path)
    mp.spawn(_worker,
             args=(2, 29871, psrfile, noisefile, str(tmp_path / "two")),
             nprocs=2, join=True)
    run_fe.main(psrfile, noisefile, str(tmp_path / "one"), **KW)
    for ext in ("null", "pfa", "max", "argmax"):
        got = np.load(tmp_path / f"two.{ext}.npy")
        want = np.load(tmp_path / f"one.{ext}.npy")
        assert got.shape == want.shape
        np.testing.assert_array_equal(got, want)
    assert np.load(tmp_path / "two.null.npy").shape == (16, 4)
