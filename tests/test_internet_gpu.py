"""The internet-video driver end to end on cuda:0, on a synthetic folder: PNG frames, the golden AlphaPose file, ``--extract``, then
``python -m dynaboa_amd.internet``'s driver with the synthetic checkpoint / SMPL bundle.  Tracks as lockstep replicas write, under the
bit-exact replica policy, the files each track writes when adapted alone; a track that ends leaves the launch set; the default single
stream runs on the native stepper and on the autograd composition; the reference's own streams (g10_internet_stream_*) are reproduced
by both paths."""
import os
import shutil

import numpy as np
import pytest
import torch

from conftest import GOLDEN

pytestmark = pytest.mark.gpu

SEQ = "g10seq"
SHORT = ["--inner_step", "1", "--interval", "2", "--optim_steps", "2"]        # the stream set-up of tests/test_native_results_gpu.py FULL


@pytest.fixture(scope="module")
def folder(tmp_path_factory):
    from PIL import Image
    from dynaboa_amd import internet as I
    root = tmp_path_factory.mktemp("video")
    shutil.copy(os.path.join(GOLDEN, "g10_internet_detections.json"), root / f"{SEQ}.json")
    os.makedirs(root / "images" / SEQ)
    yy, xx = np.mgrid[0:720, 0:1280]
    for f in range(8):                       # smooth pictures: small PNGs, and a crop that is not noise
        img = np.stack([(xx // 5 + 9 * f) % 256, (yy // 3 + 5 * f) % 256, ((xx + yy) // 7 + 3 * f) % 256], -1).astype(np.uint8)
        Image.fromarray(img).save(root / "images" / SEQ / f"{f:06d}.png")
    I.main(["--extract", str(root)])
    return root


def _bundle():
    from dynaboa_amd.base_adaptor import synthetic_bundle
    return synthetic_bundle(seed=22, identity_pose=False, randomize_norm=True, smpl_seed=0)


def _drive(folder, exp, *flags):
    from dynaboa_amd import internet as I
    o = I.parser.parse_args(["--internet_root", str(folder), "--expdir", str(exp), "--expname", "run", *SHORT, *flags])
    rows = I.run_driver(o, assets_bundle=_bundle(), device=torch.device("cuda:0"))
    torch.cuda.synchronize()
    return rows, os.path.join(str(exp), "run")


def _dumps(run):
    import joblib
    d = os.path.join(run, "result")
    return {n: joblib.load(os.path.join(d, n)) for n in sorted(os.listdir(d))}


@pytest.fixture(scope="module")
def alone(folder, tmp_path_factory):
    """Every track adapted alone (one sequence per launch), results numbered by row."""
    from dynaboa_amd import native_step as NS
    NS.set_replica_policy(False)
    rows, run = _drive(folder, tmp_path_factory.mktemp("alone"), "--split_tracks", "1", "--native_results", "1", "--replica_policy", "bitexact")
    assert sorted(rows) == list(range(15))
    return _dumps(run)


@pytest.mark.parametrize("S", [2, 3])
def test_tracks_in_lockstep_equal_the_tracks_alone(folder, tmp_path, alone, monkeypatch, S):
    from dynaboa_amd import native_step as NS
    active = []
    real = NS.NativeStepper.set_active
    monkeypatch.setattr(NS.NativeStepper, "set_active", lambda self, idx=None: (active.append(None if idx is None else list(idx)), real(self, idx))[1])
    try:
        rows, run = _drive(folder, tmp_path, "--split_tracks", "1", "--seqs_per_gpu", str(S), "--native_results", "1", "--save_res", "1",
                           "--replica_policy", "bitexact")
    finally:
        NS.set_replica_policy(False)
    assert sorted(rows) == list(range(15))                                   # one per kept detection, each once
    got = _dumps(run)
    assert sorted(got) == sorted(f"Pred_{n}.pt" for n in range(15))
    assert sorted(os.listdir(os.path.join(run, "image"))) == sorted(f"Pred_{n}.png" for n in range(15))
    assert os.path.isfile(os.path.join(run, "setting.txt"))
    # track 0 has 8 rows, track 1 has 5: after step 4 track 1 leaves the launch set and track 0 goes on alone
    assert [0] in active, active
    for n in sorted(alone):
        assert sorted(got[n]) == ["beta", "cam", "rotmat", "verts"] and got[n]["verts"].shape == (1, 6890, 3)
        for k in got[n]:
            assert got[n][k].dtype == alone[n][k].dtype and np.array_equal(got[n][k], alone[n][k]), (n, k)


@pytest.mark.parametrize("mode", ["native", "autograd"])
@pytest.mark.parametrize("tag", ["full_i2", "full_i2_gated"])
def test_reference_stream(tag, mode, tmp_path):
    """g10_internet_stream_<tag>: the reference's dynaboa_internet run, reproduced by the native stepper and by the autograd path -
    loss terms, every step count and gate decision of the gated tag, the dumped Pred dictionaries, the state within 3 x the measured
    class floor (tests/internet_cases.py)."""
    import internet_cases as IC
    s = IC.run_stream(tag, mode, tmp_path)
    if tag == "full_i2_gated":
        steps = [int(x) for x in s.g["extra_steps"]]
        assert any(1 <= e <= 2 for e in steps) and any(e == 3 for e in steps), steps         # both exits of the loop are in the stream


def test_single_stream_driver_on_both_paths(folder, tmp_path):
    """The default mode of the driver (the reference's one stream over all people, Pred_{global_step}) writes one file per row on the
    native stepper (the driver's default, --native_results 1) and on the autograd composition (--native_results 0: prediction dumps
    route it there)."""
    from dynaboa_amd import benchmark as DB, internet as I
    seen = []
    real = DB.Adaptor._adapt_native
    try:
        DB.Adaptor._adapt_native = lambda self, batch: (seen.append(1), real(self, batch))[1]
        rows_n, run_n = _drive(folder, tmp_path / "native")
        assert len(seen) == 15                              # every frame went through the stepper
        rows_a, run_a = _drive(folder, tmp_path / "autograd", "--native_results", "0")
        assert len(seen) == 15                              # ... and none of the second run's
    finally:
        DB.Adaptor._adapt_native = real
    assert rows_n == rows_a == list(range(15))
    dn, da = _dumps(run_n), _dumps(run_a)
    assert sorted(dn) == sorted(da) == sorted(f"Pred_{n}.pt" for n in range(15))
    for d in (dn, da):
        for n in d:
            assert sorted(d[n]) == ["beta", "cam", "rotmat", "verts"] and all(np.isfinite(v).all() for v in d[n].values())
