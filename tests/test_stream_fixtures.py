"""The per-step / per-frame keys of the g5 goldens and their noise files (tools/make_golden.py, tools/make_noise.py) agree with the
end-of-stream keys the same runs wrote, and every noise file covers every Adam step and frame of its golden (tests/stream_evidence.py)."""
import glob
import os

import numpy as np
import pytest

from conftest import GOLDEN, golden
from stream_evidence import SLICE_PARAMS, noise_file, per_row_bounds

TAGS = sorted(os.path.basename(p)[3:-4] for p in glob.glob(os.path.join(GOLDEN, "g5_*.npz")) if not p.endswith("_noise.npz"))
# optim_steps of each stream (tools/make_golden.py): the dynamic-BOA loop's cut-off; the literal default 7 elsewhere
OPTIM_STEPS = {"fo_inner1_full": 2, "fo_inner1_full_forced": 2, "so_inner1_full": 2}
BETA1 = 0.5         # the reference's default (every g5 stream)


def test_every_stream_is_covered():
    assert len(TAGS) == 11, TAGS


@pytest.mark.parametrize("tag", TAGS)
def test_golden_per_step_and_per_frame_keys_agree_with_the_end_of_stream(tag):
    g = golden(f"g5_{tag}.npz")
    n, nsteps, names = int(g["nframes"]), int(g["adam_steps"]), [str(x) for x in g["names"]]
    sf = np.asarray(g["step_frame"])
    # one Adam step per frame plus the dynamic loop's extra steps (8 = the cut-off: optim_steps extra steps, then break)
    per_frame = np.bincount(sf, minlength=n)
    want = 1 + np.minimum(np.asarray(g["extra_steps"]), OPTIM_STEPS.get(tag, 7))
    np.testing.assert_array_equal(per_frame, want)
    assert len(sf) == nsteps and np.all(np.diff(sf) >= 0)
    # the last frame's state is the end-of-stream state, bit for bit
    pairs = [("frame_m_norms", "m_norms"), ("frame_v_norms", "v_norms"), ("frame_delta_norms", "delta_norms")]
    if "teacher_delta_norms" in g.files:
        pairs.append(("frame_teacher_delta_norms", "teacher_delta_norms"))
    else:
        assert "frame_teacher_delta_norms" not in g.files
    for fk, ek in pairs:
        assert g[fk].shape == (n, len(names)), fk
        np.testing.assert_array_equal(g[fk][-1], g[ek], err_msg=fk)
    # g1_* is exp_avg / (1 - beta1) at the end of frame 0 (tools/make_golden.py): the first gradient itself where frame 0 holds one Adam
    # step (exact up to fp32 rounding), else Adam's first moment over the frame's steps - which the per-step slices must rebuild
    assert g["gstep_norms"].shape == (nsteps, len(names))
    ks = np.nonzero(sf == 0)[0]
    if len(ks) == 1:
        np.testing.assert_allclose(g["gstep_norms"][0], g["g1_norms"], rtol=1e-6)
    for k in SLICE_PARAMS:
        x = g["gstep_" + k]
        assert x.dtype == np.float32 and x.shape[0] == nsteps, k
        m = np.zeros(x.shape[1])
        for j in ks:
            m = BETA1 * m + (1 - BETA1) * x[j].astype(np.float64)
        ref = g["g1_" + k][:x.shape[1]]
        np.testing.assert_allclose(m / (1 - BETA1), ref, rtol=1e-5, atol=1e-6 * np.abs(ref).max(), err_msg=k)
    # a frame's state moves: an implementation frozen after frame 0 does not match frame 1
    assert np.all(np.abs(g["frame_delta_norms"][-1] - g["frame_delta_norms"][0]) > 0) or n == 1


@pytest.mark.parametrize("tag", TAGS)
def test_noise_file_covers_every_step_and_frame(tag):
    g = golden(f"g5_{tag}.npz")
    z = noise_file(tag)
    names = [str(x) for x in g["names"]]
    assert [str(x) for x in z["names"]] == names
    assert int(z["nframes"]) == int(g["nframes"])
    np.testing.assert_array_equal(z["extra_steps"], g["extra_steps"])
    np.testing.assert_array_equal(z["step_frame"], g["step_frame"])
    n, nsteps = int(g["nframes"]), int(g["adam_steps"])
    qs = ["m", "v", "d"] + (["t"] if "teacher_delta_norms" in g.files else [])
    for src in ("ref", "or", "o2"):
        for kind in ("nd", "l2", "cos"):
            x = z[f"gstep_{kind}_{src}"]
            assert x.shape == (nsteps, len(names)) and np.all(np.isfinite(x)), (src, kind)
            for q in qs:
                y = z[f"frame_{q}_{kind}_{src}"]
                assert y.shape == (n, len(names)) and np.all(np.isfinite(y)), (q, src, kind)
                # the end-of-stream keys are the last frame's (stored as float64 there, float32 here)
                if f"{q}_{kind}_{src}" in z.files:
                    np.testing.assert_array_equal(y[-1], z[f"{q}_{kind}_{src}"].astype(np.float32))
    nb = per_row_bounds(tag, names)
    assert nb["gstep"]["nd"].shape == (nsteps, len(names))
    for q in qs:
        assert nb[q]["nd"].shape == (n, len(names)), q
