"""Deferred weight gradients (stepper option "wgrad_defer", adapt_step.hip / hmr_engine.hip backward_body) on cuda:0: a chain backward
of a replica group leaves layer4's weight gradients (but block 0's conv1 / downsample) and the regressor's behind its join on the
auxiliary stream, where they run beside the next forward's stem .. layer3; the forward waits for them before layer4 / before the
pooled feature, every other consumer through settle_update.  The same kernels run on the same inputs with the same split depths -
only the issue order changes - so everything the stepper produces must be IDENTICAL with the option off and on: weights, both Adam
moments, every final prediction, every logged loss, every metric (torch.equal, no tolerance).  The predictions are read through
dyb_stepper_join / dyb_stepper_output straight after each step, with no forward following."""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

NF = 3


@pytest.fixture
def headline_switches():
    """bench.py Runner.__init__ for several sequences per GPU: native_step.set_replica_policy(True)."""
    from dynaboa_amd import _lib, native_step as NS
    lib = _lib.load()
    NS.set_replica_policy(True)
    yield lib
    lib.dyb_set_option(b"rep_split", 0)
    lib.dyb_set_option(b"tp_min", 8)


def _mk_frame_only(r):
    from dynaboa_amd import benchmark as DB
    from dynaboa_amd.base_adaptor import synthetic_bundle
    o = DB.frame_only_options(inner_step=3)                  # the benchmarked schedule: 3 inner steps + 1 outer step
    o.deferred_metrics = 1
    return DB.Adaptor(o, synthetic_bundle(seed=22 + r, identity_pose=False, randomize_norm=True, smpl_seed=0), device="cuda:0")


def _mk_default_terms(r):
    from dynaboa_amd import benchmark as DB
    from dynaboa_amd.base_adaptor import synthetic_bundle
    o = DB.parser.parse_args([])                             # the reference's default term set: teacher + motion + exemplars + dynamic loop
    o.inner_step, o.interval, o.optim_steps, o.cos_sim_threshold, o.deferred_metrics = 1, 2, 2, -1.0, 1
    return DB.Adaptor(o, synthetic_bundle(seed=22 + r, identity_pose=False, randomize_norm=True, smpl_seed=0), device="cuda:0")


def _frames(S):
    from dynaboa_amd import assets
    return [[{k: v.to("cuda:0") for k, v in assets.make_frame(100 * r + s, 1, seed=22).items()} for s in range(NF)] for r in range(S)]


def _sync_errors(lib):
    n = ctypes.c_uint(0)
    assert lib.dyb_sync_error_count(ctypes.byref(n), torch.cuda.current_stream().cuda_stream) == 0
    return int(n.value)


def _run(lib, mk, S, frames, defer, monkeypatch, backwards_per_frame=None):
    from dynaboa_amd import native_step as NS
    monkeypatch.delenv("DYB_WGRAD_DEFER", raising=False)
    ads = [mk(r) for r in range(S)]
    grp = NS.ReplicaGroup(ads, NF)
    ns = grp.stepper
    assert ns.S == S and ns._aux is not None                 # a replica group with an auxiliary stream: where the option applies
    assert lib.dyb_stepper_set_i(ns.h, b"wgrad_defer", defer) == 0
    row = {}
    for step in range(NF):
        grp.step([frames[r][step] for r in range(S)], step)
        ns.join()
        for which in range(4):                               # rotmat, state, vertices, joints of the step's final inference
            for r in range(S):
                row[f"pred/{step}/{which}/{r}"] = ns.output(which, r).clone()
    # the option really changed the schedule: 8 layer4 convolutions + 3 regressor matrices behind the join of every chain backward
    lib.dyb_stepper_get_f.restype = ctypes.c_double
    n = lib.dyb_stepper_get_f(ns.h, b"deferred_launches")
    if not defer:
        assert n == 0, n
    elif backwards_per_frame is not None:
        assert n == 11 * backwards_per_frame * NF, n
    else:
        assert n >= 11 * 4 * NF and n % 11 == 0, n          # default term set: at least the 4 chain backwards of a frame (2 levels + 2 loop steps)
    fl = grp.flush_metrics()
    for r in range(S):
        st = ads[r].optimizer.state[ads[r].model.module.theta]
        row[f"theta/{r}"] = ads[r].model.module.theta.detach().clone()
        row[f"exp_avg/{r}"] = st["exp_avg"].clone()
        row[f"exp_avg_sq/{r}"] = st["exp_avg_sq"].clone()
        if getattr(ads[r], "teacher", None) is not None:
            row[f"teacher/{r}"] = ads[r].teacher.theta.detach().clone()
        for k in ("mpjpe", "pampjpe", "pve"):
            row[f"{k}/{r}"] = torch.from_numpy(np.ravel(np.array(fl[r][k], np.float64)))
    row["loss_log"] = ns.loss_log.clone()
    row["records"] = ns.records.clone()
    torch.cuda.synchronize()
    del grp, ads
    return row


def _assert_identical(off, on):
    assert off.keys() == on.keys()
    assert any(k.startswith("pred/") for k in off) and any(k.startswith("exp_avg_sq/") for k in off)
    for k in off:
        assert torch.equal(off[k], on[k]), k
    assert all(bool(torch.isfinite(v.double()).all()) for k, v in on.items() if k.startswith(("theta/", "pred/", "mpjpe/")))


@pytest.mark.parametrize("S", [32, 8])
def test_deferred_weight_gradients_change_nothing(S, headline_switches, monkeypatch):
    """The benchmarked frame-loss stepper (3 inner + 1 outer step; fused fast-weight / Adam epilogues) at bench.py's 32 sequences
    and at 8: three frames with "wgrad_defer" 0 and 1."""
    lib = headline_switches
    before = _sync_errors(lib)
    frames = _frames(S)
    off = _run(lib, _mk_frame_only, S, frames, 0, monkeypatch, 4)          # 3 lower levels + the outer level
    on = _run(lib, _mk_frame_only, S, frames, 1, monkeypatch, 4)
    _assert_identical(off, on)
    assert _sync_errors(lib) - before == 0


def test_deferred_weight_gradients_change_nothing_default_term_set(headline_switches, monkeypatch):
    """The reference's default term set (teacher, motion and exemplar passes on the stepper's pass streams, the dynamic loop forced
    to its full length, Adam with the teacher's EMA) at 8 sequences: three frames with "wgrad_defer" 0 and 1."""
    lib = headline_switches
    before = _sync_errors(lib)
    S = 8
    frames = _frames(S)
    off = _run(lib, _mk_default_terms, S, frames, 0, monkeypatch)
    on = _run(lib, _mk_default_terms, S, frames, 1, monkeypatch)
    _assert_identical(off, on)
    assert any(k.startswith("teacher/") for k in on)
    assert _sync_errors(lib) - before == 0
