"""Deferred weight gradients ("wgrad_defer", adapt_step.hip / hmr_engine.hip backward_body) under the emulator's lazy stream mode,
beside the lazy-stream cases of test_host_emu.py: one frame step of a replica group on the throughput schedule (a lower level whose
deferred launches write the fast weights, the outer level whose deferred launches apply Adam in place, the final inference) with the
option on, drained chain-first and auxiliary-stream-first, must give the bits of the option off run in line.  A consumer of a deferred
launch that does not wait for it - the next forward's layer4 / regressor, the ranged update of [layer4, end), the final inference -
reads stale weights or activations in one of the two drain orders.  The case is the smallest there is (two sequences, one lower level
plus the outer level, one frame) and runs with every `pytest -m "not gpu"`: about 100 s per arm under the emulator."""
import ctypes
from types import SimpleNamespace

import numpy as np
import pytest
import torch


@pytest.fixture(scope="module")
def emu_lib():
    from emu.build_emu import build
    from dynaboa_amd import _abi, _lib
    lib = _abi.bind(ctypes.CDLL(build()))
    saved = _lib._lib
    _lib.use_library(lib)
    yield lib
    _lib._lib = saved


def test_deferred_weight_gradients_under_adversarial_stream_order(emu_lib, monkeypatch):
    from dynaboa_amd import _lib, assets, benchmark as DB, native_step as NS
    from dynaboa_amd.base_adaptor import synthetic_bundle
    raw = _lib.load()
    monkeypatch.delenv("DYB_WGRAD_DEFER", raising=False)
    raw.dyb_set_option(b"rep_split", 1)                    # the throughput schedule at S = 2: dy materialised per layer, igemm_tp epilogues
    raw.dyb_set_option(b"tp_min", 1)
    monkeypatch.setattr(NS, "set_replica_policy", lambda *a, **k: None, raising=False)
    raw.dyb_stepper_get_f.restype = ctypes.c_double
    S = 2
    frames = [assets.make_frame(100 * r, 1, seed=22) for r in range(S)]
    orig = NS.NativeStepper.adapt_frames
    outs = []
    try:
        for defer, order in ((0, None), (1, 0), (1, 1)):        # option off in line | on, chain drained first | on, auxiliary stream first
            used = []

            def wrapped(self, batches, side_stream=None, order=order, used=used, defer=defer):
                self._aux = SimpleNamespace(cuda_stream=1)          # any non-null handle is a second stream to the emulator
                assert self.lib.dyb_stepper_set_i(self.h, b"wgrad_defer", defer) == 0
                if order is None:
                    return orig(self, batches, side_stream)
                raw.emu_lazy(1)
                try:
                    return orig(self, batches, side_stream)
                finally:
                    used.append(raw.emu_flush(order))
                    raw.emu_lazy(0)
            monkeypatch.setattr(NS.NativeStepper, "adapt_frames", wrapped)
            ads = []
            for r in range(S):
                o = DB.frame_only_options(inner_step=1)
                o.deferred_metrics = 1
                ads.append(DB.Adaptor(o, synthetic_bundle(seed=22 + r, identity_pose=False, randomize_norm=True), device="cpu"))
            grp = NS.ReplicaGroup(ads, 1)
            grp.step(frames, 0)
            fl = grp.flush_metrics()
            if order is not None:
                assert used == [2], used
            # 8 layer4 convolutions + 3 regressor matrices per backward, two backwards (lower level, outer level)
            n = raw.dyb_stepper_get_f(grp.stepper.h, b"deferred_launches")
            assert n == (2 * 11 if defer else 0), n
            row = []
            for r in range(S):
                st = ads[r].optimizer.state[ads[r].model.module.theta]
                row += [ads[r].model.module.theta.detach().clone(), st["exp_avg"].clone(), st["exp_avg_sq"].clone(),
                        torch.from_numpy(np.ravel(np.array(fl[r]["mpjpe"], np.float64))),
                        torch.from_numpy(np.ravel(np.array(fl[r]["pampjpe"], np.float64)))]
            row.append(grp.stepper.loss_log.clone())
            outs.append(row)
    finally:
        raw.dyb_set_option(b"rep_split", 0)
        raw.dyb_set_option(b"tp_min", 8)
    for other in outs[1:]:
        for a, b in zip(outs[0], other):
            assert torch.equal(a, b)
