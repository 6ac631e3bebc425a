"""The final inference of a replica group on the side stream ("group_side", adapt_step.hip) under the emulator's lazy stream mode, beside
tests/test_wgrad_defer_emu.py: two sequences on the throughput schedule, frame-loss set, THREE frame steps and then the join, every
operation queued per stream and the queues drained chain-first and side / auxiliary-stream-first.  With the option on, every frame's
final forward + metric record + result row run on a third stream, from the frame's own copy of the staged inputs, as the consuming
forward of the frame's ranged outer update, while the chain goes on with the next frame; everything the stepper leaves behind - theta, both Adam moments, records,
loss rows, result-ring rows, output(k, r) - must be the bits of the option-off run in line, with "wgrad_defer" 0 and 1.  A missing
wait shows in one of the drain orders: chain-first runs every later frame's staging and update before any tail (a tail that does not
keep its own inputs, or an update that does not wait for e_side, reads the wrong frame or the wrong weights); side-first runs each tail
and each frame's ground-truth meshes as early as their waits allow (a tail that misses a range of its frame's outer update reads stale
weights, meshes that do not wait for the staging read the wrong pose).  In one case sequence 1 leaves the active set at the third step:
it gets its frame-1 tail and no frame-2 tail.
Every arm is three full-size frame steps under the emulator: minutes, not seconds - the reference arms are computed once per module."""
import ctypes
from types import SimpleNamespace

import pytest

import group_side_common as G

NF = 3


@pytest.fixture(scope="module")
def emu_lib():
    from emu.build_emu import build
    from dynaboa_amd import _abi, _lib, native_step as NS
    lib = _abi.bind(ctypes.CDLL(build()))
    saved = _lib._lib
    _lib.use_library(lib)
    lib.dyb_set_option(b"rep_split", 1)                    # the throughput schedule at S = 2: dy materialised per layer, igemm_tp epilogues
    lib.dyb_set_option(b"tp_min", 1)
    policy = NS.set_replica_policy
    NS.set_replica_policy = lambda *a, **k: None
    yield lib
    NS.set_replica_policy = policy
    lib.dyb_set_option(b"rep_split", 0)
    lib.dyb_set_option(b"tp_min", 8)
    _lib._lib = saved


def _arm(raw, side, defer, order, leave):
    """order None: in line (immediate execution); 0: lazy, the chain's queue drained first; 1: lazy, side / auxiliary queues first."""
    grp = G.make_group(2, NF, side, "cpu")
    ns = grp.stepper
    ns._aux = SimpleNamespace(cuda_stream=1)               # any non-null handle is a stream of its own to the emulator
    if side:
        ns._side = SimpleNamespace(cuda_stream=2)
    assert raw.dyb_stepper_set_i(ns.h, b"wgrad_defer", defer) == 0
    frames = G.frames_for(2, NF, "cpu")
    if order is None:
        G.step_all(grp, frames, NF, leave)
    else:
        raw.emu_lazy(1)
        try:
            G.step_all(grp, frames, NF, leave)
        finally:
            used = raw.emu_flush(order)
            raw.emu_lazy(0)
        assert used == (3 if side else 2), used            # chain, auxiliary stream and - with the option - the side stream held work
    return G.collect(grp)


_REF = {}


def _reference(raw, defer, leave):
    key = (defer, leave)
    if key not in _REF:
        _REF[key] = _arm(raw, 0, defer, None, leave)
    return _REF[key]


@pytest.mark.parametrize("order", [0, 1])
@pytest.mark.parametrize("defer", [0, 1])
def test_group_side_tail_under_adversarial_stream_order(emu_lib, monkeypatch, defer, order):
    monkeypatch.delenv("DYB_WGRAD_DEFER", raising=False)
    monkeypatch.delenv("DYB_GROUP_SIDE", raising=False)
    ref = _reference(emu_lib, defer, None)
    G.assert_identical(ref, _reference(emu_lib, 0, None))                # ("wgrad_defer" itself changes nothing: test_wgrad_defer_emu.py)
    G.assert_identical(ref, _arm(emu_lib, 1, defer, order, None))


@pytest.mark.parametrize("order", [0, 1])
def test_group_side_tail_when_a_sequence_leaves(emu_lib, monkeypatch, order):
    monkeypatch.delenv("DYB_WGRAD_DEFER", raising=False)
    monkeypatch.delenv("DYB_GROUP_SIDE", raising=False)
    leave = (2, 1)                                         # sequence 1 sits out the third step
    ref = _reference(emu_lib, 1, leave)
    assert bool((ref["records"][1, 2 * (G.INNER + 1):] == 0).all()) and bool((ref["records"][0, 2 * (G.INNER + 1):] != 0).any())
    G.assert_identical(ref, _arm(emu_lib, 1, 1, order, leave))
