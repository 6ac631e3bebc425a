"""The final inference of a replica group on the side stream (stepper option "group_side", adapt_step.hip) on cuda:0.  With the option
on, the frame's final forward + metric record + result row leave the chain for a third stream, where they run from the frame's own
copy of the staged inputs beside the next frame's first level; the chain's stream only waits for the outer update itself.  Same kernels, same inputs, same split depths - only the issue order changes - so three frames with the option 0 and 1 must leave
IDENTICAL bytes ("wgrad_defer" at its default): records, loss log, result ring, output(k, r) after the join, and theta / both Adam
moments at a seeded sample.  S = 8 runs the throughput schedule, S = 2 the latency-form kernels in a group; in a third case a sequence
leaves the active set at the third step (it gets its frame-1 tail and no frame-2 tail)."""
import ctypes

import pytest
import torch

import group_side_common as G

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


def _sync_errors(lib):
    n = ctypes.c_uint(0)
    assert lib.dyb_sync_error_count(ctypes.byref(n), torch.cuda.current_stream().cuda_stream) == 0
    return int(n.value)


def _run(S, side, frames, sample, leave):
    grp = G.make_group(S, NF, side, "cuda:0")
    ns = grp.stepper
    assert ns._aux is not None and (ns._side is not None) == bool(side)
    G.step_all(grp, frames, NF, leave)
    torch.cuda.synchronize()
    row = G.collect(grp, sample)
    torch.cuda.synchronize()
    return row


@pytest.mark.parametrize("S,leave", [(8, None), (2, None), (8, (2, 1))])
def test_group_side_changes_nothing(S, leave, headline_switches, monkeypatch):
    lib = headline_switches
    monkeypatch.delenv("DYB_GROUP_SIDE", raising=False)
    monkeypatch.delenv("DYB_WGRAD_DEFER", raising=False)
    before = _sync_errors(lib)
    frames = G.frames_for(S, NF, "cuda:0")
    off = _run(S, 0, frames, 1 << 16, leave)
    row = _run(S, 1, frames, 1 << 16, leave)
    G.assert_identical(off, row)
    assert all(bool(torch.isfinite(v.double()).all()) for v in row.values())
    assert bool((row["results"] != 0).any()) and bool((row["records"] != 0).any())
    if leave is not None:                                   # the sequence that left has no records of the third frame; the others do
        k = leave[0] * (G.INNER + 1)
        assert bool((row["records"][leave[1], k:] == 0).all()) and bool((row["records"][0, k:] != 0).any())
    assert _sync_errors(lib) - before == 0
