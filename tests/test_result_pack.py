"""dyb_result_pack (csrc/adapt_step.hip): one final inference packed into one row of the native stepper's result ring - on the kernel
emulator here, on cuda:0 under `-m gpu`.  Row per sample: verts [6890][3] | rotmat [24][9] | beta [10] | cam [3] | 1 pad float."""
import ctypes

import numpy as np
import pytest
import torch

_EMU = {}
ROW = 20900
SENTINEL = -77.25


@pytest.fixture
def emu_lib():
    from emu.build_emu import build
    from dynaboa_amd import _abi, _lib
    if "lib" not in _EMU:
        _EMU["lib"] = _abi.bind(ctypes.CDLL(build()))
    saved = _lib._lib
    _lib.use_library(_EMU["lib"])
    yield _EMU["lib"]
    _lib._lib = saved


@pytest.fixture(params=["emu", pytest.param("gpu", marks=pytest.mark.gpu)])
def dev(request):
    if request.param == "emu":
        request.getfixturevalue("emu_lib")
        return "cpu"
    return "cuda:0"


@pytest.mark.parametrize("B", [1, 2])
def test_result_pack_equals_the_concatenation(dev, B):
    """B = 2: the odd sample's vertices start at 20670 floats - 8-byte aligned only, the two-load path of the kernel.  The pad float of
    every sample and the floats behind the row keep their sentinel."""
    from dynaboa_amd import _lib
    lib = _lib.load()
    g = torch.Generator().manual_seed(11 + B)
    rot, state, verts = torch.randn(B, 24, 9, generator=g), torch.randn(B, 160, generator=g), torch.randn(B, 6890, 3, generator=g)
    out = torch.full((B * ROW + 64,), SENTINEL)
    d_rot, d_state, d_verts, d_out = (t.to(dev) for t in (rot, state, verts, out))
    assert d_verts.data_ptr() % 16 == 0 and d_out.data_ptr() % 16 == 0
    st = torch.cuda.current_stream().cuda_stream if dev != "cpu" else None
    assert lib.dyb_result_pack(d_rot.data_ptr(), d_state.data_ptr(), d_verts.data_ptr(), d_out.data_ptr(), B, st) == 0
    got = d_out.cpu().numpy()
    want = np.full(B * ROW + 64, SENTINEL, np.float32)
    for b in range(B):
        want[b * ROW:b * ROW + ROW - 1] = np.concatenate([verts[b].numpy().ravel(), rot[b].numpy().ravel(), state[b, 144:154].numpy(),
                                                           state[b, 154:157].numpy()])
    assert got.tobytes() == want.tobytes()
    # bad arguments: nothing is written
    d_out.fill_(SENTINEL)
    assert lib.dyb_result_pack(None, d_state.data_ptr(), d_verts.data_ptr(), d_out.data_ptr(), B, st) == -1
    assert lib.dyb_result_pack(d_rot.data_ptr(), d_state.data_ptr(), d_verts.data_ptr(), d_out.data_ptr(), 0, st) == -1
    assert lib.dyb_result_pack(d_rot.data_ptr(), d_state.data_ptr(), d_verts.data_ptr(), d_out.data_ptr() + 4, B, st) == -1
    assert bool((d_out.cpu() == SENTINEL).all())
