"""Closed-form second derivative of the frame-loss head (--hvp_head closed): the cases, run by test_head_hvp_emu.py on the
emulator and by test_head_hvp_gpu.py on the MI355X through the same `be` back-end object as kernel_cases.py.

Yardstick: the fp64 oracle (oracle/ref_cpu.py), differentiated twice by torch.  Errors are norm-wise relative, |a - b| / |b|,
per block of the 157-vector (pose 144, shape 10, cam 3) and over the whole vector.

Tolerances (DESIGN.md section 4 holds the table per case; below, the largest figure over the four whole-head cases):

    floor 1  fp32 torch double-backward of the oracle vs fp64 (CPU)       pose 5.4e-7  shape 5.4e-7  cam 1.8e-7  all 2.1e-7
    floor 2  the EXISTING first-derivative head (_head_grad) vs the fp64 oracle gradient
                                                     emulator             pose 3.2e-7  shape 4.8e-7  cam 2.1e-7  all 2.1e-7
                                                     MI355X               pose 3.6e-7  shape 5.7e-7  cam 1.8e-7  all 2.1e-7
    FLOOR    the larger of the two, per block                             pose 5.4e-7  shape 5.7e-7  cam 2.1e-7  all 2.2e-7
    BOUND    conftest.NOISE_FACTOR (3) x FLOOR                            pose 1.6e-6  shape 1.7e-6  cam 6.3e-7  all 6.6e-7
             (the cap; a case is held to 3 x the larger floor of ITS inputs and block, re-measured in the run, when that is tighter)
    closed   measured                                emulator             pose 3.9e-7  shape 5.7e-7  cam 1.9e-7  all 2.3e-7
                                                     MI355X               pose 3.8e-7  shape 5.3e-7  cam 1.4e-7  all 2.2e-7
    fd       the difference quotient it replaces, whole vector: 8.9e-6 ... 4.5e-5 (emulator), 8.5e-6 ... 7.2e-5 (MI355X)

Floor 1 depends on the CPU that runs torch (its fp32 matrix kernels): the figures are from the machine the suite was developed on; on
the MI355X host it came out larger (shape block up to 2.1e-6), which would only widen the bound, so the smaller floor is the one committed.
Both floors are re-measured and printed by every run next to the committed bound (they involve no code this feature adds)."""
from __future__ import annotations

import types

import numpy as np
import torch

from conftest import NOISE_FACTOR, golden
from dynaboa_amd._abi import check
from kernel_cases import smpl_device_tables
from oracle import ref_cpu as O

W2D, WSHAPE, WPOSE = 10.0, 2e-6, 1e-4              # the reference's loss weights
BLOCKS = {"pose": slice(0, 144), "shape": slice(144, 154), "cam": slice(154, 157), "all": slice(0, 157)}
# the larger of the two floors per block (see the module docstring)
FLOOR = {"pose": 5.4e-7, "shape": 5.7e-7, "cam": 2.1e-7, "all": 2.2e-7}
BOUND = {k: NOISE_FACTOR * v for k, v in FLOOR.items()}
# stage entry points: one bound for every output, 3 x the largest block floor of the whole head above (the stages are pieces of it;
# measured on the stage outputs: 1e-7 ... 5e-7 on either back end)
STAGE_BOUND = NOISE_FACTOR * 5.7e-7
# value half of a stage's (value, tangent) kernel against the first-order kernel: the same arithmetic, contracted differently by the
# compiler - a few fp32 roundings (eps = 6e-8) on a chain of a few operations; bit-identical where no multiply-add is fused
VALUE_BOUND = 1e-6
IDENTITY_ANGLE = 1e-4                              # see case_identity


def nrel(a, b):
    a, b = np.asarray(a, np.float64).ravel(), np.asarray(b, np.float64).ravel()
    return float(np.linalg.norm(a - b) / (np.linalg.norm(b) + 1e-300))


def block_errs(a, b):
    return {k: nrel(np.asarray(a)[:, s], np.asarray(b)[:, s]) for k, s in BLOCKS.items()}


# ------------------------------------------------------------------------------------------------------------- oracle side
def oracle_head(T, gm, state, kp):
    B = state.shape[0]
    rot = O.rot6d_to_rotmat(state[:, :144].reshape(-1, 6)).view(B, 24, 3, 3)
    shape, cam = state[:, 144:154], state[:, 154:157]
    _, j49 = O.smpl_forward(T, shape, rot[:, 1:], rot[:, 0:1], pose2rot=False)
    return W2D * O.kp2d_loss(O.projection(cam, j49), kp) + WSHAPE * O.shape_prior(shape) + WPOSE * O.pose_prior(rot, gm)


def oracle_grad_hv(tab, gmm, state, tstate, kp, dtype):
    """(gradient, H . tstate) of the oracle head at `state` [B][157], evaluated in `dtype`."""
    T = O.smpl_tables_to_torch(tab, dtype=dtype)
    gm = {k: torch.as_tensor(v).to(dtype) for k, v in gmm.items()}
    x = torch.as_tensor(state[:, :157]).to(dtype).clone().requires_grad_(True)
    t = torch.as_tensor(tstate[:, :157]).to(dtype)
    g, = torch.autograd.grad(oracle_head(T, gm, x, torch.as_tensor(kp).to(dtype)), x, create_graph=True)
    hv, = torch.autograd.grad((g * t).sum(), x)
    return g.detach().double().numpy(), hv.double().numpy()


def selections(gmm, state, dtype):
    """(quaternion branch of the 23 body joints, selected mixture component) per sample, as the oracle selects them in `dtype`."""
    B = state.shape[0]
    x = torch.as_tensor(state[:, :144]).to(dtype)
    R = O.rot6d_to_rotmat(x.reshape(-1, 6)).view(B, 24, 3, 3)[:, 1:].reshape(-1, 3, 3)
    d2, d01, d0n1 = R[:, 2, 2] < 1e-6, R[:, 0, 0] > R[:, 1, 1], R[:, 0, 0] < -R[:, 1, 1]
    branch = torch.where(d2 & d01, 0, torch.where(d2, 1, torch.where(d0n1, 2, 3))).view(B, 23).numpy()
    aa = O.rotmat_to_axis_angle(R).reshape(B, 69)
    gm = {k: torch.as_tensor(v).to(dtype) for k, v in gmm.items()}
    d = aa[:, None, :] - gm["means"][None]
    quad = 0.5 * (torch.einsum("mij,bmj->bmi", gm["precisions"], d) * d).sum(-1) - gm["nll_weights"].log()
    return branch, quad.argmin(1).numpy()


# ------------------------------------------------------------------------------------------------------------- inputs
def _x6_of_aa(aa):
    """rot6d numbers whose rotation is Rodrigues(aa): the first two columns of R, read as the (3, 2) matrix rot6d expects."""
    R = O.smplx_rodrigues(torch.as_tensor(aa, dtype=torch.float64).reshape(-1, 3))
    return R[:, :, :2].reshape(-1, 24 * 6).numpy()


def _pack(x6, shape, cam):
    B = x6.shape[0]
    s = np.zeros((B, 160), np.float32)
    s[:, :144], s[:, 144:154], s[:, 154:157] = x6, shape, cam
    return s


def _tangent(rng, B):
    """a state tangent of the size the network's tangent pass hands over (J v for |v| ~ 1e-2 |theta|): a few percent of the state"""
    t = np.zeros((B, 160), np.float32)
    t[:, :144] = rng.standard_normal((B, 144)) * 0.05
    t[:, 144:154] = rng.standard_normal((B, 10)) * 0.1
    t[:, 154:157] = rng.standard_normal((B, 3)) * 0.02
    return t


def _synthetic(tab, seed, B, angle_lo, angle_hi):
    rng = np.random.default_rng(seed)
    axis = rng.standard_normal((B, 24, 3))
    axis /= np.linalg.norm(axis, axis=-1, keepdims=True)
    aa = axis * rng.uniform(angle_lo, angle_hi, (B, 24, 1))
    shape = rng.standard_normal((B, 10)) * 0.5
    cam = np.concatenate([rng.uniform(0.7, 1.1, (B, 1)), rng.uniform(-0.1, 0.1, (B, 2))], 1)
    state = _pack(_x6_of_aa(aa), shape, cam)
    # key points: the projection of a nearby pose, plus noise, random confidences
    T = O.smpl_tables_to_torch(tab, dtype=torch.float64)
    near = torch.as_tensor(state[:, :157], dtype=torch.float64) + 0.05 * torch.as_tensor(rng.standard_normal((B, 157)))
    rot = O.rot6d_to_rotmat(near[:, :144].reshape(-1, 6)).view(B, 24, 3, 3)
    _, j49 = O.smpl_forward(T, near[:, 144:154], rot[:, 1:], rot[:, 0:1], pose2rot=False)
    kp = np.zeros((B, 49, 3), np.float32)
    kp[:, :, :2] = O.projection(near[:, 154:157], j49).numpy() + 0.02 * rng.standard_normal((B, 49, 2))
    kp[:, :, 2] = rng.uniform(0.0, 1.0, (B, 49))
    return state, _tangent(rng, B), kp


def head_inputs(name, tab):
    """-> (state [B][160], tstate [B][160], kp [B][49][3]) float32"""
    if name == "g4":                                # the three samples of the reference's own loss golden
        g = golden("g4_losses.npz")
        B = g["shape"].shape[0]
        return _pack(_x6_of_aa(g["aa"].reshape(B, 24, 3)), g["shape"], g["cam"]), _tangent(np.random.default_rng(4), B), g["kp"].astype(np.float32)
    if name == "large":                             # joint angles past 90 degrees: quaternion branches other than 3
        return _synthetic(tab, 11, 4, 1.7, 3.0)
    if name == "near_identity":                     # about 0.02 rad per joint
        return _synthetic(tab, 12, 2, 0.01, 0.03)
    if name == "moderate":                          # about 0.3 rad per joint, one sample
        return _synthetic(tab, 13, 1, 0.2, 0.4)
    raise KeyError(name)


HEAD_CASES = ("g4", "large", "near_identity", "moderate")


def assert_same_selection(gmm, state, name):
    b32, m32 = selections(gmm, state, torch.float32)
    b64, m64 = selections(gmm, state, torch.float64)
    assert np.array_equal(b32, b64) and np.array_equal(m32, m64), f"{name}: fp32 and fp64 select different branches / components"
    census = np.bincount(b64.ravel(), minlength=4)
    if name == "g4":
        assert census[3] == b64.size, census
    if name == "large":
        assert (census[:3] > 0).sum() >= 2, f"large-pose case must reach two branches besides 3: {census}"
    return census, m64


# ------------------------------------------------------------------------------------------------------------- library side
def _t(be, a, dtype=torch.float32):
    t = torch.as_tensor(np.ascontiguousarray(a)).to(dtype)
    return t.to(be.device) if be.name == "gpu" else t.clone()


def _np(be, t):
    be.sync()
    return t.detach().cpu().numpy().copy()


class Head:
    """The library's head on a back end: tables and prior on the device once; closed form, first derivative, difference quotient."""

    def __init__(self, be, tab, gmm):
        self.be = be
        self.fb, self.ib, (self._ka, pf), (self._kb, pi) = smpl_device_tables(be, tab)
        self.smpl = types.SimpleNamespace(_pf=pf, _pi=pi)
        logw = np.log(gmm["nll_weights"]).astype(np.float32).reshape(-1)
        self.prior = types.SimpleNamespace(means=_t(be, gmm["means"]), precisions=_t(be, gmm["precisions"]), log_nll_weights=_t(be, logw))

    def closed(self, state, tstate, kp, with_losses=False):
        be, B = self.be, state.shape[0]
        S, TS, KP = _t(be, state), _t(be, tstate), _t(be, kp)
        g0 = torch.full((B, 160), float("nan"), device=S.device)
        td = torch.full((B, 160), float("nan"), device=S.device)
        wsb = int(be.lib.dyb_head_hvp_workspace_bytes(B))
        ws = torch.empty(wsb, dtype=torch.uint8, device=S.device)
        L4 = torch.zeros(4, device=S.device)
        p = self.prior
        check(be.lib.dyb_head_hvp(self.smpl._pf, self.smpl._pi, S.data_ptr(), TS.data_ptr(), 160, KP.data_ptr(), p.means.data_ptr(),
                                  p.precisions.data_ptr(), p.log_nll_weights.data_ptr(), W2D, WSHAPE, WPOSE,
                                  L4.data_ptr() if with_losses else None, g0.data_ptr(), td.data_ptr(), 160, B, ws.data_ptr(), wsb,
                                  be.stream), "dyb_head_hvp")
        out = (_np(be, g0), _np(be, td))
        return out + (_np(be, L4),) if with_losses else out

    def closed_py(self, state, tstate, kp):
        """the same through the Python entry the adaptor uses (dynaboa_amd.hvp.head_hvp)"""
        from dynaboa_amd.hvp import head_hvp
        be = self.be
        g0, td = head_hvp(be.lib, self.smpl, self.prior, _t(be, state), _t(be, tstate), _t(be, kp), W2D, WSHAPE, WPOSE, be.stream)
        return _np(be, g0), _np(be, td)

    def grad(self, state, kp):
        from dynaboa_amd.hvp import _head_grad
        be = self.be
        return _np(be, _head_grad(be.lib, self.smpl, self.prior, _t(be, state), _t(be, kp), W2D, WSHAPE, WPOSE, be.stream))

    def fd(self, state, tstate, kp):
        from dynaboa_amd.hvp import head_fd
        be = self.be
        g0, td = head_fd(be.lib, self.smpl, self.prior, _t(be, state), _t(be, tstate), _t(be, kp).repeat(3, 1, 1), W2D, WSHAPE, WPOSE,
                         be.stream)
        return _np(be, g0), _np(be, td)


class HeadSpy:
    """Counts, from construction on, what the adaptor's Hessian-vector products run: products formed by frame_level_hvp, calls of the
    Python heads (hvp.head_hvp / hvp.head_fd), calls of the library's dyb_head_hvp and the batch of every first-derivative head
    evaluation (hvp._head_grad: the fd head runs it on 3 B states).  Fails where the closed head does not exist."""

    def __init__(self, monkeypatch):
        from dynaboa_amd import _lib, hvp
        self.reset()
        lib = _lib.load()
        c_head, py_closed, py_fd, grad, level = lib.dyb_head_hvp, hvp.head_hvp, hvp.head_fd, hvp._head_grad, hvp.frame_level_hvp

        def count(key, fn):
            def f(*a, **k):
                self.n[key] += 1
                return fn(*a, **k)
            return f

        def grad_spy(lib_, smpl, prior, state, *a, **k):
            self.grad_batches.append(int(state.shape[0]))
            return grad(lib_, smpl, prior, state, *a, **k)

        def level_spy(*a, **k):
            self.heads.append(k.get("head", "fd"))
            return count("products", level(*a, **k))
        monkeypatch.setattr(lib, "dyb_head_hvp", count("c_head", c_head))
        monkeypatch.setattr(hvp, "head_hvp", count("py_closed", py_closed))
        monkeypatch.setattr(hvp, "head_fd", count("py_fd", py_fd))
        monkeypatch.setattr(hvp, "_head_grad", grad_spy)
        monkeypatch.setattr(hvp, "frame_level_hvp", level_spy)

    def reset(self):
        self.n = dict(products=0, c_head=0, py_closed=0, py_fd=0)
        self.grad_batches, self.heads = [], []

    def assert_closed(self, B):
        """every product took the closed head: one dyb_head_hvp call each, no difference quotient, no 3 B first-derivative batch"""
        n = self.n
        assert n["products"] > 0 and set(self.heads) == {"closed"}, (n, self.heads)
        assert n["c_head"] == n["py_closed"] == n["products"] and n["py_fd"] == 0, n
        assert 3 * B not in self.grad_batches, self.grad_batches

    def assert_fd(self, B):
        n = self.n
        assert n["products"] > 0 and set(self.heads) == {"fd"}, (n, self.heads)
        assert n["py_fd"] == n["products"] and n["c_head"] == 0 and n["py_closed"] == 0, n
        assert self.grad_batches == [3 * B] * n["products"], self.grad_batches


# ------------------------------------------------------------------------------------------------------------- whole head
def case_head(be, tab, gmm, name, head=None):
    """Items 2, 4 and 5: dyb_head_hvp against the fp64 double-backward of the composed oracle head, per block; against the difference
    quotient it replaces; its gradient bit-identical to the first-derivative head."""
    head = head or Head(be, tab, gmm)
    state, tstate, kp = head_inputs(name, tab)
    census, comp = assert_same_selection(gmm, state, name)
    g64, hv64 = oracle_grad_hv(tab, gmm, state, tstate, kp, torch.float64)
    g32, hv32 = oracle_grad_hv(tab, gmm, state, tstate, kp, torch.float32)
    g_first = head.grad(state, kp)
    g0, td = head.closed(state, tstate, kp)
    _, td_fd = head.fd(state, tstate, kp)
    floor1, floor2 = block_errs(hv32, hv64), block_errs(g_first[:, :157], g64)
    e_closed, e_fd, e_g = block_errs(td[:, :157], hv64), block_errs(td_fd[:, :157], hv64), block_errs(g0[:, :157], g64)
    print(f"\n[{be.name}] head case {name}: B={state.shape[0]} branch census {census.tolist()} components {comp.tolist()}")
    for k in BLOCKS:
        print(f"  {k:5s} floor1 {floor1[k]:.2e}  floor2 {floor2[k]:.2e}  bound {min(BOUND[k], NOISE_FACTOR * max(floor1[k], floor2[k])):.1e} | closed {e_closed[k]:.2e}  fd {e_fd[k]:.2e}"
              f"  | gradient {e_g[k]:.2e}")
    # item 5: the gradient is the first-derivative head's, bit for bit; pad columns zero
    assert np.array_equal(g0.view(np.uint32), g_first.view(np.uint32)), "d_state differs from _head_grad"
    assert not g0[:, 157:].any() and not td[:, 157:].any() and np.isfinite(td).all()
    # item 2: 3 x the larger floor of THIS case and block, never looser than the committed figure (the floors are re-measured here on code
    # this feature does not add; the committed figure caps them where a host's fp32 torch rounds worse than the development machine's)
    bound = {k: min(BOUND[k], NOISE_FACTOR * max(floor1[k], floor2[k])) for k in BLOCKS}
    for k in BLOCKS:
        assert e_closed[k] <= bound[k], (name, k, e_closed[k], bound[k])
    # item 4
    assert e_closed["all"] < e_fd["all"], (name, e_closed["all"], e_fd["all"])
    for k in ("pose", "shape", "cam"):
        assert e_closed[k] <= max(e_fd[k], bound[k]), (name, k, e_closed[k], e_fd[k])
    return dict(closed=e_closed, fd=e_fd, floor1=floor1, floor2=floor2)


def case_python_entry(be, tab, gmm):
    """dynaboa_amd.hvp.head_hvp (what frame_level_hvp(head="closed") calls) hands the library the right key points, leading
    dimensions and workspace: bit-identical to the direct C call on a batch of 4, and not the difference quotient."""
    head = Head(be, tab, gmm)
    state, tstate, kp = head_inputs("large", tab)
    g0, td = head.closed(state, tstate, kp)
    g0p, tdp = head.closed_py(state, tstate, kp)
    assert np.array_equal(g0.view(np.uint32), g0p.view(np.uint32)) and np.array_equal(td.view(np.uint32), tdp.view(np.uint32))
    _, td_fd = head.fd(state, tstate, kp)
    assert not np.array_equal(td_fd.view(np.uint32), tdp.view(np.uint32))


def case_rot6d_degenerate(be):
    """rot6d clamps: a 6-vector whose first column is exactly zero (norm 0 < 1e-12, clamp active) and one whose second column is
    parallel to the first (|u| = 0).  Tangent of an active clamp is zero: outputs finite, never the NaN of d sqrt at 0."""
    x = np.zeros((1, 160), np.float32)
    x[0, :144] = np.tile(np.array([1, 0, 0, 1, 0, 0], np.float32), 24)
    x[0, 0:6] = [0, 1, 0, 0, 0, 1]                   # a1 = 0
    x[0, 6:12] = [1, 2, 0, 0, 0, 0]                  # a2 = 2 a1
    tx = np.full((1, 160), 0.1, np.float32)
    tx[0, 12:18] = 0                                 # and a zero tangent on a regular joint
    X, TX = _t(be, x), _t(be, tx)
    R, TR = (torch.full((1, 24, 9), float("nan"), device=X.device) for _ in range(2))
    check(be.lib.dyb_rot6d_jvp(X.data_ptr(), TX.data_ptr(), 160, R.data_ptr(), TR.data_ptr(), 1, be.stream), "rot6d jvp")
    for a in (R, TR):
        assert np.isfinite(_np(be, a)).all()
    assert not _np(be, TR)[0, 2].any()


def case_head_losses_and_errors(be, tab, gmm):
    """losses4 as dyb_frame_losses reports them; argument errors through DYB_REQUIRE."""
    head = Head(be, tab, gmm)
    state, tstate, kp = head_inputs("g4", tab)
    g = golden("g4_losses.npz")
    _, _, L4 = head.closed(state, tstate, kp, with_losses=True)
    assert abs(L4[1] - g["lsh"]) <= 1e-5 * abs(g["lsh"])          # the shape prior does not depend on the rot6d round trip
    assert np.isfinite(L4).all() and abs(L4[3] - (W2D * L4[0] + WSHAPE * L4[1] + WPOSE * L4[2])) <= 1e-5 * abs(L4[3])
    B = state.shape[0]
    S, TS, KP = _t(be, state), _t(be, tstate), _t(be, kp)
    out = torch.zeros(2, B, 160, device=S.device)
    wsb = int(be.lib.dyb_head_hvp_workspace_bytes(B))
    assert wsb > 0 and be.lib.dyb_head_hvp_workspace_bytes(0) == 0
    ws = torch.empty(wsb, dtype=torch.uint8, device=S.device)
    p = head.prior
    call = lambda s, ld, nbytes: be.lib.dyb_head_hvp(
        head.smpl._pf, head.smpl._pi, s, TS.data_ptr(), ld, KP.data_ptr(), p.means.data_ptr(), p.precisions.data_ptr(),
        p.log_nll_weights.data_ptr(), W2D, WSHAPE, WPOSE, None, out[0].data_ptr(), out[1].data_ptr(), 160, B, ws.data_ptr(), nbytes,
        be.stream)
    assert call(None, 160, wsb) == -1                # DYB_ERR_ARG
    assert call(S.data_ptr(), 100, wsb) == -1        # leading dimension shorter than the state
    assert call(S.data_ptr(), 160, wsb - 16) == -4   # DYB_ERR_WORKSPACE
    assert call(S.data_ptr(), 160, wsb) == 0
    be.sync()


def case_identity(be, tab, gmm):
    """Item 3: every pose 6-vector exactly (1,0,0,1,0,0).  The oracle itself is 0/0 there (NaN in fp32 and fp64), so the yardstick is
    the fp64 oracle with every joint rotated by an angle `a` about a random axis.

    What the angle costs, measured in fp64 (this function prints it): the yardstick moves linearly with the angle - between a and a / 2
    by 1.17e-3 (pose block) at a = 1e-3, 1.17e-4 at 1e-4, 1.17e-5 at 1e-5 - so it drops under the bound of item 2 (pose 1.6e-6) only below
    a ~ 1e-6 rad, where the fp64 oracle's own k = tt / s and its derivatives have lost their digits (eps64 / s^2 = 1e-3 at 1e-6 rad).
    Shrinking the angle alone therefore cannot bring the move under that bound.  Used instead, with IDENTITY_ANGLE = 1e-4 rad (where
    eps64 / s^2 = 1e-7 of one joint's pose-prior term, 1e-4 of the total weight):
      * the plain comparison the issue describes, with the move included in the bound: err <= BOUND + 2 x move(a, a / 2)
        (the yardstick at a is off the identity by twice what it moves between a and a / 2);
      * the sharp one: the linear term removed by extrapolating the yardstick to zero angle, y0 = 2 y(a / 2) - y(a).  What is left is
        second order in the angle; it is measured the same way (y0 from (a, a / 2) against y0 from (a / 2, a / 4): 1.6e-8) and added:
        err <= BOUND + residual, i.e. the bound of item 2 to within 1 %."""
    head = Head(be, tab, gmm)
    B = 2
    rng = np.random.default_rng(21)
    _, tstate, kp = _synthetic(tab, 21, B, 0.01, 0.03)
    shape = rng.standard_normal((B, 10)) * 0.5
    cam = np.concatenate([rng.uniform(0.7, 1.1, (B, 1)), rng.uniform(-0.1, 0.1, (B, 2))], 1)
    ident = np.tile(np.array([1, 0, 0, 1, 0, 0], np.float32), (B, 24))
    state = _pack(ident, shape, cam)
    g0, td = head.closed(state, tstate, kp)
    assert np.isfinite(g0).all() and np.isfinite(td).all()
    assert np.array_equal(g0.view(np.uint32), head.grad(state, kp).view(np.uint32))
    axes = np.random.default_rng(22).standard_normal((B, 24, 3))
    axes /= np.linalg.norm(axes, axis=-1, keepdims=True)

    def yard(angle):
        s64 = _pack(_x6_of_aa(axes * angle), shape, cam).astype(np.float64)
        s64[:, :144] = _x6_of_aa(axes * angle)           # the rotated pose at full fp64 precision
        return oracle_grad_hv(tab, gmm, s64, tstate, kp, torch.float64)[1]
    a = IDENTITY_ANGLE
    y1, y2, y4 = yard(a), yard(a / 2), yard(a / 4)
    move = block_errs(y2, y1)
    y0, y0b = 2 * y2 - y1, 2 * y4 - y2
    resid = block_errs(y0b, y0)
    err, err0 = block_errs(td[:, :157], y1), block_errs(td[:, :157], y0)
    print(f"\n[{be.name}] identity: angle {a:g} rad")
    for k in BLOCKS:
        print(f"  {k:5s} closed vs rotated fp64 oracle {err[k]:.2e} (yardstick move a vs a/2 {move[k]:.2e}) | vs extrapolation to zero angle "
              f"{err0[k]:.2e} (residual {resid[k]:.2e}) | bound {BOUND[k]:.1e}")
    for k in BLOCKS:
        assert err[k] <= BOUND[k] + 2.0 * move[k], (k, err[k], BOUND[k], move[k])
        assert err0[k] <= BOUND[k] + resid[k], (k, err0[k], BOUND[k], resid[k])
    return err0, move


# ------------------------------------------------------------------------------------------------------------- stages
def _hv(scalar, xs, ts):
    """double backward: tangents of the gradients of `scalar` w.r.t. xs along ts (the Hessian is symmetric)"""
    gs = torch.autograd.grad(scalar, xs, create_graph=True)
    return [g.detach() for g in gs], torch.autograd.grad(sum((g * t).sum() for g, t in zip(gs, ts)), xs, allow_unused=True)


def _stage_check(tag, be, got, ref):
    e = {k: nrel(got[k], ref[k]) for k in ref}
    print(f"[{be.name}] stage {tag}: " + "  ".join(f"{k} {v:.2e}" for k, v in e.items()) + f"  (bound {STAGE_BOUND:.1e})")
    assert max(e.values()) <= STAGE_BOUND, (tag, e)
    return e


def case_stage_rot6d(be, B, seed=31):
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((B, 160)).astype(np.float32)
    x[:, :144] += np.tile(np.array([1, 0, 0, 1, 0, 0], np.float32), (B, 24))
    tx = (rng.standard_normal((B, 160)) * 0.1).astype(np.float32)
    dR = rng.standard_normal((B, 24, 9)).astype(np.float32)
    tdR = rng.standard_normal((B, 24, 9)).astype(np.float32)
    X, TX, DR, TDR = _t(be, x), _t(be, tx), _t(be, dR), _t(be, tdR)
    dev = X.device
    R, TR, R0 = (torch.full((B, 24, 9), float("nan"), device=dev) for _ in range(3))
    DX, TDX, DX0 = (torch.zeros(B, 160, device=dev) for _ in range(3))
    check(be.lib.dyb_rot6d_jvp(X.data_ptr(), TX.data_ptr(), 160, R.data_ptr(), TR.data_ptr(), B, be.stream), "rot6d jvp")
    check(be.lib.dyb_rot6d_fwd(X.data_ptr(), 160, R0.data_ptr(), B, be.stream), "rot6d fwd")
    check(be.lib.dyb_rot6d_bwd_jvp(X.data_ptr(), TX.data_ptr(), 160, DR.data_ptr(), TDR.data_ptr(), DX.data_ptr(), TDX.data_ptr(), 160, B,
                                   be.stream), "rot6d bwd jvp")
    check(be.lib.dyb_rot6d_bwd(X.data_ptr(), 160, DR.data_ptr(), DX0.data_ptr(), 160, B, be.stream), "rot6d bwd")
    assert nrel(_np(be, R), _np(be, R0)) <= VALUE_BOUND and nrel(_np(be, DX), _np(be, DX0)) <= VALUE_BOUND
    x64 = torch.as_tensor(x[:, :144], dtype=torch.float64).requires_grad_(True)
    d64 = torch.as_tensor(dR, dtype=torch.float64).requires_grad_(True)
    f = lambda xx: O.rot6d_to_rotmat(xx.reshape(-1, 6)).reshape(B, 24, 9)
    tR64 = torch.autograd.functional.jvp(f, x64.detach(), torch.as_tensor(tx[:, :144], dtype=torch.float64))[1]
    _, (tdx64, _) = _hv((f(x64) * d64).sum(), [x64, d64], [torch.as_tensor(tx[:, :144], dtype=torch.float64), torch.as_tensor(tdR, dtype=torch.float64)])
    return _stage_check(f"rot6d B={B}", be, dict(tR=_np(be, TR), tdx=_np(be, TDX)[:, :144]), dict(tR=tR64.numpy(), tdx=tdx64.numpy()))


def case_stage_lbs(be, tab, B, seed=32):
    """dyb_lbs_jvp and dyb_lbs_bwd_jvp against O.smpl_forward in fp64; value halves against dyb_lbs_fwd / dyb_lbs_bwd."""
    rng = np.random.default_rng(seed)
    betas = (rng.standard_normal((B, 10)) * 0.5).astype(np.float32)
    tbetas = (rng.standard_normal((B, 10)) * 0.1).astype(np.float32)
    rot = O.smplx_rodrigues(torch.from_numpy((rng.standard_normal((B * 24, 3)) * 0.5).astype(np.float32))).view(B, 24, 9).numpy()
    trot = (rng.standard_normal((B, 24, 9)) * 0.05).astype(np.float32)
    dj = rng.standard_normal((B, 49, 3)).astype(np.float32)
    tdj = rng.standard_normal((B, 49, 3)).astype(np.float32)
    fb, ib, (_ka, pf), (_kb, pi) = smpl_device_tables(be, tab)
    BE, TBE, ROT, TROT, DJ, TDJ = (_t(be, a) for a in (betas, tbetas, rot, trot, dj, tdj))
    dev = BE.device
    nan = lambda *s: torch.full(s, float("nan"), device=dev)
    ns = int(be.lib.dyb_lbs_saved_floats(B))
    V, TV, V0, J, TJ, J0 = nan(B, 6890, 3), nan(B, 6890, 3), nan(B, 6890, 3), nan(B, 49, 3), nan(B, 49, 3), nan(B, 49, 3)
    SV, TSV, SV0 = nan(ns), nan(ns), nan(ns)
    check(be.lib.dyb_lbs_jvp(pf, pi, BE.data_ptr(), TBE.data_ptr(), 10, ROT.data_ptr(), TROT.data_ptr(), V.data_ptr(), TV.data_ptr(),
                             J.data_ptr(), TJ.data_ptr(), SV.data_ptr(), TSV.data_ptr(), B, be.stream), "lbs jvp")
    check(be.lib.dyb_lbs_fwd(pf, pi, BE.data_ptr(), 10, ROT.data_ptr(), V0.data_ptr(), J0.data_ptr(), SV0.data_ptr(), B, be.stream), "lbs fwd")
    wsb = int(be.lib.dyb_lbs_bwd_workspace_bytes(B))
    ws = torch.empty(2 * wsb, dtype=torch.uint8, device=dev)
    DR, TDR, DR0, DB, TDB, DB0 = nan(B, 24, 9), nan(B, 24, 9), nan(B, 24, 9), nan(B, 10), nan(B, 10), nan(B, 10)
    check(be.lib.dyb_lbs_bwd_jvp(pf, pi, ROT.data_ptr(), TROT.data_ptr(), SV.data_ptr(), TSV.data_ptr(), DJ.data_ptr(), TDJ.data_ptr(),
                                 DR.data_ptr(), TDR.data_ptr(), DB.data_ptr(), TDB.data_ptr(), 10, B, ws.data_ptr(), 2 * wsb, be.stream),
          "lbs bwd jvp")
    assert be.lib.dyb_lbs_bwd_jvp(pf, pi, ROT.data_ptr(), TROT.data_ptr(), SV.data_ptr(), TSV.data_ptr(), DJ.data_ptr(), TDJ.data_ptr(),
                                  DR.data_ptr(), TDR.data_ptr(), DB.data_ptr(), TDB.data_ptr(), 10, B, ws.data_ptr(), wsb, be.stream) == -4
    check(be.lib.dyb_lbs_bwd(pf, pi, ROT.data_ptr(), SV0.data_ptr(), DJ.data_ptr(), None, DR0.data_ptr(), DB0.data_ptr(), 10, B, ws.data_ptr(),
                             wsb, be.stream), "lbs bwd")
    same = lambda a, b: nrel(_np(be, a), _np(be, b)) <= VALUE_BOUND
    assert same(V, V0) and same(J, J0) and same(SV, SV0) and same(DR, DR0) and same(DB, DB0), "value half differs from the first-order kernels"
    T = O.smpl_tables_to_torch(tab, dtype=torch.float64)
    d = lambda a: torch.as_tensor(a, dtype=torch.float64)
    b64, r64, dj64 = d(betas).requires_grad_(True), d(rot).view(B, 24, 3, 3).requires_grad_(True), d(dj).requires_grad_(True)
    fwd = lambda bb, rr: O.smpl_forward(T, bb, rr[:, 1:], rr[:, 0:1], pose2rot=False)[1]
    tj64 = torch.autograd.functional.jvp(fwd, (b64.detach(), r64.detach()), (d(tbetas), d(trot).view(B, 24, 3, 3)))[1]
    _, (tdb64, tdr64, _) = _hv((fwd(b64, r64) * dj64).sum(), [b64, r64, dj64], [d(tbetas), d(trot).view(B, 24, 3, 3), d(tdj)])
    return _stage_check(f"lbs B={B}", be, dict(tjoints=_np(be, TJ), tdrot=_np(be, TDR), tdbetas=_np(be, TDB)),
                        dict(tjoints=tj64.numpy(), tdrot=tdr64.reshape(B, 24, 9).numpy(), tdbetas=tdb64.numpy()))


def case_stage_losses(be, tab, gmm, B, seed=33):
    """dyb_frame_losses_jvp: tangents of the gradients of 10 kp2d(projection) + 2e-6 shape prior + 1e-4 pose prior, each term against
    its oracle function in fp64 (the kernel's outputs separate them: drot = pose prior, dshape = shape prior, dcam / djoints = 2-D)."""
    rng = np.random.default_rng(seed)
    state, tstate, kp = _synthetic(tab, seed, B, 0.2, 1.2)
    T = O.smpl_tables_to_torch(tab, dtype=torch.float64)
    d = lambda a: torch.as_tensor(a, dtype=torch.float64)
    rot64 = O.rot6d_to_rotmat(d(state[:, :144]).reshape(-1, 6)).view(B, 24, 3, 3)
    rot = rot64.float().numpy().reshape(B, 24, 9)
    trot = (rng.standard_normal((B, 24, 9)) * 0.05).astype(np.float32)
    shape, tshape, cam, tcam = state[:, 144:154].copy(), tstate[:, 144:154].copy(), state[:, 154:157].copy(), tstate[:, 154:157].copy()
    joints = O.smpl_forward(T, d(shape), rot64[:, 1:], rot64[:, 0:1], pose2rot=False)[1].float().numpy()
    tjoints = (rng.standard_normal((B, 49, 3)) * 0.02).astype(np.float32)
    b32, m32 = selections(gmm, state, torch.float32)
    b64, m64 = selections(gmm, state, torch.float64)
    assert np.array_equal(b32, b64) and np.array_equal(m32, m64)
    logw = np.log(gmm["nll_weights"]).astype(np.float32).reshape(-1)
    A = {k: _t(be, v) for k, v in dict(rot=rot, trot=trot, shape=shape, tshape=tshape, cam=cam, tcam=tcam, joints=joints, tjoints=tjoints,
                                      kp=kp, means=gmm["means"], prec=gmm["precisions"], logw=logw).items()}
    dev = A["rot"].device
    nan = lambda *s: torch.full(s, float("nan"), device=dev)
    out = {k: nan(*s) for k, s in dict(L=(4,), L0=(4,), DR=(B, 24, 9), TDR=(B, 24, 9), DR0=(B, 24, 9), DS=(B, 10), TDS=(B, 10), DS0=(B, 10),
                                       DC=(B, 3), TDC=(B, 3), DC0=(B, 3), DJ=(B, 49, 3), TDJ=(B, 49, 3), DJ0=(B, 49, 3), ws=(B * 4,)).items()}
    p = lambda k: (A[k] if k in A else out[k]).data_ptr()
    check(be.lib.dyb_frame_losses_jvp(p("rot"), p("trot"), p("shape"), p("tshape"), 10, p("cam"), p("tcam"), 3, p("joints"), p("tjoints"),
                                      p("kp"), p("means"), p("prec"), p("logw"), W2D, WSHAPE, WPOSE, p("L"), p("DR"), p("TDR"), p("DS"),
                                      p("TDS"), 10, p("DC"), p("TDC"), 3, p("DJ"), p("TDJ"), B, p("ws"), B * 16, be.stream), "losses jvp")
    check(be.lib.dyb_frame_losses(p("rot"), p("shape"), 10, p("cam"), 3, p("joints"), p("kp"), p("means"), p("prec"), p("logw"), W2D, WSHAPE,
                                  WPOSE, p("L0"), p("DR0"), p("DS0"), 10, p("DC0"), 3, p("DJ0"), B, p("ws"), B * 16, be.stream), "losses")
    for a, b in (("L", "L0"), ("DR", "DR0"), ("DS", "DS0"), ("DC", "DC0"), ("DJ", "DJ0")):
        assert nrel(_np(be, out[a]), _np(be, out[b])) <= VALUE_BOUND, a
    gm = {k: d(v) for k, v in gmm.items()}
    r, s, c, j = (d(a).requires_grad_(True) for a in (rot.reshape(B, 24, 3, 3), shape, cam, joints))
    _, (tdc, tdj) = _hv(W2D * O.kp2d_loss(O.projection(c, j), d(kp)), [c, j], [d(tcam), d(tjoints)])
    _, (tds,) = _hv(WSHAPE * O.shape_prior(s), [s], [d(tshape)])
    _, (tdr,) = _hv(WPOSE * O.pose_prior(r, gm), [r], [d(trot).view(B, 24, 3, 3)])
    return _stage_check(f"losses B={B}", be, dict(tdcam=_np(be, out["TDC"]), tdjoints=_np(be, out["TDJ"]), tdshape=_np(be, out["TDS"]),
                                                   tdrot=_np(be, out["TDR"])),
                        dict(tdcam=tdc.numpy(), tdjoints=tdj.numpy(), tdshape=tds.numpy(), tdrot=tdr.reshape(B, 24, 9).numpy()))
