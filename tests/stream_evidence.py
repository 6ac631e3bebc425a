"""Frame-by-frame parity of an adaptation stream with the reference's (goldens g5_<tag>.npz, noise floors g5_<tag>_noise.npz).

The end-of-stream check (test_adaptation_gpu.assert_final_state_matches_golden) sees the Adam state after every frame has been folded
in, with bounds as wide as the fp32 trajectory noise of the whole stream.  This module checks every frame on its own:
  - after each frame: the per-tensor norms of exp_avg, exp_avg_sq, theta - theta0 (and the teacher's drift) against the golden's
    frame_*_norms;
  - the outer gradient of every Adam step that can be isolated, g = (m_after - beta1 * m_before) / (1 - beta1) in float64: its
    per-tensor norms against gstep_norms and its first 256 elements of SLICE_PARAMS against gstep_<name>.  A recorder that wraps
    ad.optimizer.step (the autograd path) isolates every step; one that only sees frames (the native stepper, replica groups) isolates
    the frames that hold exactly one Adam step (extra_steps == 0).
Bounds are built like conftest.noise_bounds, row by row: factor x the largest fp32-vs-fp64 deviation the noise file records for the
tensor's class (stage x kind) at that frame or step or any before it, never tighter than NOISE_MIN (and ADAM_SLICE_FLIP for
Adam-normalised drifts)."""
import os

import numpy as np
import torch

from conftest import ADAM_SLICE_FLIP, GOLDEN, NOISE_FACTOR, NOISE_MIN, golden, tensor_class

SLICE_PARAMS = ["conv1.weight", "layer1.0.conv2.weight", "layer2.0.conv2.weight", "layer3.5.conv1.weight",
                "layer4.0.conv2.weight", "layer4.2.bn3.weight", "fc1.weight", "fc2.weight", "decpose.weight",
                "decpose.bias", "deccam.bias"]
FRAME_KEYS = {"m": "frame_m_norms", "v": "frame_v_norms", "d": "frame_delta_norms", "t": "frame_teacher_delta_norms"}
DRAWS = ("ref", "or", "o2")


class EvidenceError(AssertionError):
    pass


def noise_file(tag):
    """-> the loaded g5_<tag>_noise.npz; every tagged stream must have one (no stream falls back to blanket bounds)."""
    path = os.path.join(GOLDEN, f"g5_{tag}_noise.npz")
    assert os.path.exists(path), f"stream {tag} has no noise file {os.path.basename(path)} (tools/make_noise.py --only {tag})"
    return golden(f"g5_{tag}_noise.npz")


def row_bounds(floor_nd, floor_cos, znames, names, factor, cos_min):
    """[rows, 169] fp32-vs-fp64 deviations (file order) -> per-row, per-tensor (nd, cos, floor_nd) bounds in `names` order:
    nd = max(NOISE_MIN['nd'], factor x class max), cos = 1 - max(cos_min, factor x class max of 1 - cos), the class max taken over the
    tensor's class in this row and every row before it."""
    cls = [tensor_class(n) for n in znames]
    keys = sorted(set(cls))
    ci = np.array([keys.index(c) for c in cls])
    idx = np.array([znames.index(n) for n in names])
    nd_c = np.zeros((floor_nd.shape[0], len(keys)))
    cs_c = np.zeros_like(nd_c)
    for k in range(len(keys)):
        nd_c[:, k] = floor_nd[:, ci == k].max(axis=1)
        cs_c[:, k] = (1.0 - floor_cos[:, ci == k]).max(axis=1)
    # a row is ONE draw of the floor per run (three runs, one step): it jumps by 2x - 5x from one step to the next (measured on the gated
    # streams).  The floor only grows along the trajectory, so a row's class value is the running maximum over the rows up to it - the
    # first rows keep their own floor, no row gets a bound below its own
    nd_c, cs_c = np.maximum.accumulate(nd_c, axis=0), np.maximum.accumulate(cs_c, axis=0)
    cn = ci[idx]
    return dict(nd=np.maximum(NOISE_MIN["nd"], factor * nd_c[:, cn]), cos=1.0 - np.maximum(cos_min, factor * cs_c[:, cn]),
                floor=floor_nd[:, idx], floor_cos=1.0 - floor_cos[:, idx])


def per_row_bounds(tag, names, factor=NOISE_FACTOR):
    """-> {"gstep": bounds [nsteps], "m"/"v"/"d"(/"t"): bounds [nframes]} for golden g5_<tag> (see row_bounds)."""
    z = noise_file(tag)
    znames = [str(x) for x in z["names"]]
    draws = [d for d in DRAWS if f"gstep_nd_{d}" in z.files]
    assert draws, f"g5_{tag}_noise.npz has no per-step floors (tools/make_noise.py)"
    out = {}
    for key, pre, cmin in [("gstep", "gstep", NOISE_MIN["cos"])] + [(q, f"frame_{q}", ADAM_SLICE_FLIP if q in "dt" else NOISE_MIN["cos"])
                                                                       for q in "mvdt"]:
        if f"{pre}_nd_ref" not in z.files:
            continue
        nd = np.max([z[f"{pre}_nd_{d}"] for d in draws], axis=0).astype(np.float64)
        cs = np.min([z[f"{pre}_cos_{d}"] for d in draws], axis=0).astype(np.float64)
        out[key] = row_bounds(nd, cs, znames, names, factor, cmin)
    return out


def _norms(flat, layout, names):
    t = layout.unpack(flat)
    return np.array([float(t[k].double().norm()) for k in names]), t


def _cos(a, b):
    a = np.asarray(a, np.float64).ravel()
    b = np.asarray(b, np.float64).ravel()
    return float(a @ b / (np.linalg.norm(a) * np.linalg.norm(b) + 1e-300))


class Evidence:
    """The per-frame / per-step checks of golden g5_<tag> on per-tensor values in the golden's name order; `factor` scales the noise
    floor (NOISE_FACTOR = 3 on the GPU, 5 for the CPU oracle).  `gradient_check(k, frame, norms, slices)` can be replaced (second-order
    finite-difference paths have allowances of their own).  A failure raises EvidenceError naming the frame, the tensor, the value,
    the bound and the floor; report() prints the worst frame / step and tensor as a fraction of its bound."""

    def __init__(self, tag, factor=NOISE_FACTOR, gradient_check=None):
        self.tag = tag
        self.g = golden(f"g5_{tag}.npz")
        self.names = [str(x) for x in self.g["names"]]
        self.nb = per_row_bounds(tag, self.names, factor)
        self.step_frame = np.asarray(self.g["step_frame"])
        self.gradient_check = gradient_check or self.noise_gradient_check
        self.worst = (0.0, "")
        self.steps_checked, self.frames_checked = 0, 0

    def _note(self, frac, what):
        if frac > self.worst[0]:
            self.worst = (frac, what)

    # -- checks
    def noise_gradient_check(self, k, frame, gn, sl):
        """the outer gradient of Adam step k (frame `frame`): per-tensor norms within the step's noise bound, slices above its cosine."""
        b = self.nb["gstep"]
        ref = self.g["gstep_norms"][k]
        e = np.abs(gn - ref) / ref
        for i in np.argsort(-(e / b["nd"][k])):
            if e[i] < b["nd"][k, i]:
                break
            raise EvidenceError(f"{self.tag}: frame {frame} Adam step {k}: outer gradient of {self.names[i]}: norm deviation {e[i]:.3e} "
                                f">= bound {b['nd'][k, i]:.3e} (fp32 floor {b['floor'][k, i]:.3e}); ours {gn[i]:.6e} reference {ref[i]:.6e}")
        i = int(np.argmax(e / b["nd"][k]))
        self._note(e[i] / b["nd"][k, i], f"frame {frame} step {k} gradient norm {self.names[i]}")
        for name, x in sl.items():
            j = self.names.index(name)
            c = _cos(x, self.g["gstep_" + name][k])
            lim = b["cos"][k, j]
            if c <= lim:
                raise EvidenceError(f"{self.tag}: frame {frame} Adam step {k}: outer gradient slice of {name}: cosine {c:.7f} <= bound "
                                    f"{lim:.7f} (fp32 floor of 1 - cos {b['floor_cos'][k, j]:.2e})")
            self._note((1 - c) / (1 - lim), f"frame {frame} step {k} gradient slice {name}")

    def check_gradient(self, k, gn, sl):
        """Adam step k applied the outer gradient with per-tensor norms `gn` (name order) and slices {name: first 256 elements}."""
        assert 0 <= k < len(self.step_frame), (self.tag, k, len(self.step_frame))
        self.gradient_check(k, int(self.step_frame[k]), gn, sl)
        self.steps_checked += 1

    def check_frame(self, frame, norms):
        """after frame `frame`: {q: per-tensor norms} for q in m, v, d (theta - theta0) and t (teacher - theta0)."""
        for q, x in norms.items():
            ref = self.g[FRAME_KEYS[q]][frame]
            b = self.nb[q]
            e = np.abs(x - ref) / ref
            bad = np.nonzero(e >= b["nd"][frame])[0]
            if len(bad):
                i = bad[int(np.argmax(e[bad] / b["nd"][frame, bad]))]
                raise EvidenceError(f"{self.tag}: frame {frame}: {q} norm of {self.names[i]}: deviation {e[i]:.3e} >= bound "
                                    f"{b['nd'][frame, i]:.3e} (fp32 floor {b['floor'][frame, i]:.3e}); ours {x[i]:.6e} reference "
                                    f"{ref[i]:.6e} ({len(bad)} tensors out of bounds)")
            i = int(np.argmax(e / b["nd"][frame]))
            self._note(e[i] / b["nd"][frame, i], f"frame {frame} {q} norm {self.names[i]}")
        self.frames_checked += 1

    def report(self):
        line = (f"per-frame evidence {self.tag}: {self.frames_checked} frames, {self.steps_checked} outer gradients checked; worst "
                f"{self.worst[0]:.3f} of its bound ({self.worst[1]})")
        print(line)
        return line


class StreamEvidence(Evidence):
    """Recorder of one dynaboa_amd Adaptor (single sequence or replica r of a group) running golden g5_<tag> frame by frame:

        ev = StreamEvidence(ad, tag, theta0)           # per_step=True on the autograd path: wraps ad.optimizer.step
        for step in range(n):
            ev.begin_frame()                           # (device snapshot of exp_avg)
            ad.adaptation(batch)
            ev.end_frame(step)
        ev.report()

    The moments are read from ad.optimizer.state[theta] and unpacked through hmr._layout1.  states=False: outer gradients only (the
    second-order difference-quotient paths, whose gradient allowances are their own - fd_gradient_check)."""

    def __init__(self, ad, tag, theta0, per_step=False, factor=NOISE_FACTOR, gradient_check=None, states=True):
        super().__init__(tag, factor, gradient_check)
        self.ad, self.theta0, self.states = ad, theta0, states
        self.hmr = ad.model.module
        self.L = self.hmr._layout1
        self.b1 = float(ad.optimizer.param_groups[0]["betas"][0])
        self.teacher = getattr(ad, "teacher", None) if getattr(ad.options, "use_meanteacher", 0) else None
        self.per_step = per_step
        self._m0 = None
        if per_step:
            opt = ad.optimizer
            orig = opt.step

            def step(*a, **k):
                m0 = self._m()
                out = orig(*a, **k)
                self._check_step(self._t() - 1, m0)
                return out
            opt.step = step

    def _t(self):
        st = self.ad.optimizer.state.get(self.hmr.theta)
        return 0 if st is None else int(st["step"])

    def _m(self):
        st = self.ad.optimizer.state.get(self.hmr.theta)
        return torch.zeros_like(self.hmr.theta, dtype=torch.float64) if st is None else st["exp_avg"].detach().double().clone()

    def _check_step(self, k, m0):
        g = (self._m() - self.b1 * m0) / (1.0 - self.b1)          # float64: m_after = beta1 * m_before + (1 - beta1) * g
        gn, t = _norms(g, self.L, self.names)
        self.check_gradient(k, gn, {n: t[n].flatten()[:256].numpy() for n in SLICE_PARAMS})

    def begin_frame(self):
        if not self.per_step:
            self._m0, self._t0 = self._m(), self._t()

    def end_frame(self, frame):
        t1 = self._t()
        ks = np.nonzero(self.step_frame == frame)[0]
        assert t1 == ks[-1] + 1, (self.tag, frame, "Adam steps so far", t1, "reference", ks[-1] + 1)
        if not self.per_step and len(ks) == 1:
            assert self._t0 == ks[0], (self.tag, frame, self._t0, ks[0])
            self._check_step(int(ks[0]), self._m0)
        self._m0 = None
        if not self.states:
            return
        st = self.ad.optimizer.state[self.hmr.theta]
        flats = dict(m=st["exp_avg"], v=st["exp_avg_sq"], d=self.hmr.theta.detach().double() - self.theta0.double())
        if self.teacher is not None and "t" in self.nb and "frame_teacher_delta_norms" in self.g.files:
            flats["t"] = self.teacher.theta.detach().double() - self.theta0.double()
        self.check_frame(frame, {q: _norms(f, self.L, self.names)[0] for q, f in flats.items()})


def fd_gradient_check(ev, tag_fo, median_cap, max_cap, slice_factor=None):
    """gradient_check of the second-order difference-quotient paths (--hvp fd, --hvp_terms other than all): their frame-0 allowances
    on every step.  Against the reference's second-order gradient of the step (ev's golden) and its first-order twin's (g5_<tag_fo>):
    the median norm error below 0.1 x the median FO-vs-SO gap and below `median_cap`, every tensor below `max_cap`; with
    `slice_factor` every slice's relative error below slice_factor x the FO slice's + 2e-2."""
    gfo = golden(f"g5_{tag_fo}.npz")

    def rel(a, b):
        a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
        return float(np.abs(a - b).max() / (np.abs(b).max() + 1e-30))

    def check(k, frame, gn, sl):
        so, fo = ev.g["gstep_norms"][k], gfo["gstep_norms"][k]
        err, gap = np.abs(gn - so) / so, np.abs(fo - so) / so
        med, gmed = float(np.median(err)), float(np.median(gap))
        if not (med < 0.1 * gmed and med < median_cap and err.max() < max_cap):
            i = int(np.argmax(err))
            raise EvidenceError(f"{ev.tag}: frame {frame} Adam step {k}: outer gradient norm error median {med:.3e} (bound "
                                f"{min(0.1 * gmed, median_cap):.3e}, FO-vs-SO gap median {gmed:.3e}), max {err[i]:.3e} on {ev.names[i]} "
                                f"(bound {max_cap:.1e})")
        ev._note(max(med / min(0.1 * gmed, median_cap), float(err.max()) / max_cap), f"frame {frame} step {k} FD gradient norms")
        for name, x in (sl.items() if slice_factor else ()):
            e, lim = rel(x, ev.g["gstep_" + name][k]), slice_factor * rel(gfo["gstep_" + name][k], ev.g["gstep_" + name][k]) + 2e-2
            if e >= lim:
                raise EvidenceError(f"{ev.tag}: frame {frame} Adam step {k}: outer gradient slice of {name}: relative error {e:.3e} >= "
                                    f"bound {lim:.3e}")
            ev._note(e / lim, f"frame {frame} step {k} FD gradient slice {name}")
    return check
