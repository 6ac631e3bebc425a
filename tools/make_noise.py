#!/usr/bin/env python3
"""fp32 noise floor of the g5 adaptation streams: how far does an fp32 run of the reference's algorithm sit from
the SAME algorithm evaluated in fp64?  Three runs of every stream on the same seeded inputs, in the build container:

  ref32     the REFERENCE's own Adaptor.adaptation() in fp32 (tools/make_golden.py machinery: the run the goldens come from)
  oracle32  oracle.ref_cpu.Adapter in fp32 (a second, independent fp32 evaluation order: torch.func vs nn.Module, other op sequence)
  oracle32b the same with oneDNN switched off (torch.backends.mkldnn: convolutions through im2col + sgemm - a third summation order)
  oracle64  oracle.ref_cpu.Adapter in fp64 - the noise-free trajectory (its own rounding is ~1e-16)

and per parameter tensor, for Adam's m and v and for theta_after - theta_before (and the teacher's drift):
  *_nd_*   | ||X32|| - ||X64|| | / ||X64||      - the deviation of the NORM (what the stream tests compare against the golden's norms)
  *_l2_*   ||X32 - X64|| / ||X64||              - the element-wise distance
  *_cos_*  cosine of the first 256 elements     - what the slice checks compare
Everything lands in tests/golden/g5_<tag>_noise.npz; tests derive their bounds from it (tests/conftest.py noise_bounds): a bound is
3 x the largest deviation either fp32 run shows in the tensor's class (stage x kind), so it is data, not a blanket 2e-2 / 5e-2 / 0.99.
ReLU-mask flips of near-zero activations and Adam's sign-like step (an element whose gradient is rounding noise still moves by ~lr)
are what the floor consists of; the file makes that a measurement instead of an assertion.

Per Adam step the same three statistics of the outer gradient the step applied (gstep_*), per frame those of the state after it
(frame_<q>_*), shaped [nsteps|nframes, 169]: the floor of tests/stream_evidence.py's frame-by-frame checks.

usage:  PYTHONDONTWRITEBYTECODE=1 python tools/make_noise.py [--only tag,tag] [--out tests/golden] [--verify-existing]
"""
from __future__ import annotations

import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.dont_write_bytecode = True

import make_golden as MG                        # noqa: E402  (stubs + the reference adaptor factory)
from dynaboa_amd import assets                  # noqa: E402
from oracle import ref_cpu as O                 # noqa: E402

FRAME_ONLY = dict(retrieval=0, lower_level_mixtrain=0, upper_level_mixtrain=0, use_meanteacher=0, use_motion=0, dynamic_boa=0,
                  use_temporal_losses_upper=0)


def streams():
    """tag -> (options, identity_pose, nframes, first_order)"""
    out = {
        "fo_inner3_frameonly": (dict(FRAME_ONLY, inner_step=3), False, 4, True),
        "fo_inner1_frameonly_identity": (dict(FRAME_ONLY, inner_step=1), True, 3, True),
        "fo_inner1_full": (dict(inner_step=1, interval=2, optim_steps=2), False, 5, True),
        "fo_inner1_full_forced": (dict(inner_step=1, interval=2, optim_steps=2, cos_sim_threshold=-1.0), False, 4, True),
        "fo_inner2_frameonly": (dict(FRAME_ONLY, inner_step=2), False, 2, True),
        # second order: the reference under learn2learn first_order=False, the oracle as Adapter(..., first_order=False)
        "so_inner2_frameonly": (dict(FRAME_ONLY, inner_step=2), False, 2, False),
        "so_inner3_frameonly": (dict(FRAME_ONLY, inner_step=3), False, 2, False),
        "so_inner1_full": (dict(inner_step=1, interval=2, optim_steps=2), False, 4, False),
    }
    for t in ("fo_inner1_full_gated", "fo_inner1_full_gated_b", "fo_inner1_full_gated_c"):
        p = os.path.join(ROOT, "tests", "golden", f"g5_{t}.npz")
        if os.path.exists(p):
            g = np.load(p)
            out[t] = (dict(inner_step=1, cos_sim_threshold=float(g["gate_threshold"])), False, int(g["nframes"]), True)
    return out


class Run:
    """One evaluation of a stream, advanced frame by frame so that the four evaluations can be compared step by step without keeping
    every step's gradient of every run: `on_grad(run, {name: grad})` is called before each Adam step with the outer gradient it applies,
    state() is the Adam state / drift after the frame."""
    steps: list
    names: list
    on_grad = None

    def _grad(self, gr):
        if self.on_grad is not None:
            self.on_grad(self, gr)


class RefRun(Run):
    """the REFERENCE's Adaptor.adaptation() in fp32 (tools/make_golden.py; its optimizer.step wrapped to expose p.grad)"""

    def __init__(self, opts, ident, first_order):
        self.use_teacher = bool(opts.get("use_meanteacher", 1))
        self.a, _ = MG.make_ref_adaptor(opts, identity_pose=ident, first_order=first_order)
        self.names = [n for n, _ in self.a.model.module.named_parameters()]
        self.theta0 = {n: p.detach().clone() for n, p in self.a.model.module.named_parameters()}
        MG.record_adam_steps(self.a, self.names, hook=self._grad)
        self.steps = []

    def frame(self, step):
        a = self.a
        a.global_step = step
        a.fit_losses = {}
        a.model.eval()
        a.adaptation(assets.make_frame(step, 1, seed=22))
        self.steps.append(a.optim_step_record[-1] if a.optim_step_record else 0)

    def state(self):
        a, names, theta0 = self.a, self.names, self.theta0
        st = a.optimizer.state
        pm = dict(zip(names, a.model.module.parameters()))
        res = dict(m={n: st[pm[n]]["exp_avg"].double() for n in names}, v={n: st[pm[n]]["exp_avg_sq"].double() for n in names},
                   d={n: pm[n].detach().double() - theta0[n].double() for n in names})
        if self.use_teacher:
            tm = dict(a.teacher.named_parameters())
            res["t"] = {n: tm[n].detach().double() - theta0[n].double() for n in names}
        return res


class OracleRun(Run):
    """oracle.ref_cpu.Adapter in `dtype` (mkldnn=False: convolutions without oneDNN; its adam_step wrapped to expose the gradient)"""

    def __init__(self, opts, ident, first_order, dtype, mkldnn=True):
        self.dtype, self.mkldnn = dtype, mkldnn
        mp = assets.make_smpl_mean_params(identity_pose=ident, seed=3)
        sd = assets.make_synthetic_checkpoint(22, mp, randomize_norm=True, prefix="")["model"]
        self.sd = {k: v.to(dtype) for k, v in sd.items()}
        T = O.smpl_tables_to_torch(assets.make_synthetic_smpl(0), dtype=dtype)
        gmm = {k: torch.from_numpy(v).to(dtype) for k, v in assets.load_gmm_prior().items()}
        self.ad = ad = O.Adapter(self.sd, T, gmm, opts, first_order=first_order)
        self.cast = lambda b: {k: (v.to(dtype) if torch.is_tensor(v) and v.is_floating_point() else v) for k, v in b.items()}
        ad.exemplar_fn = lambda step: self.cast(assets.make_exemplars(step, ad.o["sample_num"]))
        self.names = list(ad.theta)
        orig = ad.adam_step

        def adam_step(grads):
            self._grad(grads)
            return orig(grads)
        ad.adam_step = adam_step
        self.steps = []

    def frame(self, step):
        with torch.backends.mkldnn.flags(enabled=self.mkldnn):
            rec = self.ad.adapt_frame(self.cast(assets.make_frame(step, 1, seed=22)))
        self.steps.append(rec["extra_steps"])

    def state(self):
        ad, sd, names = self.ad, self.sd, self.names
        res = dict(m={n: ad.m[n].double() for n in names}, v={n: ad.v[n].double() for n in names},
                   d={n: ad.theta[n].detach().double() - sd[n].double() for n in names})
        if ad.o["use_meanteacher"]:
            res["t"] = {n: ad.teacher[n].double() - sd[n].double() for n in names}
        return res


def compare(x32, x64, names):
    nd, l2, cs = [], [], []
    for n in names:
        a, b = x32[n].flatten(), x64[n].flatten()
        nb = float(b.norm())
        nd.append(abs(float(a.norm()) - nb) / nb if nb > 0 else 0.0)
        l2.append(float((a - b).norm()) / nb if nb > 0 else 0.0)
        a2, b2 = a[:256], b[:256]
        den = float(a2.norm() * b2.norm())
        cs.append(float(a2 @ b2) / den if den > 0 else 1.0)
    return np.array(nd), np.array(l2), np.array(cs)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", default="")
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden"))
    ap.add_argument("--verify-existing", action="store_true",
                    help="before writing g5_<tag>_noise.npz, assert every key of the committed file comes back identical")
    args = ap.parse_args()
    torch.manual_seed(0)
    torch.set_num_threads(8)
    MG.install_stubs()
    S = streams()
    for tag in (args.only.split(",") if args.only else list(S)):
        opts, ident, nframes, first_order = S[tag]
        o64 = OracleRun(opts, ident, first_order, torch.float64)
        draws = (("ref", RefRun(opts, ident, first_order)), ("or", OracleRun(opts, ident, first_order, torch.float32)),
                 ("o2", OracleRun(opts, ident, first_order, torch.float32, mkldnn=False)))
        names = draws[0][1].names
        assert all(r.names == names for _, r in draws) and o64.names == names
        # frame by frame: the fp64 run first (its outer gradients of the frame kept), then each fp32 run compared with it step by step
        g64, gstep, step_frame, frames = [], {src: [] for src, _ in draws}, [], {src: [] for src, _ in draws}
        o64.on_grad = lambda run, gr: g64.append({n: gr[n].detach().double().clone() for n in names})

        def cmp_grad(src):
            def f(run, gr):
                gstep[src].append(compare({n: gr[n].detach().double() for n in names}, g64[len(gstep[src]) - k0[src]], names))
            return f
        for src, r in draws:
            r.on_grad = cmp_grad(src)
        for step in range(nframes):
            g64.clear()
            o64.frame(step)
            step_frame += [step] * len(g64)
            s64 = o64.state()
            k0 = {src: len(gstep[src]) for src, _ in draws}
            for src, r in draws:
                r.frame(step)
                assert len(gstep[src]) - k0[src] == len(g64), (tag, step, src)
                frames[src].append({q: compare(x, s64[q], names) for q, x in r.state().items()})
            del s64
        ref, o32, o32b = (r for _, r in draws)
        assert ref.steps == o32.steps == o64.steps == o32b.steps, (ref.steps, o32.steps, o32b.steps, o64.steps)      # the fp64 run takes the same path
        payload = dict(names=np.array(names), nframes=nframes, extra_steps=np.array(ref.steps))
        for q in ("m", "v", "d") + (("t",) if "t" in frames["ref"][-1] else ()):
            for src, _ in draws:
                nd, l2, cs = frames[src][-1][q]          # the end of the stream
                payload[f"{q}_nd_{src}"], payload[f"{q}_l2_{src}"], payload[f"{q}_cos_{src}"] = nd, l2, cs
            worst = np.maximum(np.maximum(payload[f"{q}_nd_ref"], payload[f"{q}_nd_or"]), payload[f"{q}_nd_o2"])
            i = int(np.argmax(worst))
            print(f"{tag:34s} {q}: norm deviation median {np.median(worst):.2e} max {worst.max():.2e} ({names[i]}); element-wise median "
                  f"{np.median(payload[f'{q}_l2_ref']):.2e} max {payload[f'{q}_l2_ref'].max():.2e}; worst slice cosine "
                  f"{min(payload[f'{q}_cos_ref'].min(), payload[f'{q}_cos_or'].min(), payload[f'{q}_cos_o2'].min()):.6f}", flush=True)
        # per Adam step (the outer gradient it applied) and per frame (the state after it), float32 [nsteps|nframes, 169]:
        # gstep_{nd,l2,cos}_<src>, frame_<q>_{nd,l2,cos}_<src> (tests/stream_evidence.py)
        payload["step_frame"] = np.array(step_frame)
        for src, _ in draws:
            for j, kind in enumerate(("nd", "l2", "cos")):
                payload[f"gstep_{kind}_{src}"] = np.array([c[j] for c in gstep[src]], np.float32)
                for q in frames[src][0]:
                    payload[f"frame_{q}_{kind}_{src}"] = np.array([f[q][j] for f in frames[src]], np.float32)
        worst = np.max([payload[f"gstep_nd_{src}"] for src, _ in draws], axis=0)
        k, i = np.unravel_index(int(np.argmax(worst)), worst.shape)
        print(f"{tag:34s} outer gradient per step: norm deviation median {np.median(worst):.2e} max {worst.max():.2e} "
              f"(step {k}, {names[i]}); worst slice cosine {min(payload[f'gstep_cos_{s}'].min() for s, _ in draws):.6f}", flush=True)
        path = os.path.join(args.out, f"g5_{tag}_noise.npz")
        if args.verify_existing:
            MG.verify_existing(path, payload)
        np.savez_compressed(path, **payload)


if __name__ == "__main__":
    main()
