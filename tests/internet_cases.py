"""The stream goldens of the internet-video driver (tests/golden/g10_internet_stream_<tag>.npz, tools/make_golden_internet.py: the
reference's ``dynaboa_internet.Adaptor.adaptation`` + ``inference`` on ``internet.synthetic_frame``) run through
``dynaboa_amd.internet.Adaptor`` frame by frame - shared by the GPU tests of tests/test_internet_gpu.py.

Bounds.  State (Adam's m and v, theta - theta0, the teacher's drift; per frame the per-tensor norms, at the end the slice cosines):
3 x the class floor measured in g10_internet_stream_<tag>_noise.npz (the reference in fp32, the oracle in fp32 with and without oneDNN,
each against the oracle in fp64), by conftest.noise_bounds' rule.  Step counts and gate decisions: exact.  Logged loss terms, gate
values and the dumped predictions are functions of one frame's forward, not accumulated state: they are held to what
tests/online_cases.py holds the same quantities of the online streams to (terms and predictions 1e-3 of themselves, the two small
difference terms - teacher, motion - 1e-2, a level's total 1e-4 as the g5 stream tests hold it, a gate value half its distance from the threshold and 1e-2 of itself)."""
import os

import numpy as np
import torch

from conftest import ADAM_SLICE_FLIP, NOISE_FACTOR, NOISE_MIN, cosine, golden, rel_err, tensor_class

STREAM_OPTS = {"full_i2": dict(inner_step=1, interval=2, dynamic_boa=0),
               "full_i2_gated": dict(inner_step=1, interval=2, dynamic_boa=1, optim_steps=2)}


def stream_noise_bounds(tag, names):
    """-> {q: dict(cos [169], frame_nd [nframes][169])}: NOISE_FACTOR x the largest deviation any fp32 draw shows over the tensor's
    class (stage x kind), never below NOISE_MIN (slice cosines of Adam-normalised quantities: ADAM_SLICE_FLIP)."""
    z = golden(f"g10_internet_stream_{tag}_noise.npz")
    assert [str(x) for x in z["names"]] == list(names)
    cls = [tensor_class(n) for n in names]

    def pooled(x):
        x = np.asarray(x, np.float64)
        out = np.empty_like(x)
        for c in set(cls):
            idx = [i for i, ci in enumerate(cls) if ci == c]
            out[..., idx] = x[..., idx].max(axis=-1, keepdims=True)
        return out
    res = {}
    for q in ("m", "v", "d", "t"):
        draws = [d for d in ("ref", "or", "o2") if f"{q}_nd_{d}" in z.files]
        assert draws, q
        cs = 1.0 - np.min([z[f"{q}_cos_{d}"] for d in draws], axis=0)
        fnd = np.max([z[f"frame_{q}_nd_{d}"] for d in draws], axis=0)
        cmin = ADAM_SLICE_FLIP if q in ("d", "t") else NOISE_MIN["cos"]
        res[q] = dict(cos=1.0 - np.maximum(cmin, NOISE_FACTOR * pooled(cs)), frame_nd=np.maximum(NOISE_MIN["nd"], NOISE_FACTOR * pooled(fnd)))
    return res


class InternetStream:
    """One golden stream through internet.Adaptor: mode 'autograd' (--native_results 0: prediction dumps route the run to the autograd
    composition) or 'native' (--native_results 1: the stepper, metrics 0, results from its ring)."""

    def __init__(self, tag, mode, expdir, device="cuda:0"):
        from dynaboa_amd import internet as I
        from dynaboa_amd.base_adaptor import synthetic_bundle
        self.tag, self.mode, self.g = tag, mode, golden(f"g10_internet_stream_{tag}.npz")
        g = self.g
        opts = dict(STREAM_OPTS[tag])
        if "gate_threshold" in g.files:
            opts["cos_sim_threshold"] = float(g["gate_threshold"])
        self.K = int(opts.get("optim_steps", 0)) if opts["dynamic_boa"] else 0
        o = I.parser.parse_args(["--expdir", str(expdir), "--expname", "stream", "--internet_root", str(expdir),
                                 "--native_results", "1" if mode == "native" else "0"])
        for k, v in opts.items():
            setattr(o, k, v)
        self.ad = ad = I.Adaptor(o, synthetic_bundle(seed=22, identity_pose=False, randomize_norm=True, smpl_seed=0), device=device)
        self.hmr = ad.model.module
        self.theta0 = self.hmr.theta.detach().clone()
        self.names = [str(x) for x in g["names"]]
        self.nb = stream_noise_bounds(tag, self.names)
        self.nframes = int(g["nframes"])
        ad.reset_records(self.nframes)
        os.makedirs(os.path.join(ad.exppath, "result"), exist_ok=True)
        self.n = 0

    def frame(self):
        import joblib
        from dynaboa_amd import internet as I
        ad, n = self.ad, self.n
        batch = {k: v.to(ad.device) if torch.is_tensor(v) else v for k, v in I.synthetic_frame(n).items()}
        ad.global_step, ad.fit_losses = n, {}
        ad.model.eval()
        ad.adaptation(batch)
        ad.write_frame_results(batch)
        if self.mode == "native":
            assert ad._native is not None and ad._native.full and ad._native_why == "", ad._native_why
        else:
            assert ad._native is None and ad._native_why == "prediction dumps", ad._native_why
        self.check_frame(joblib.load(os.path.join(ad.exppath, "result", f"Pred_{n}.pt")))
        self.n += 1

    def state(self):
        ad, hmr = self.ad, self.hmr
        st = ad.optimizer.state[hmr.theta]
        L = hmr._layout1
        return int(st["step"]), dict(m=L.unpack(st["exp_avg"]), v=L.unpack(st["exp_avg_sq"]),
                                     d=L.unpack((hmr.theta.detach().double() - self.theta0.double()).float()),
                                     t=L.unpack((ad.teacher.theta.detach().double() - self.theta0.double()).float()))

    def check_frame(self, pred):
        ad, g, n, K = self.ad, self.g, self.n, self.K
        log = {k: float(v.detach()) if torch.is_tensor(v) else float(v) for k, v in ad.fit_losses.items()}
        extra = int(g["extra_steps"][n])
        for k, ref in zip([str(x) for x in g["loss_keys"]], g["losses"][n]):
            if np.isnan(ref):
                continue
            # the reference stores the loss TENSOR under */unlabelloss and then adds the teacher, motion and labelled terms to it in
            # place (base_adaptor.py:247-266): what its log holds under that key at the end of the level is the level's total -
            # this project's */total (as tests/test_adaptation_gpu.py reads the g5 streams' upper_loss), held to that test's 1e-4
            total = k.endswith("/unlabelloss")
            ours = k.replace("/unlabelloss", "/total") if total else k
            assert ours in log, (n, ours, sorted(log))
            small = k.startswith("teacher/") or k == "ul/motion_loss"
            print(f"frame {n} {k}: {log[ours]:.8g} (reference {ref:.8g})")
            assert abs(log[ours] - ref) < (1e-4 if total else 1e-2 if small else 1e-3) * abs(ref), (n, k, log[ours], float(ref))
        if K:
            assert int(ad.optimized_step) == extra, (n, ad.optimized_step, extra)
            thr = float(g["gate_threshold"])
            sims = ad.feat_sims[ad.global_step]
            nchk = int(g["gate_checks"][n])
            assert len(sims) == nchk, (n, len(sims), nchk)
            for k in range(nchk):
                ours, refd = float(sims[k][12]["cos"]), float(g["gate_1mcos12"][n, k])
                dev = abs((1.0 - ours) - refd)
                print(f"frame {n} check {k}: 1 - cos {1.0 - ours:.6e} (reference {refd:.6e}, threshold {thr:.6e})")
                assert ((1.0 - ours) > thr) == (refd > thr), (n, k)
                assert dev < 0.5 * abs(refd - thr) and dev < 1e-2 * refd, (n, k, 1.0 - ours, refd, thr)
        assert sorted(pred) == ["beta", "cam", "rotmat", "verts"]
        for k in pred:
            ref = g[f"pred{n}_{k}"]
            assert pred[k].shape == ref.shape and pred[k].dtype == ref.dtype, (n, k, pred[k].shape, ref.shape)
            e = rel_err(pred[k], ref)
            print(f"frame {n} Pred {k}: {e:.2e}")
            assert e < 1e-3, (n, k, e)
        step, st = self.state()
        assert step == int((g["step_frame"] <= n).sum()), (n, step)
        for q, key in (("m", "frame_m_norms"), ("v", "frame_v_norms"), ("d", "frame_delta_norms"), ("t", "frame_teacher_delta_norms")):
            x = np.array([float(st[q][k].double().norm()) for k in self.names])
            ref = g[key][n]
            e = np.abs(x - ref) / np.where(ref > 0, ref, 1.0)
            b = self.nb[q]["frame_nd"][n]
            print(f"frame {n} {q}: worst norm deviation / bound {float((e / b).max()):.3f}")
            bad = [(self.names[j], float(e[j]), float(b[j])) for j in range(len(e)) if e[j] >= b[j]]
            assert not bad, (self.tag, n, q, "norm deviation beyond 3 x the class floor", bad[:6])

    def check_end(self):
        g = self.g
        step, st = self.state()
        assert step == int(g["adam_steps"])
        for k in [k[2:] for k in g.files if k.startswith("m_")]:
            j = self.names.index(k)
            for q in ("m", "d"):
                c = cosine(st[q][k].flatten()[:256].double().cpu().numpy(), g[f"{q}_{k}"])
                assert c > self.nb[q]["cos"][j], (self.tag, q, k, c, float(self.nb[q]["cos"][j]))


def run_stream(tag, mode, expdir):
    s = InternetStream(tag, mode, expdir)
    for _ in range(s.nframes):
        s.frame()
    s.check_end()
    return s
