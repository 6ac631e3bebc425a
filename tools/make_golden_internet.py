#!/usr/bin/env python3
"""Goldens of the internet-video path's host side, from the REFERENCE's own code (imported read-only through the stub recipe of
tools/make_golden.py):

  tests/golden/g10_internet_detections.json   a small synthetic AlphaPose file: two tracks over 8 frames of a 1280 x 720 video, a
                                              detection without ``idx``, detections that fail the score test, detections that fail
                                              the height test, joints below 0.3 confidence (also straddling it), one person whose box
                                              leaves the frame
  tests/golden/g10_internet_extract.npz       what the reference's ``utils/data_preprocess/internet_data.py::internet_data_extract``
                                              writes for that file (imgname, center, scale, part)
  tests/golden/g10_internet_items.npz         the reference's ``Internet_dataset.__getitem__`` for those rows: ``smpl_j2d`` (its
                                              ``j2d_processing``) and ``bbox``; ``cv2``, ``torchvision`` and ``crop`` are stubbed as in the
                                              other goldens (the image half is the crop kernel's own tests')

  tests/golden/g10_internet_stream_<tag>.npz  the reference's ``dynaboa_internet.Adaptor.adaptation`` + ``inference`` on seeded synthetic
                                              frames (``dynaboa_amd.internet.synthetic_frame``: COCO-shaped keypoints, exact zeros in the
                                              7 unmapped joints of the window), 5 frames, interval 2, synthetic exemplars, the synthetic
                                              checkpoint / SMPL tables of ``make_golden.make_ref_adaptor``: per frame the logged loss terms,
                                              extra steps and gate checks, the dumped ``Pred`` dictionary, per-tensor norms of m, v,
                                              theta - theta0 and the teacher's drift; per Adam step the outer gradient's norms / slices
  tests/golden/g10_internet_stream_<tag>_noise.npz  the fp32 noise floor by the method of tools/make_noise.py (its Run classes): the
                                              reference in fp32, the oracle in fp32 with and without oneDNN, each against the oracle in fp64
Streams:  full_i2        dynamic_boa 0
          full_i2_gated  dynamic_boa 1, optim_steps 2, threshold found on the reference run (probe / margin method of
                         make_golden_online.search_threshold): a frame leaves by convergence, a frame runs into the cut-off, every
                         decision >= 2 % of the threshold away from it

usage:  PYTHONDONTWRITEBYTECODE=1 python tools/make_golden_internet.py [--only host,full_i2,full_i2_gated] [--gate_threshold T] [--no-noise]
"""
from __future__ import annotations

import argparse
import json
import os
import shutil
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.dont_write_bytecode = True

import make_golden as MG                        # noqa: E402

SEQ = "g10seq"
# a standing person in units of its height (x to the person's left is +): COCO-17 order
POSE = np.array([[0.00, 0.06], [0.02, 0.04], [-0.02, 0.04], [0.05, 0.05], [-0.05, 0.05], [0.11, 0.18], [-0.11, 0.18], [0.15, 0.34],
                 [-0.15, 0.34], [0.17, 0.48], [-0.17, 0.48], [0.07, 0.52], [-0.07, 0.52], [0.08, 0.75], [-0.08, 0.75], [0.09, 0.97],
                 [-0.09, 0.97]])


def detections():
    rng = np.random.default_rng(1010)
    out = []

    def det(frame, track, x, y, height, score, conf=None, idx_form="list"):
        kp = np.concatenate([np.array([x, y]) + POSE * height + rng.normal(0, 2.0, (17, 2)), rng.uniform(0.4, 0.98, (17, 1))], 1)
        if conf is not None:
            for j, c in conf.items():
                kp[j, 2] = c
        rec = dict(image_id=f"{frame:06d}.png", category_id=1, keypoints=[round(float(v), 3) for v in kp.ravel()], score=score,
                   box=[0.0, 0.0, 0.0, 0.0])
        if idx_form == "list":
            rec["idx"] = [float(track)]
        elif idx_form == "scalar":
            rec["idx"] = track
        out.append(rec)

    for f in range(8):
        # track 0 walks to the right; low-confidence wrists on two frames, one joint exactly around the 0.3 threshold
        det(f, 0, 400 + 25 * f, 150, 420, 2.9 + 0.01 * f, conf={9: 0.12, 10: 0.29} if f in (2, 5) else {3: 0.3, 4: 0.300001})
        # track 1: tall and at the left edge - its square box leaves the frame on the left (and at the bottom from frame 4 on);
        # it ends after frame 5; frame 3 fails the score test
        if f < 6:
            det(f, 1, 60, 230 + 30 * f, 460, 2.2 if f == 3 else 3.1)
        # a small person in the background: fails the height test (with a good score)
        if f in (1, 6):
            det(f, 2, 900, 300, 180, 3.3)
        # a person whose visible joints span little although the detection is tall: most joints under 0.3 - the height test reads the
        # visible ones only
        if f == 4:
            det(f, 3, 1000, 100, 500, 3.0, conf={j: 0.1 for j in range(5, 17)})
        # detections without a track id (scalar idx on one record to cover that form)
        if f == 7:
            det(f, -1, 800, 120, 400, 2.7, idx_form="none")
            det(f, 5, 1100, 140, 380, 2.6, idx_form="scalar")
    return out


# ---------------------------------------------------------------------------------------- streams
STREAMS = {"full_i2": dict(inner_step=1, interval=2, dynamic_boa=0),
           "full_i2_gated": dict(inner_step=1, interval=2, dynamic_boa=1, optim_steps=2)}
NFRAMES = 5


def make_ref_internet_adaptor(opts_over):
    """dynaboa_internet.Adaptor without its __init__: the fields of make_golden.make_ref_adaptor, minus everything metric."""
    import tempfile as tf
    import torch
    import dynaboa_internet as DI                # reference module (stubs installed)
    from dynaboa_amd import assets
    from oracle import ref_cpu as O
    prior = MG.load_file("ref_prior", "utils/smplify/prior.py")
    opts = DI.parser.parse_args([])
    for k, v in opts_over.items():
        setattr(opts, k, v)
    opts.mixtrain = opts.lower_level_mixtrain or opts.upper_level_mixtrain
    a = DI.Adaptor.__new__(DI.Adaptor)
    a.options, a.device = opts, torch.device("cpu")
    a.exppath = tf.mkdtemp()
    os.makedirs(os.path.join(a.exppath, "result"), exist_ok=True)
    model, _ = MG.build_ref_hmr(randomize_norm=True, identity_pose=False)
    a.model = MG.MAMLStub(model, lr=opts.fastlr, first_order=True).eval()
    a.optimizer = torch.optim.Adam(a.model.parameters(), lr=opts.lr, betas=(opts.beta1, opts.beta2), foreach=False)
    teacher, _ = MG.build_ref_hmr(randomize_norm=True, identity_pose=False)
    for p in teacher.parameters():
        p.detach_()
    a.teacher = teacher
    a.gmm_f = prior.MaxMixturePrior(prior_folder=os.path.join(MG.REF, "data"), num_gaussians=8, dtype=torch.float32)
    a.smpl_neutral = MG.SMPLStub(O.smpl_tables_to_torch(assets.make_synthetic_smpl(0)))
    a.history, a.kp2dlosses_lower, a.kp2dlosses_upper, a.fit_losses = {}, [], {}, {}
    a.sims, a.feat_sims, a.global_step = [], {}, 0
    a.retrieval = lambda feature: assets.make_exemplars(a.global_step, opts.sample_num)
    return a


def stream_runs():
    import joblib
    import torch
    import make_noise as MN
    from dynaboa_amd import internet as I

    class RefRun(MN.Run):
        """The REFERENCE's dynaboa_internet.Adaptor: adaptation(), then inference() (which dumps Pred_{step}.pt)."""

        def __init__(self, opts):
            self.a = a = make_ref_internet_adaptor(opts)
            MG.record_exact_cosines(a)
            self.names = [n for n, _ in a.model.module.named_parameters()]
            self.theta0 = {n: p.detach().clone() for n, p in a.model.module.named_parameters()}
            MG.record_adam_steps(a, self.names, hook=self._grad)
            self.use_teacher, self.steps, self.frames = True, [], []

        def frame(self, step):
            a = self.a
            a.global_step, a.fit_losses = step, {}
            batch = I.synthetic_frame(step)
            a.model.eval()
            a.adaptation(batch)
            a.inference(batch, a.model)
            extra = int(a.optimized_step) if a.options.dynamic_boa else 0
            self.steps.append(extra)
            self.frames.append(dict(losses={k: float(v) for k, v in a.fit_losses.items()}, extra=extra, gate=MG.gate_checks(a, step),
                                    gate64=np.array(a.feat_sims64.get(step, [])), state=MG.frame_state(a, self.names, self.theta0),
                                    pred=joblib.load(os.path.join(a.exppath, "result", f"Pred_{step}.pt"))))
        state = MN.RefRun.state

    class OracleRun(MN.OracleRun):
        def frame(self, step):
            with torch.backends.mkldnn.flags(enabled=self.mkldnn):
                rec = self.ad.adapt_frame(self.cast(I.synthetic_frame(step)))
            self.steps.append(rec["extra_steps"])
    return RefRun, OracleRun


def probe(opts, threshold):
    RefRun, _ = stream_runs()
    r = RefRun(dict(opts, cos_sim_threshold=threshold))
    for n in range(NFRAMES):
        r.frame(n)
    return [1.0 - f["gate"][:, 12] for f in r.frames], r.steps


def search_threshold(opts):
    """make_golden_online.search_threshold at this stream."""
    K = opts["optim_steps"]
    forced, _ = probe(opts, -1.0)
    vals = np.sort(np.concatenate(forced))
    print("forced-run 1-cos:", vals, flush=True)
    best = None
    for i in range(len(vals) - 1):
        if vals[i + 1] <= vals[i] * 1.05 or vals[i] <= 0:
            continue
        t = float(0.5 * (vals[i] + vals[i + 1]))
        checks, steps = probe(opts, t)
        m = MG.gate_margin(checks, t)
        ok = any(1 <= s <= K for s in steps) and any(s == K + 1 for s in steps) and m >= 0.02
        print(f"  candidate {t:.9e}: margin {m:.3%} steps {steps} {'ok' if ok else ''}", flush=True)
        if ok and (best is None or m > best[1]):
            best = (t, m)
            if m >= 0.05:
                break
    assert best is not None
    return best[0]


def run_stream(tag, out, opts, noise=True):
    import torch
    import make_noise as MN
    RefRun, OracleRun = stream_runs()
    ref = RefRun(opts)
    names = ref.names
    draws = [("ref", ref)]
    if noise:
        o64 = OracleRun(opts, False, True, torch.float64)
        draws += [("or", OracleRun(opts, False, True, torch.float32)), ("o2", OracleRun(opts, False, True, torch.float32, mkldnn=False))]
        g64, gstep, frames = [], {s: [] for s, _ in draws}, {s: [] for s, _ in draws}
        o64.on_grad = lambda run, gr: g64.append({n: gr[n].detach().double().clone() for n in names})
        k0 = {}
        for src, r in draws:
            r.on_grad = (lambda src: lambda run, gr: gstep[src].append(
                MN.compare({n: gr[n].detach().double() for n in names}, g64[len(gstep[src]) - k0[src]], names)))(src)
    for n in range(NFRAMES):
        if noise:
            g64.clear()
            o64.frame(n)
            s64 = o64.state()
            k0.update({src: len(gstep[src]) for src, _ in draws})
        for src, r in draws:
            r.frame(n)
            if noise:
                assert len(gstep[src]) - k0[src] == len(g64) and r.steps[-1] == o64.steps[-1], (tag, n, src, r.steps, o64.steps)
                frames[src].append({q: MN.compare(x, s64[q], names) for q, x in r.state().items()})
        print(f"{tag} frame {n}: extra {ref.steps[-1]} losses {ref.frames[-1]['losses']}", flush=True)
    a, K = ref.a, int(opts.get("optim_steps", 0)) if opts.get("dynamic_boa") else 0
    keys = sorted({k for f in ref.frames for k in f["losses"]})
    st = ref.state()
    payload = dict(nframes=NFRAMES, names=np.array(names), options=np.array([f"{k}={v}" for k, v in sorted(opts.items())]),
                   loss_keys=np.array(keys), losses=np.array([[f["losses"].get(k, np.nan) for k in keys] for f in ref.frames]),
                   extra_steps=np.array(ref.steps), adam_steps=len(a.adam_log["frame"]), step_frame=np.array(a.adam_log["frame"]),
                   gstep_norms=np.array(a.adam_log["norms"]), g1_norms=np.array(a.adam_log["norms"][0]),
                   frame_m_norms=np.array([f["state"]["m"] for f in ref.frames]), frame_v_norms=np.array([f["state"]["v"] for f in ref.frames]),
                   frame_delta_norms=np.array([f["state"]["d"] for f in ref.frames]),
                   frame_teacher_delta_norms=np.array([f["state"]["t"] for f in ref.frames]))
    for n in MG.STEP_SLICE_PARAMS:
        payload["gstep_" + n] = np.stack(a.adam_log["slices"][n]).astype(np.float32)
    for n in MG.SLICE_PARAMS:
        for q in st:
            payload[f"{q}_{n}"] = MG.head(st[q][n])
    for i, f in enumerate(ref.frames):
        for k, v in f["pred"].items():
            payload[f"pred{i}_{k}"] = np.asarray(v)
    if K:
        thr = float(opts["cos_sim_threshold"])
        gate, gate64 = np.full((NFRAMES, 1 + K), np.nan), np.full((NFRAMES, 1 + K), np.nan)
        for i, f in enumerate(ref.frames):
            gate[i, :len(f["gate"])] = f["gate"][:, 12]
            gate64[i, :len(f["gate64"])] = f["gate64"][:, 12]
        margin = MG.gate_margin([1.0 - f["gate"][:, 12] for f in ref.frames], thr)
        payload.update(gate_1mcos12=1.0 - gate, gate_cos12_64=gate64, gate_threshold=np.array(thr), gate_margin=np.array(margin),
                       gate_checks=np.array([len(f["gate"]) for f in ref.frames]))
        assert any(1 <= e <= K for e in ref.steps) and any(e == K + 1 for e in ref.steps) and margin >= 0.02, (ref.steps, margin)
    np.savez_compressed(os.path.join(out, f"g10_internet_stream_{tag}.npz"), **payload)
    print(f"g10_internet_stream_{tag} ok: extra steps {ref.steps}", flush=True)
    if noise:
        npay = dict(names=np.array(names), nframes=NFRAMES, extra_steps=np.array(ref.steps), step_frame=payload["step_frame"])
        for src, _ in draws:
            for q, (nd, l2, cs) in frames[src][-1].items():
                npay[f"{q}_nd_{src}"], npay[f"{q}_l2_{src}"], npay[f"{q}_cos_{src}"] = nd, l2, cs
            for j, kind in enumerate(("nd", "l2", "cos")):
                npay[f"gstep_{kind}_{src}"] = np.array([c[j] for c in gstep[src]], np.float32)
                for q in frames[src][0]:
                    npay[f"frame_{q}_{kind}_{src}"] = np.array([f[q][j] for f in frames[src]], np.float32)
        np.savez_compressed(os.path.join(out, f"g10_internet_stream_{tag}_noise.npz"), **npay)
        for q in ("m", "v", "d", "t"):
            w = np.max([npay[f"{q}_nd_{s}"] for s, _ in draws], axis=0)
            print(f"  noise {q}: norm deviation median {np.median(w):.2e} max {w.max():.2e}", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden"))
    ap.add_argument("--only", default="")
    ap.add_argument("--gate_threshold", type=float, default=None, help="full_i2_gated with a fixed threshold (the file's gate_threshold)")
    ap.add_argument("--no-noise", action="store_true")
    args = ap.parse_args()
    MG.install_stubs()
    todo = args.only.split(",") if args.only else ["host"] + list(STREAMS)
    if "host" in todo:
        host(args.out)
    if any(t in STREAMS for t in todo):
        import torch
        torch.manual_seed(0)
        torch.set_num_threads(8)
    for tag in [t for t in todo if t in STREAMS]:
        opts = dict(STREAMS[tag])
        if opts.get("dynamic_boa"):
            opts["cos_sim_threshold"] = args.gate_threshold if args.gate_threshold is not None else search_threshold(opts)
        run_stream(tag, args.out, opts, noise=not args.no_noise)


def host(out_dir):
    args = argparse.Namespace(out=out_dir)
    dets = detections()
    jpath = os.path.join(args.out, "g10_internet_detections.json")
    with open(jpath, "w") as fh:
        json.dump(dets, fh, separators=(",", ":"))
    tmp = tempfile.mkdtemp()
    try:
        shutil.copy(jpath, os.path.join(tmp, f"{SEQ}.json"))
        ext = MG.load_file("ref_internet_extract", "utils/data_preprocess/internet_data.py")
        ext.internet_data_extract(tmp)
        z = np.load(os.path.join(tmp, f"{SEQ}.npz"))
        extract = {k: z[k] for k in z.files}
    finally:
        shutil.rmtree(tmp)
    # np.savez stores the name list as a unicode array; keep it that way (allow_pickle stays off in the tests)
    np.savez_compressed(os.path.join(args.out, "g10_internet_extract.npz"), **extract)
    n = len(extract["imgname"])
    print("extract ok:", {k: v.shape for k, v in extract.items()}, "kept", n, "of", len(dets))

    import config                                # reference modules (stubs installed)
    ids = MG.load_file("ref_internet_dataset", "boa_dataset/internet_data.py")
    ds = ids.Internet_dataset.__new__(ids.Internet_dataset)
    ds.imgdir = os.path.join(config.InternetData_ROOT, "images")
    ds.normalize_img = lambda x: x
    ds.imgnames, ds.scales, ds.centers = extract["imgname"], extract["scale"], extract["center"]
    ds.smpl_j2ds = extract["part"].copy()        # (the reference rewrites this array in place: a copy, read once per row)
    ds.read_image = lambda imgname: np.zeros((720, 1280, 3), np.float32)
    ds.rgb_processing = lambda *a, **k: np.zeros((3, 224, 224), np.float32)
    items = [ds[i] for i in range(n)]
    assert [str(it["imgname"]) for it in items] == [str(x) for x in extract["imgname"]]
    np.savez_compressed(os.path.join(args.out, "g10_internet_items.npz"), smpl_j2d=np.stack([it["smpl_j2d"].numpy() for it in items]),
                        bbox=np.stack([np.asarray(it["bbox"], np.float64) for it in items]))
    print("items ok:", items[0]["smpl_j2d"].shape, items[0]["bbox"])


if __name__ == "__main__":
    main()
