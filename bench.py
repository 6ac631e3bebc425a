#!/usr/bin/env python3
"""Headline benchmark: adapted frames / s on MI355X.

    python bench.py --gpus N --steps K --warmup W
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N ... bench.py --gpus N --steps K --warmup W

One "step" = one pass of the per-frame bilevel adaptation (BASELINE.json metric: 3 inner steps +
1 outer step, batch 1, first-order, frame losses only = configs[1]) over one synthetic frame
already resident in HBM.  The default schedule is the reference-faithful one of
dynaboa_benchmark.py:126-157 (initial feature forward, inference() after every inner step and after
the outer step: 9 forwards + 4 backwards + 13 SMPL forwards per frame); nothing is skipped.
Each rank owns an independent replica + stream shard (weak scaling, no data-path collective;
SURVEY 8e); rank 0 prints ONE JSON line.

A plain run does what the headline needs and nothing else: set up, warm up, time the steps, write
--dump-outputs, print the line.  --full adds every other measurement, outside the headline's clock:
the conv roofline pass, the per-step percentile pass, the PCIe-inclusive pass, the sequences-per-GPU
sweep, the side configurations (each in a fresh process), the CPU baseline and, with N > 1 ranks,
the 3DPW operating point.  The --no_* switches and --percentile_frames trim a --full run.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time
import zlib

import numpy as np
import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

F_GFLOP = 8.195           # one HMR forward, B=1 (SURVEY 8 header)
B_GFLOP = 16.15           # dgrad + wgrad
MIN_SCHEDULE_GFLOP = 4 * (F_GFLOP + B_GFLOP) + F_GFLOP      # 105.6: algorithmic work per adapted frame
PEAK_FP32_MFMA_TFLOPS = 157.3                                # MI355X_MICROARCH.md
PEAK_BF16_MFMA_TFLOPS = 2500.0                               # dense bf16 MFMA, same guide

# the 53 convolutions as (count, H, W, Cin, Cout, k, stride, pad)
RESNET_CONVS = [
    (1, 224, 224, 4, 64, 7, 2, 3), (1, 56, 56, 64, 64, 1, 1, 0), (3, 56, 56, 64, 64, 3, 1, 1), (4, 56, 56, 64, 256, 1, 1, 0),
    (2, 56, 56, 256, 64, 1, 1, 0), (1, 56, 56, 256, 128, 1, 1, 0), (1, 56, 56, 128, 128, 3, 2, 1), (4, 28, 28, 128, 512, 1, 1, 0),
    (1, 56, 56, 256, 512, 1, 2, 0), (3, 28, 28, 512, 128, 1, 1, 0), (3, 28, 28, 128, 128, 3, 1, 1), (1, 28, 28, 512, 256, 1, 1, 0),
    (1, 28, 28, 256, 256, 3, 2, 1), (6, 14, 14, 256, 1024, 1, 1, 0), (1, 28, 28, 512, 1024, 1, 2, 0), (5, 14, 14, 1024, 256, 1, 1, 0),
    (5, 14, 14, 256, 256, 3, 1, 1), (1, 14, 14, 1024, 512, 1, 1, 0), (1, 14, 14, 512, 512, 3, 2, 1), (3, 7, 7, 512, 2048, 1, 1, 0),
    (1, 14, 14, 1024, 2048, 1, 2, 0), (2, 7, 7, 2048, 512, 1, 1, 0), (2, 7, 7, 512, 512, 3, 1, 1)]


# sources of the second-order-only kernels: the measured (first-order, 32-sequence) run never launches them
PMC_HASH_EXCLUDE = ("hvp_kernels.hip", "hvp_engine.inc")


def csrc_sha16():
    """Content hash of the kernel sources the benchmarked path is built from (dynaboa_amd/csrc/* minus PMC_HASH_EXCLUDE): PMC summaries
    under profiles/ carry the hash of the sources they were measured on, and a summary of other sources is not quoted (there is no
    .git on the GPU box to ask for a commit)."""
    import glob
    import hashlib
    h = hashlib.sha256()
    for f in sorted(glob.glob(os.path.join(ROOT, "dynaboa_amd", "csrc", "*.*"))):
        if f.endswith((".hip", ".inc", ".h")) and os.path.basename(f) not in PMC_HASH_EXCLUDE:
            h.update(os.path.basename(f).encode())
            h.update(open(f, "rb").read())
    return h.hexdigest()[:16]


def chain_stream(device):
    """The stream a frame chain is issued on.  DYB_CHAIN_PRIORITY = -1 gives it a high dispatch priority (the chain is the critical path,
    the library's auxiliary stream has slack): +0.7 % at 32 sequences (464.1 / 463.6 against 461.0 / 460.3 frames/s, alternating runs) - but a
    second-order autograd run issued on a high-priority stream sporadically falls to a FIFTH of its rate (6.7 instead of 31 frames/s,
    profiles/r04_sessions.txt s10; the runtime's high-priority queue against the engine's normal-priority side streams), so the default stays
    normal priority."""
    return torch.cuda.Stream(device=device, priority=int(os.environ.get("DYB_CHAIN_PRIORITY", "0")))


def pmc_traffic():
    """HBM bytes per launch (read + write) of the conv kernel family from the newest committed PMC summary
    (profiles/r*_pmc_igemm_traffic.json, written by tools/pmc_summarize.py from two rocprofv3 runs of THIS command:
    --pmc FETCH_SIZE and --pmc WRITE_SIZE, each in its own pass; reads x2 = the gfx950 correction, calibrated there on
    the 216 / 432 MB streaming kernels; writes calibrate exact).  A PMC pass cannot run inside the bench process, so the
    figure is the one of the commit named in the note; None if no summary is committed."""
    import glob
    try:
        path = sorted(glob.glob(os.path.join(ROOT, "profiles", "r*_pmc_igemm_traffic.json")))[-1]
        d = json.load(open(path))
        if d.get("csrc_sha16") != csrc_sha16():
            return dict(bytes=None, note="the newest PMC summary (%s) was measured on other kernel sources (csrc hash %s, now %s): not quoted" %
                                         (os.path.relpath(path, ROOT), d.get("csrc_sha16", d.get("commit", "?")), csrc_sha16()))
        return dict(bytes=float(d["hbm_bytes_per_launch"]),
                    note="HBM read (FETCH_SIZE x2) + write (WRITE_SIZE) bytes per conv launch from %s, measured on these kernel sources "
                         "(csrc hash %s)" % (os.path.relpath(path, ROOT), d["csrc_sha16"]))
    except Exception:      # noqa: BLE001
        return None


def mfma_busy():
    """MFMA-pipe busy fraction of the throughput conv kernel family from the newest committed SQ-counter summary
    (profiles/r*_pmc_sq_A_tp.json: rocprofv3 --pmc SQ_VALU_MFMA_BUSY_CYCLES ... GRBM_GUI_ACTIVE, own pass, no tracing):
    sum over launches of busy cycles / (kernel cycles x 1024 SIMDs); GRBM_GUI_ACTIVE is summed over the 8 XCDs."""
    import glob
    try:
        path = sorted(glob.glob(os.path.join(ROOT, "profiles", "r*_pmc_sq_tp.json")))[-1]
        d = json.load(open(path))
        if d.get("_csrc_sha16") != csrc_sha16():
            return dict(value=None, note="the newest SQ-counter summary (%s) was measured on other kernel sources: not quoted" % os.path.relpath(path, ROOT))
        busy = cyc = 0.0
        for k, v in d.items():
            if k.startswith("igemm_tp_kernel") and isinstance(v, dict) and "SQ_VALU_MFMA_BUSY_CYCLES" in v and "GRBM_GUI_ACTIVE" in v:
                busy += v["SQ_VALU_MFMA_BUSY_CYCLES"] * v["launches"]
                cyc += v["GRBM_GUI_ACTIVE"] * v["launches"]
        if cyc <= 0:
            return None
        return dict(value=busy / (cyc / 8.0 * 1024.0),
                    note="SQ_VALU_MFMA_BUSY_CYCLES / (GRBM_GUI_ACTIVE / 8 XCDs x 1024 SIMDs) over every igemm_tp_kernel launch of a "
                         "32-sequence run, from %s (PMC pass: kernels serialised; padded tile rows count as busy)" % os.path.relpath(path, ROOT))
    except Exception:      # noqa: BLE001
        return None


HBM_ALGORITHMIC_GB_PER_FRAME = 3.4     # SURVEY 8(d), weights-side algorithmic bytes per adapted frame (bs=1, first order, frame losses)
PEAK_HBM_GBPS = 8000.0                 # MI355X_MICROARCH.md: HBM3E ~8 TB/s


def conv_roofline(run, lo, hi, main_stream):
    """Dominant kernel family = igemm_mfma_kernel<fwd|dgrad|wgrad, with/without the GroupNorm loaders>.
    Measured IN the path: frames [lo, hi) of the same loop are run once more with a timing scope open on the
    issuing thread, inside which the library times every conv launch on its own dispatch (HIP start/stop
    events carried by the launch itself, on whichever stream - main or the weight-gradient side stream -
    it was issued to), whichever host thread issued it (main, autograd, metric worker)."""
    import ctypes
    from dynaboa_amd import _lib
    lib = _lib.load()
    nfr = hi - lo
    if lib.dyb_conv_timing_begin(int(nfr * 6000)) != 0:
        return None
    with torch.cuda.stream(main_stream):
        run(lo, hi)
    torch.cuda.synchronize()
    ms, n, flop, nbytes = ctypes.c_double(), ctypes.c_longlong(), ctypes.c_double(), ctypes.c_double()
    if lib.dyb_conv_timing_end(ctypes.byref(ms), ctypes.byref(n), ctypes.byref(flop), ctypes.byref(nbytes)) != 0 or n.value == 0:
        return None
    table = None
    if hasattr(lib, "dyb_conv_timing_table"):
        need = lib.dyb_conv_timing_table(None, 0)
        buf = ctypes.create_string_buffer(int(need))
        lib.dyb_conv_timing_table(buf, need)
        table = buf.value.decode()
    union_ms = float(lib.dyb_conv_timing_union_ms()) if hasattr(lib, "dyb_conv_timing_union_ms") else None
    return dict(table=table, achieved=flop.value / (ms.value * 1e-3) / 1e12, conv_ms_per_frame=ms.value / nfr,
                union_ms_per_frame=(union_ms / nfr if union_ms else None),
                achieved_while_running=(flop.value / (union_ms * 1e-3) / 1e12 if union_ms else None),
                launches_per_frame=n.value / nfr, avg_launch_us=ms.value * 1e3 / n.value,
                gflop_per_frame=flop.value / nfr / 1e9, algorithmic_bytes_per_launch=nbytes.value / n.value,
                sample_frames=nfr)


def cpu_baseline_worker(inner_step=3, budget_s=20.0, max_frames=6):
    """The oracle (a torch-CPU restatement of the reference, validated against it in the build
    container) on this host's cores, same synthetic stream and options, bounded sample.  One thread
    per physical core of one socket at most: oversubscribing all SMT threads of a 2-socket host makes
    batch-1 oneDNN convolutions crawl."""
    from oracle import ref_cpu as O
    from dynaboa_amd import assets
    cores = max(1, min(64, (os.cpu_count() or 8) // 2))
    torch.set_num_threads(cores)
    mp = assets.make_smpl_mean_params(identity_pose=True)
    sd = assets.make_synthetic_checkpoint(22, mp, prefix="")["model"]
    T = O.smpl_tables_to_torch(assets.make_synthetic_smpl(0))
    gmm = {k: torch.from_numpy(v) for k, v in assets.load_gmm_prior().items()}
    opts = dict(retrieval=0, lower_level_mixtrain=0, upper_level_mixtrain=0, use_meanteacher=0, use_motion=0, dynamic_boa=0,
                use_temporal_losses_upper=0, inner_step=inner_step)
    ad = O.Adapter(sd, T, gmm, opts)
    ad.adapt_frame(assets.make_frame(0, 1))
    t0 = time.time()
    n = 0
    while n < max_frames and (n < 2 or time.time() - t0 < budget_s):
        n += 1
        ad.adapt_frame(assets.make_frame(n, 1))
    dt = time.time() - t0
    return dict(value=n / dt, unit="adapted frames/s", cores=cores, kind="port",
                sample=f"{n} frames after 1 warm-up in {dt:.1f}s, inner_step={inner_step}, frame losses only, "
                       f"torch-CPU fp32 oracle (6 HMR forwards + 4 backwards per frame), torch threads={cores} of {os.cpu_count()} logical CPUs",
                schedule_note="the oracle shares the forwards the reference repeats with identical weights: 6 HMR forwards + 4 backwards per "
                              "frame where the reference's own loop runs 9 + 4 (dynaboa_benchmark.py:126-157) - favourable to the CPU by ~1.25x "
                              "in flops; the GPU path produces every output of the 9-forward schedule with 5 forwards (bit-identical sharing)")


def cpu_baseline(inner_step=3, timeout_s=240):
    """Run the worker in a child process so a pathological host cannot stall the benchmark."""
    import subprocess
    try:
        out = subprocess.run([sys.executable, os.path.abspath(__file__), "--cpu_baseline_only", "--inner_step", str(inner_step)],
                             capture_output=True, text=True, timeout=timeout_s, env=dict(os.environ, CUDA_VISIBLE_DEVICES="", HIP_VISIBLE_DEVICES=""))
        line = [l for l in out.stdout.splitlines() if l.startswith("{")][-1]
        return json.loads(line)
    except Exception as e:        # noqa: BLE001
        return dict(value=None, unit="adapted frames/s", cores=None, kind="port", sample=f"cpu baseline did not finish: {type(e).__name__}")


def self_spawn(n, argv):
    """`python bench.py --gpus N` without a launcher: re-exec under torch.distributed.run, one rank per GPU."""
    import socket
    import subprocess
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={n}", "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.abspath(__file__)] + argv
    return subprocess.call(cmd, env=dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY=os.environ.get("HSA_ENABLE_IPC_MODE_LEGACY", "0")))


_BUNDLE = {}


def _bundle(resident_exemplars=False):
    """The seeded synthetic asset bundle (checkpoint, SMPL models, exemplar generator): generated once per process - every
    adaptor copies what it needs into its own device arenas, so the 32+ sequences of a run can share the host-side source
    (1.1 s per adaptor otherwise).  resident_exemplars (opt-in): the retrieved exemplars of a step live on the device and are
    shared by all sequences; off (default) every sequence's retrieval() uploads its own copy from host memory inside the clock, as the
    reference does (base_adaptor.py:82-96)."""
    key = "res" if resident_exemplars else "b"
    if key not in _BUNDLE:
        from dynaboa_amd.base_adaptor import synthetic_bundle
        _BUNDLE[key] = synthetic_bundle(seed=22, identity_pose=True, resident_exemplars=bool(resident_exemplars))
    return _BUNDLE[key]


def build_adaptor(device, batch, inner_step, full_losses=0, second_order=0, share_forwards=1, overlap=2, schedule="faithful",
                  **over):
    from dynaboa_amd import benchmark as DB
    if full_losses:
        o = DB.parser.parse_args([])
        o.inner_step = inner_step
    else:
        o = DB.frame_only_options(inner_step=inner_step)
    o.batch_size = batch
    o.second_order = second_order
    o.share_forwards = share_forwards
    o.deferred_metrics = 1
    o.overlap_metrics = overlap
    o.eval_lower = 1 if schedule == "faithful" else 0
    resident = bool(over.pop("resident_exemplars", 0))
    for k, v in over.items():
        setattr(o, k, v)
    return DB.Adaptor(o, _bundle(resident), device=device)


class Runner:
    """What is timed: `seqs` independent sequences on this GPU, one frame step at a time.  seqs = 1: one Adaptor walking
    its stream (adaptation() per frame); seqs > 1: a ReplicaGroup - every sequence owns its weights / Adam state / records
    and its own frames, the native stepper issues ONE chain of launches per step covering all of them (per-sequence
    results bit-identical to running alone, tests)."""

    def __init__(self, device, seqs, batch, inner_step, nframes, rank=0, frame_base=0, groups=1, **kw):
        from dynaboa_amd import assets
        self.S, self.batch, self.device = seqs, batch, device
        self.G = groups if (seqs > 1 and groups > 1 and seqs % groups == 0) else 1
        mk = lambda r, s: {k: v.to(device) for k, v in assets.make_frame(rank * 100_000 + r * 7_000 + frame_base + s, batch, seed=22).items()}
        self.frames = [[mk(r, s) for s in range(nframes)] for r in range(seqs)]      # resident in HBM before any clock starts
        if (kw.get("full_losses") or kw.get("retrieval")) and not kw.get("resident_exemplars"):
            # the exemplar "dataset" of the synthetic bundle lives in pinned host memory before the clock starts (the reference's sits in
            # host RAM / on disk); every sequence's retrieval() still uploads its own copy inside the clock (base_adaptor.py:82-96)
            assets.pregenerate_exemplars(range(nframes), int(kw.get("sample_num", 1)))
        if seqs == 1:
            from dynaboa_amd import _lib
            _lib.load().dyb_set_option(b"rep_split", 0)
            self.ad = build_adaptor(device, batch, inner_step, **kw)
            self.ad.reset_records(nframes)
            self.grp = None
        else:
            from dynaboa_amd import _lib, native_step as NS
            kw = dict(kw, overlap=0)
            # several sequences per launch: let the split-K policy see the replica-multiplied grid (fewer slabs to write and
            # fold; +5..7 % measured).  Summation order then differs from a sequence running alone - results equal to fp32
            # rounding (test_replica_group_with_replica_aware_split); with rep_split = 0 they are bit-identical
            NS.set_replica_policy(True)          # (+ the throughput schedule from 5 sequences per launch: native_step.TP_MIN_SEQUENCES)
            self.ads = [build_adaptor(device, batch, inner_step, **kw) for _ in range(seqs)]
            per = seqs // self.G
            # G > 1: the sequences form G lockstep groups, each with its own stepper, issuing thread and stream, free-running
            # against each other - one group's streaming phases (GroupNorm backward, optimiser) overlap another's convolutions
            self.grps = [NS.ReplicaGroup(self.ads[g * per:(g + 1) * per], nframes) for g in range(self.G)]
            self.grp = self.grps[0]
            self.gstreams = [chain_stream(device) for _ in range(self.G)] if self.G > 1 else None
            self.ad = self.ads[0]

    def step(self, s):
        if self.grp is None:
            ad = self.ad
            ad.global_step = s
            ad.fit_losses = {}
            ad.model.eval()
            ad.adaptation(self.frames[0][s])
        else:
            self.grp.step([self.frames[r][s] for r in range(self.S)], s)

    def step_with_upload(self, s, pinned):
        """The same step with the frame's inputs handed over as pinned HOST buffers (what the reference's loop does every frame,
        dynaboa_benchmark.py:86 `.to(device)`): upload on the issuing stream, then the step."""
        dev = self.device
        # one upload per input kind for all sequences of the step (a stacked pinned buffer), not one per sequence and kind
        keys = list(pinned[0][s].keys())
        stacked = {k: pinned["stack"][s][k].to(dev, non_blocking=True) for k in keys}
        up = [{k: stacked[k][r] for k in keys} for r in range(self.S)]
        if self.grp is None:
            ad = self.ad
            ad.global_step = s
            ad.fit_losses = {}
            ad.model.eval()
            ad.adaptation(up[0])
        else:
            self.grp.step(up, s)

    def run_range(self, lo, hi, evs=None):
        """G > 1: every group walks steps [lo, hi) from its own host thread on its own stream; returns when all have issued,
        with the caller's current stream made to wait for them.  evs: group 0 records an event after each of its steps."""
        import threading
        per = self.S // self.G
        errs = []

        def work(g):
            try:
                torch.cuda.set_device(self.device)
                with torch.cuda.stream(self.gstreams[g]):
                    for s in range(lo, hi):
                        self.grps[g].step([self.frames[r][s] for r in range(g * per, (g + 1) * per)], s)
                        if evs is not None and g == 0:
                            e = torch.cuda.Event(enable_timing=True)
                            e.record(self.gstreams[g])
                            evs.append(e)
            except Exception as e:      # noqa: BLE001
                errs.append(e)
        cur = torch.cuda.current_stream(self.device)
        for gs in self.gstreams:
            gs.wait_stream(cur)
        th = [threading.Thread(target=work, args=(g,)) for g in range(self.G)]
        for t in th:
            t.start()
        for t in th:
            t.join()
        if errs:
            raise errs[0]
        for gs in self.gstreams:
            cur.wait_stream(gs)

    def flush(self):
        """-> list of per-sequence metric dicts"""
        if self.grp is None:
            return [self.ad.flush_metrics()]
        return [m for g in self.grps for m in g.flush_metrics()]

    def native(self):
        return all(a._native is not None for a in ([self.ad] if self.grp is None else self.ads))


def timed_stream(runner, warmup, steps, stream, dist=None, per_frame=False):
    """warmup untimed steps, then `steps` steps between barrier + device synchronise on both sides; the metric tail of
    the last frames and flush_metrics() - the Procrustes launch + the device-to-host transfer of the per-frame errors the
    reference performs inside every inference() - are INSIDE the clock.  per_frame: a HIP event after every step on the
    issuing stream gives the per-step completion intervals (p50 / p99)."""
    def run(lo, hi, evs=None):
        if getattr(runner, "G", 1) > 1:
            return runner.run_range(lo, hi, evs)
        for s in range(lo, hi):
            runner.step(s)
            if evs is not None:
                e = torch.cuda.Event(enable_timing=True)
                e.record(stream)
                evs.append(e)
    torch.cuda.synchronize()
    with torch.cuda.stream(stream):
        run(0, warmup)
        runner.flush()
    torch.cuda.synchronize()
    if dist is not None:
        dist.barrier()
    torch.cuda.synchronize()
    evs = [] if per_frame else None
    # The cyclic garbage collector stays out of the timed region (as `timeit` keeps it): after the ~300 adaptors this process builds
    # for its side runs a generation-2 pass walks a large heap, and the configurations whose steps end in a host wait (the default
    # term set's gate poll) then show the collector instead of the path - 309 - 333 frames/s as the tenth side run against 353 - 369
    # as a fresh process (profiles/r05_sessions.txt s18).  Reference counting still frees everything a step allocates.
    import gc
    gc.collect()
    gc_was = gc.isenabled()
    gc.disable()
    t0 = time.perf_counter()
    with torch.cuda.stream(stream):
        if evs is not None:
            e0 = torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            evs.append(e0)
        run(warmup, warmup + steps, evs)
        t_issue = time.perf_counter() - t0          # host finished issuing; GPU may still be draining
        metrics = runner.flush()                    # joins side work, Procrustes launch, D2H of the scalars
    torch.cuda.synchronize()
    if dist is not None:
        dist.barrier()
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    if gc_was:
        gc.enable()
    out = dict(dt=dt, t_issue=t_issue, metrics=metrics, run=run)
    if evs is not None:
        out["frame_ms"] = np.array([evs[i].elapsed_time(evs[i + 1]) for i in range(len(evs) - 1)])
    return out


def pa_mean(metrics):
    v = [np.atleast_1d(x) for m in metrics for x in m["pampjpe"]]
    return float(np.mean(np.concatenate(v))) if v else None


DUMP_WEIGHT_SAMPLE = 16384         # elements of each sequence's weight arena (and Adam moments) in --dump-outputs
DUMP_ARRAY_LIMIT = 1 << 20         # elements per dumped array: 12 arrays x 4 MB stay under the 64 MB a dump may take
DUMP_SEED = 20240611


def _dump_sample(a, seed):
    """`a` as float32, or a fixed seeded sample of DUMP_ARRAY_LIMIT of its elements (flattened, in index order) when it is larger."""
    a = np.ascontiguousarray(a, dtype=np.float32)
    if a.size <= DUMP_ARRAY_LIMIT:
        return a
    idx = np.sort(np.random.default_rng(seed).choice(a.size, DUMP_ARRAY_LIMIT, replace=False))
    return a.reshape(-1)[idx]


def dump_outputs(runner, metrics, out_dir):
    """--dump-outputs: what the timed loop's last step handed its caller, one float32 .npy per array under out_dir, read after the clock
    stopped and before any further step.  Per sequence (leading axis, in Runner order): the frame's errors from the metric flush
    (mpjpe / pampjpe [S][B] in mm, pve [S]), the final inference of the native stepper (pred_rotmat [S][B][24][3][3], pred_shape,
    pred_cam, pred_joints [S][B][49][3], pred_vertices [S][B][6890][3]) and the adapted weights with both Adam moments at a fixed seeded
    sample of DUMP_WEIGHT_SAMPLE positions of the parameter arena (theta / adam_m / adam_v [S][DUMP_WEIGHT_SAMPLE]; the whole arenas are
    ~100 MB per sequence).  The inputs are seeded, so two builds run with the same arguments can be compared file for file."""
    ads = [runner.ad] if runner.grp is None else runner.ads
    torch.cuda.synchronize()
    arrays = dict(mpjpe=[m["mpjpe"][-1] for m in metrics], pampjpe=[m["pampjpe"][-1] for m in metrics], pve=[m["pve"][-1] for m in metrics])
    # the stepper's output buffer holds a sequence's final inference unless a replica left the dynamic-BOA loop before the last launch
    # (full term set, several sequences: dyb_stepper_output follows the last launch's arena) - those runs dump no predictions
    if all(a._native is not None for a in ads) and not (ads[0]._native.full and len(ads) > 1):
        outs = [[a._native.output(k, a._native_replica).cpu().numpy() for k in range(4)] for a in ads]
        arrays.update(pred_rotmat=[o[0].reshape(-1, 24, 3, 3) for o in outs], pred_shape=[o[1][:, 144:154] for o in outs],
                      pred_cam=[o[1][:, 154:157] for o in outs], pred_vertices=[o[2] for o in outs], pred_joints=[o[3] for o in outs])
    thetas = [getattr(a.model, "module", a.model).theta for a in ads]
    n = thetas[0].numel()
    idx = torch.from_numpy(np.sort(np.random.default_rng(DUMP_SEED).choice(n, min(n, DUMP_WEIGHT_SAMPLE), replace=False))).to(thetas[0].device)
    arrays["theta"] = [t.detach()[idx].cpu().numpy() for t in thetas]
    for name, key in (("adam_m", "exp_avg"), ("adam_v", "exp_avg_sq")):
        arrays[name] = [a.optimizer.state[t][key][idx].cpu().numpy() for a, t in zip(ads, thetas)]
    os.makedirs(out_dir, exist_ok=True)
    total = 0
    for name, per_seq in sorted(arrays.items()):
        a = _dump_sample(np.stack([np.asarray(x, np.float32) for x in per_seq]), DUMP_SEED + zlib.crc32(name.encode()))
        np.save(os.path.join(out_dir, name + ".npy"), a)
        total += a.nbytes
    assert total <= 64 << 20, total


def replica_run(device, S, steps, warmup, batch, inner_step, rank=0, **kw):
    """Aggregate frames/s of S sequences in lockstep on one GPU (a short side run: see Runner).  S = 1, the latency
    configuration, runs 200 frames and also reports the per-frame completion intervals."""
    if S == 1:
        steps = max(steps, 200)
    n_roof = 8 if S == 1 else 0          # S = 1: the literal bs=1 stream gets its own roofline object
    rn = Runner(device, S, batch, inner_step, warmup + steps + n_roof, rank=rank, frame_base=3_000, **kw)
    st = chain_stream(device)
    r = timed_stream(rn, warmup, steps, st, per_frame=(S == 1))
    out = dict(value=S * steps * batch / r["dt"], unit="adapted frames/s", seqs=S, steps=steps, warmup=warmup,
               ms_per_step=r["dt"] * 1e3 / steps, host_issue_ms_per_step=r["t_issue"] * 1e3 / steps,
               pa_mpjpe_mm_synthetic_mean=pa_mean(r["metrics"]))
    if n_roof:
        c = conv_roofline(r["run"], warmup + steps, warmup + steps + n_roof, st)
        rn.flush()
        fps = out["value"]
        if c is not None:
            out["roofline"] = dict(
                bound="mfma", achieved=c["achieved"], peak=PEAK_FP32_MFMA_TFLOPS, unit="TFLOP/s", frac=c["achieved"] / PEAK_FP32_MFMA_TFLOPS,
                traffic=None, avg_launch_us=c["avg_launch_us"], launches_per_frame=c["launches_per_frame"],
                conv_ms_per_frame=c["conv_ms_per_frame"], conv_busy_ms_per_frame=c.get("union_ms_per_frame"),
                achieved_while_convs_run=c.get("achieved_while_running"),
                whole_frame_frac=MIN_SCHEDULE_GFLOP * fps / 1e3 / PEAK_FP32_MFMA_TFLOPS, sample_frames=n_roof,
                note="the conv family of ONE bs=1 stream, every launch timed on its own dispatch inside the path (same dyb_conv_timing_* pass "
                     "as the headline's roofline, latency-form kernels); whole_frame_frac = 105.3 GFLOP per frame x frames/s / peak")
        out["hbm_view"] = dict(bound="hbm", achieved=HBM_ALGORITHMIC_GB_PER_FRAME * fps, peak=PEAK_HBM_GBPS, unit="GB/s",
                               frac=HBM_ALGORITHMIC_GB_PER_FRAME * fps / PEAK_HBM_GBPS,
                               note="SURVEY 8(d): 3.4 GB of algorithmic weight-side traffic per adapted frame (weights read twice per "
                                    "forward+backward, gradient written, 3 fast-weight steps, clone, Adam, LBS tables) x frames/s against 8 TB/s: "
                                    "the one-stream frame is bound by neither roof but by its chain of dependent launches")
    if "frame_ms" in r:
        ft = r["frame_ms"]
        out["frame_time_ms"] = dict(mean=float(ft.mean()), p50=float(np.percentile(ft, 50)), p99=float(np.percentile(ft, 99)), max=float(ft.max()))
    return out


def sub_record(device, name, steps, warmup, batch, inner_step, note, roofline_peak=None, seqs=1, **kw):
    """One of the side configurations carried in the same JSON line, measured in a FRESH PROCESS (as a user would run it): the tenth
    configuration of one process inherits its predecessors' state - a large Python heap (the collector), and above all the HIP streams
    earlier steppers created, which shift how the runtime multiplexes this configuration's streams onto its hardware queues: after the
    one-sequence default-term-set run (two pass streams of its own, round 5) the later side runs lost 8 - 50 % in the same process and
    nothing as fresh processes (profiles/r05_sessions.txt s26 / s27).  DYB_BENCH_SUB_INPROC=1 keeps them in this process."""
    if os.environ.get("DYB_BENCH_SUB_INPROC") == "1":
        return sub_record_here(device, name, steps, warmup, batch, inner_step, note, roofline_peak, seqs, **kw)
    import subprocess
    spec = dict(name=name, steps=steps, warmup=warmup, batch=batch, inner_step=inner_step, note=note, roofline_peak=roofline_peak, seqs=seqs, kw=kw)
    try:
        out = subprocess.run([sys.executable, os.path.abspath(__file__), "--sub_record", json.dumps(spec)], capture_output=True, text=True, timeout=900)
        sys.stderr.write("".join(l + "\n" for l in out.stderr.splitlines() if l.startswith("[bench]")))
        line = [l for l in out.stdout.splitlines() if l.startswith("{")][-1]
        return json.loads(line)
    except Exception as e:      # noqa: BLE001
        return dict(value=None, error=f"side run in its own process: {type(e).__name__}: {e}", config=note)


def sub_record_here(device, name, steps, warmup, batch, inner_step, note, roofline_peak=None, seqs=1, **kw):
    """The side configuration itself (value + ms_per_step), a short run; with roofline_peak (TFLOP/s) also the conv family's in-path
    achieved rate against that peak (2 extra steps).  seqs > 1: that many sequences in lockstep (a ReplicaGroup), value = aggregate
    frames/s."""
    t_sub = time.perf_counter()
    try:
        extra = 2 if roofline_peak else 0
        rn = Runner(device, seqs, batch, inner_step, warmup + steps + extra, frame_base=500_000, **kw)
        st = chain_stream(device)
        r = timed_stream(rn, warmup, steps, st)
        out = dict(value=seqs * steps * batch / r["dt"], unit="adapted frames/s", ms_per_step=r["dt"] * 1e3 / steps, steps=steps,
                   warmup=warmup, batch=batch, inner_step=inner_step, host_issue_ms_per_step=r["t_issue"] * 1e3 / steps,
                   native_stepper=rn.native(), config=note)
        if seqs > 1:
            out["sequences_per_gpu"] = seqs
            ads = rn.ads
            if getattr(ads[0], "optim_step_record", None):
                out["dynamic_loop_extra_steps_mean"] = float(np.mean([np.mean(a.optim_step_record) for a in ads if a.optim_step_record]))
        elif getattr(rn.ad, "optim_step_record", None):
            out["dynamic_loop_extra_steps_mean"] = float(np.mean(rn.ad.optim_step_record))
        if roofline_peak:
            c = conv_roofline(r["run"], warmup + steps, warmup + steps + extra, st)
            rn.flush()
            if c is not None:
                out["roofline"] = dict(bound="mfma", achieved=c["achieved"], peak=roofline_peak, unit="TFLOP/s",
                                       frac=c["achieved"] / roofline_peak, avg_launch_us=c["avg_launch_us"],
                                       conv_ms_per_step=c["conv_ms_per_frame"])
        print("[bench] side run %s: %.1f s" % (name, time.perf_counter() - t_sub), file=sys.stderr)
        return out
    except Exception as e:      # noqa: BLE001
        return dict(value=None, error=f"{type(e).__name__}: {e}", config=note)


def calibrate_gate_threshold(device, frames=5):
    """A cos_sim_threshold at which the dynamic-BOA loop (dynaboa_benchmark.py:161-192) takes 2-3 extra upper-level steps per frame on
    THIS synthetic stream, as it does on real video (the default 3.1e-4 never opens it here): a few frames with the gate forced open
    (threshold -1: every frame takes all optim_steps), then the median over frames of 1 - cos(feature 12) at the check after the third
    extra step (frames whose feature still moves more than that continue)."""
    rn = Runner(device, 1, 1, 1, frames, frame_base=700_000, full_losses=1, cos_sim_threshold=-1.0)
    st = chain_stream(device)
    with torch.cuda.stream(st):
        for s_ in range(frames):
            rn.step(s_)
        rn.flush()
    torch.cuda.synchronize()
    nat = rn.ad._native
    gl = nat.gate_log[0, :frames, :, 12].detach().cpu().numpy().astype(np.float64)       # [frame][check] cos of feature 12
    d = np.maximum(1.0 - gl, 1e-12)
    thr = float(np.median(d[:, 3]))
    # the forced run adapts harder than a gated one, so refine on gated probes: bisect the threshold (log scale) until a probe takes 2-3
    # extra steps per frame on average
    lo, hi, tried = thr / 4.0, thr * 1.5, []
    for _ in range(6):
        # (the probe IS the one-sequence side run below: same frames - sub_record's frame_base -, 4 warm-up + 16 counted frames)
        rn = Runner(device, 1, 1, 1, 20, frame_base=500_000, full_losses=1, cos_sim_threshold=thr)
        with torch.cuda.stream(st):
            for s_ in range(20):
                rn.step(s_)
            rn.flush()
        torch.cuda.synchronize()
        m = float(np.mean(rn.ad.optim_step_record)) if rn.ad.optim_step_record else 0.0      # (over all 20 frames, as the side run reports it)
        tried.append((thr, m))
        if 2.0 <= m <= 3.0:
            break
        if m < 2.0:
            hi = thr
        else:
            lo = thr
        thr = float(np.sqrt(lo * hi))
    thr = min(tried, key=lambda t: abs(t[1] - 2.5))[0]                  # the probed threshold closest to the target
    return thr, dict(one_minus_cos12_by_check_forced=d.tolist(), probes=tried)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=60)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--batch", type=int, default=1)
    ap.add_argument("--inner_step", type=int, default=3)
    ap.add_argument("--schedule", choices=["faithful", "minimal"], default="faithful")
    ap.add_argument("--full_losses", type=int, default=0, help="1: the reference's default term set (teacher+motion+exemplars+dynamic loop)")
    ap.add_argument("--overlap", type=int, default=2,
                    help="1: metric / feature forwards on a side HIP stream (same results); 2: also issued from a second host thread")
    ap.add_argument("--share_forwards", type=int, default=1,
                    help="0: re-run the forwards the reference schedule repeats with identical weights (9 instead of 5 per frame)")
    ap.add_argument("--second_order", type=int, default=0,
                    help="1: second-order MAML (BASELINE config 5's ablation arm); the reference and the default run are first-order")
    ap.add_argument("--hvp", choices=["fd", "exact"], default="exact", help="second order: exact (tangent passes) or finite-difference Hessian-vector products")
    ap.add_argument("--full", action="store_true",
                    help="also the measurements beyond the headline (roofline, percentile and PCIe-inclusive passes, sequences-per-GPU sweep, "
                         "side configurations, CPU baseline; with --gpus N > 1 the 3DPW operating point)")
    ap.add_argument("--no_cpu_baseline", action="store_true")
    ap.add_argument("--no_roofline", action="store_true")
    ap.add_argument("--no_sub_records", action="store_true", help="skip the second-order / batch-8 / full-loss-set side runs")
    ap.add_argument("--seqs", type=int, default=32,
                    help="independent sequences per GPU in the timed run (each with its own weights / Adam state / records, batch "
                         "--batch each), stepped in lockstep by one chain of launches (the throughput configuration; second-order / full-loss runs use 1); "
                         "1 = the single-sequence latency configuration")
    ap.add_argument("--groups", type=int, default=1,
                    help="split the --seqs sequences into this many lockstep groups, each issued by its own host thread on its own stream")
    ap.add_argument("--replicas", type=str, default="1,2,4,5,8,16,37,48,64",
                    help="comma list: sequences-per-GPU sweep carried as a sub-record (short runs)")
    ap.add_argument("--percentile_frames", type=int, default=80, help="frames of the per-frame-time pass when --steps < 200")
    ap.add_argument("--probe", type=str, default="", help="mode,H,C,K,R: phase clocks of the throughput conv kernel for that layer (diagnostic)")
    ap.add_argument("--probe_out", type=str, default="")
    ap.add_argument("--conv_table", type=str, default="", help="write the per-shape conv timing table of the roofline leg (CSV) here")
    ap.add_argument("--cpu_baseline_only", action="store_true")
    ap.add_argument("--sub_record", type=str, default="", help="(internal) one side configuration as JSON: run it here, print its record")
    ap.add_argument("--seqs_full", type=int, default=0, help="1: --seqs also applies to --full_losses 1 (lab runs / traces of the replica-batched default term set)")
    ap.add_argument("--cos_sim_threshold", type=float, default=None, help="--full_losses 1: the dynamic-BOA gate's threshold (default: the reference's 3.1e-4)")
    ap.add_argument("--all_sub_records", action="store_true",
                    help="also the side runs whose kernels have not changed since round 3 (finite-difference HVP, batch 16 on the latency "
                         "schedule, the 32-sequence bf16 arm)")
    ap.add_argument("--dump-outputs", default="", metavar="DIR",
                    help="after the timed steps write what their last step computed (predictions, errors, a sample of the adapted weights) "
                         "as DIR/<name>.npy (rank 0)")
    args = ap.parse_args()
    if (args.conv_table or args.all_sub_records) and not args.full:
        ap.error("--conv_table and --all_sub_records belong to the --full run")
    if args.cpu_baseline_only:
        print(json.dumps(cpu_baseline_worker(args.inner_step)))
        return
    if args.sub_record:
        spec = json.loads(args.sub_record)
        dev = torch.device("cuda:0")
        torch.cuda.set_device(dev)
        if "tp_batch_min" in spec["kw"]:          # (the latency-schedule arm of the batch-16 comparison: a library switch, set in this process)
            from dynaboa_amd import _lib as _Ls
            _Ls.load().dyb_set_option(b"tp_batch_min", int(spec["kw"].pop("tp_batch_min")))
        print(json.dumps(sub_record_here(dev, spec["name"], spec["steps"], spec["warmup"], spec["batch"], spec["inner_step"], spec["note"],
                                         spec["roofline_peak"], spec["seqs"], **spec["kw"])))
        return

    if "WORLD_SIZE" not in os.environ and args.gpus > 1:
        sys.exit(self_spawn(args.gpus, sys.argv[1:]))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    if world != args.gpus:
        raise SystemExit(f"bench.py: --gpus {args.gpus} but WORLD_SIZE={world}: launch one rank per GPU "
                         f"(python -m torch.distributed.run --nproc-per-node {args.gpus} bench.py --gpus {args.gpus} ...)")
    dist = None
    if world > 1:
        import torch.distributed as dist
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        # DYB_BENCH_SMOKE_ONE_GPU=1: functional check of this N>1 control flow on a ONE-GPU box (all ranks on cuda:0 over
        # gloo, since RCCL refuses two ranks on one device) - never a measurement
        one_gpu = os.environ.get("DYB_BENCH_SMOKE_ONE_GPU") == "1"
        if one_gpu:
            local = 0
            dist.init_process_group("gloo", rank=rank, world_size=world)
        else:
            dist.init_process_group("nccl", rank=rank, world_size=world, device_id=torch.device(f"cuda:{local}"))
    device = torch.device(f"cuda:{local}")
    torch.cuda.set_device(device)
    if dist is not None and os.environ.get("DYB_BENCH_SMOKE_ONE_GPU") == "1":
        # several PROCESSES on one GPU are time-sliced: the workgroups of a GroupNorm slab that meet on a counter inside one launch are
        # then not co-resident for long stretches and the hand-off times out (the library counts it, the metric flush raises - round 5;
        # the first closing session's smoke run failed exactly so: 96 timed-out hand-offs).  One-workgroup slabs only in this mode.
        from dynaboa_amd import _lib as _L0
        _L0.load().dyb_set_option(b"tp_gn_onepass", 1)

    simple = not (args.second_order or args.full_losses)
    # replica groups cover the first-order configurations: frame losses (the headline) and, given explicitly, the default term set
    seqs = args.seqs if (simple or (args.full_losses and not args.second_order and args.seqs_full)) else 1
    total = args.warmup + args.steps
    # the extra passes below run with --full only; a plain run builds the frames of its warm-up and timed steps and no more
    n_roof = 4 if (args.full and not args.no_roofline) else 0      # extra steps for the instrumented roofline pass (outside the clock)
    n_pct = args.percentile_frames if (args.full and args.steps < 200 and args.percentile_frames > 0) else 0
    # extra steps of the PCIe-inclusive pass (outside the clock): as many timed steps as the headline (round 6: it used to time 5 steps, whose
    # end-of-run metric flush and drain weighed four times as much as in the headline's 20)
    n_h2d = max(6, min(args.steps, 40) + 1) if (args.full and not args.no_sub_records and simple and args.groups <= 1) else 0
    nfr = total + n_roof + n_pct + n_h2d
    rn = Runner(device, seqs, args.batch, args.inner_step, nfr, rank=rank, groups=args.groups, full_losses=args.full_losses,
                second_order=args.second_order, share_forwards=args.share_forwards, overlap=args.overlap, schedule=args.schedule,
                hvp=args.hvp, **({} if args.cos_sim_threshold is None else dict(cos_sim_threshold=args.cos_sim_threshold)))

    # the adaptation chain runs on a non-default stream: the engine's whole-call hipGraph cache cannot
    # capture on the legacy null stream
    main_stream = chain_stream(device)
    probe_buf = None
    if args.probe:
        from dynaboa_amd import _lib
        pm, pH, pC, pK, pR = (int(v) for v in args.probe.split(","))
        cap = 8192
        probe_buf = torch.zeros(cap * 4 * 8, dtype=torch.int64, device=device)
        _lib.load().dyb_conv_probe_set(probe_buf.data_ptr(), cap, pm, pH, pC, pK, pR)
    res = timed_stream(rn, args.warmup, args.steps, main_stream, dist, per_frame=(args.steps >= 200))
    if probe_buf is not None:
        torch.cuda.synchronize()
        _lib.load().dyb_conv_probe_set(None, 0, 0, 0, 0, 0, 0)
        rec = probe_buf.cpu().numpy().reshape(cap, 4, 8)
        rec = rec[rec[:, 0, 1] != 0]                      # workgroups of the last matching launch
        if len(rec):
            t0, t1 = rec[..., 0].min(), rec[..., 1].max()
            steps = np.maximum(rec[..., 6], 1).astype(np.float64)
            life = (rec[..., 1] - rec[..., 0]).astype(np.float64)
            pr = dict(workgroups=int(len(rec)), kernel_span_cycles=int(t1 - t0), ksteps_per_wg=float(steps.mean()),
                      wave_lifetime_cycles=dict(mean=float(life.mean()), min=float(life.min()), max=float(life.max())),
                      start_offset_cycles=dict(mean=float((rec[..., 0] - t0).mean()), max=float((rec[..., 0] - t0).max())),
                      per_kstep_cycles=dict(load_issue=float((rec[..., 2] / steps).mean()), mfma_block=float((rec[..., 3] / steps).mean()),
                                            wait_and_stage=float((rec[..., 4] / steps).mean()), barrier=float((rec[..., 5] / steps).mean())),
                      outside_loop_cycles=float((life - rec[..., 2:6].sum(-1)).mean()),
                      note="s_memtime clocks (100 MHz constant clock on gfx950 if REALTIME; else shader cycles) of lane 0 of every wave; "
                           "the MFMA block's time is the time to ISSUE its 32 MFMAs")
            print("PROBE " + json.dumps(pr), file=sys.stderr)
            if args.probe_out:
                json.dump(pr, open(args.probe_out, "w"), indent=1)
    dt, t_issue, metrics, run = res["dt"], res["t_issue"], res["metrics"], res["run"]
    if args.dump_outputs and rank == 0:
        dump_outputs(rn, metrics, args.dump_outputs)
    if dist is not None:
        t = torch.tensor([dt], device=device, dtype=torch.float64)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        dt = float(t.item())
        # end-of-stream gather of the per-frame errors over RCCL (the path's only collective)
        from dynaboa_amd.sharding import gather_frame_metrics
        v = [np.atleast_1d(x) for m in metrics for x in m["pampjpe"]]
        pa = torch.tensor(np.concatenate(v) if v else np.zeros(0), device=device, dtype=torch.float32)
        gathered = gather_frame_metrics(pa)
        cnt = [torch.zeros(1, device=device, dtype=torch.int64) for _ in range(world)]
        dist.all_gather(cnt, torch.tensor([pa.numel()], device=device, dtype=torch.int64))
        frames_per_rank = [int(c.item()) for c in cnt]
    else:
        gathered, frames_per_rank = None, None
    frames_done = args.steps * args.batch * seqs * world
    value = frames_done / dt

    if rank == 0:
        fwd_ref = (1 + 2 * args.inner_step + 2) if args.schedule == "faithful" else (args.inner_step + 3)
        # with forward sharing the identical-weight repeats (feature forward, per-inner-step inference) reuse a level forward
        fwd_pf = (args.inner_step + 2) if (args.share_forwards and not args.full_losses) else fwd_ref
        order = "second-order" if args.second_order else "first-order"
        how = ("%d independent sequences per GPU stepped in lockstep by one chain of launches (own weights / Adam state / records "
               "each, batch %d each; per-sequence results equal to running alone - bit-identical with the split policy of a "
               "single sequence, to fp32 rounding with the replica-aware one used here)" % (seqs, args.batch)) if seqs > 1 else \
              "one sequence per GPU"
        out = {"metric": "adapted frames/sec, whole job (%d inner + 1 outer step, bs=%d per sequence, %s; synthetic 224x224 stream, no 3DPW "
                         "assets in the image: PA-MPJPE on 3DPW not measured)" % (args.inner_step, args.batch, order),
               "value": value, "unit": "adapted frames/s", "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
               "ms_per_step": dt * 1e3 / args.steps, "host_issue_ms_per_step": t_issue * 1e3 / args.steps,
               "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
               "dtype": "f32", "data": "synthetic",
               "config": {"workload": "configs[1]: full bilevel adapt, synthetic 224x224 frames, bs=%d per sequence, %d inner + 1 outer, %s, %d seqs/GPU"
                                      % (args.batch, args.inner_step, order, seqs),
                          "workload_detail": "configs[1]: single MI355X full bilevel adapt on synthetic 224x224 frames, batch=%d, "
                                      "inner_step=%d + 1 outer, %s, %s; %s; a step = one frame of every sequence; schedule=%s: every "
                                      "output of the reference's %d-forward schedule is produced (metrics after each inner step when "
                                      "faithful), %d HMR forwards + %d backwards executed per frame%s; native frame stepper: %s; "
                                      "metric flush (Procrustes + D2H) inside the clock" %
                                      (args.batch, args.inner_step,
                                       ("second-order (exact Hessian-vector products: one tangent pass through the forward and one through the "
                                        "backward per inner step, beside the first-order passes)" if args.hvp == "exact" else
                                        "second-order (finite-difference Hessian-vector products: +2 forward+backward per inner step)")
                                       if args.second_order else "first-order (reference parity mode)",
                                       "reference default loss set" if args.full_losses else "frame losses only", how,
                                       args.schedule, fwd_ref, fwd_pf, args.inner_step + 1,
                                       " (forwards the reference repeats with identical weights and input are shared - bit-identical results)"
                                       if fwd_pf != fwd_ref else "", rn.native()),
                          "sequences_per_gpu": seqs, "lockstep_groups": getattr(rn, "G", 1), "global_batch": args.batch * seqs * world,
                          "parallelism": f"replicas{world} x {seqs} sequences (stream sharded by sequence)",
                          "per_gpu_frames_per_s": value / world,
                          "pa_mpjpe_mm_synthetic_mean": pa_mean(metrics),
                          "gathered_frames": int(gathered.numel()) if gathered is not None else None,
                          "gathered_frames_per_rank": frames_per_rank,
                          "gather_note": ("one ragged all-gather of the per-frame PA-MPJPE over %s at the end of the run (the path's only "
                                          "collective); gathered_frames must equal steps x seqs x n_gpus" %
                                          ("gloo (DYB_BENCH_SMOKE_ONE_GPU)" if os.environ.get("DYB_BENCH_SMOKE_ONE_GPU") == "1" else "RCCL"))
                          if gathered is not None else None,
                          "engine_graphs": __import__("dynaboa_amd.hmr", fromlist=["get_layout"]).get_layout(args.batch).graph_stats()}}
        if n_roof:
            lo = total
            torch.cuda.synchronize()
            r = conv_roofline(run, lo, lo + n_roof, main_stream)
            rn.flush()
        if n_roof and r is not None and args.conv_table and r.get("table"):
            with open(args.conv_table, "w") as f:
                f.write(r["table"])
        if n_roof and r is not None:
            tr = pmc_traffic()
            fr = n_roof * seqs
            out["roofline"] = {"bound": "mfma", "achieved": r["achieved"], "peak": PEAK_FP32_MFMA_TFLOPS, "unit": "TFLOP/s",
                               "frac": r["achieved"] / PEAK_FP32_MFMA_TFLOPS, "traffic": tr["bytes"] if tr else None,
                               "traffic_note": tr["note"] if tr else "no PMC summary under profiles/",
                               "algorithmic_bytes_per_launch": r["algorithmic_bytes_per_launch"],
                               "mfma_pipe_busy": mfma_busy(),
                               "kernel": "the convolution family - igemm_tp_kernel<fwd|dgrad|wgrad> (throughput form: launches covering >= 8 sequences), "
                                         "igemm_mfma_kernel / igemm_k4_* (latency form): every conv launch of the adaptation chain (main + "
                                         "weight-gradient streams; a launch covers all sequences of the step), timed on its own dispatch "
                                         "inside the path",
                               "sample_steps": r["sample_frames"], "sample_frames": fr,
                               "achieved_while_convs_run": r.get("achieved_while_running"),
                               "frac_while_convs_run": (r["achieved_while_running"] / PEAK_FP32_MFMA_TFLOPS) if r.get("achieved_while_running") else None,
                               "conv_busy_ms_per_step": r.get("union_ms_per_frame"),
                               "while_convs_run_note": "data- and weight-gradient launches run on two queues and share the chip, so their durations (the "
                                                       "denominator of `achieved`) add up to more than the time the chip spends on convolutions; "
                                                       "achieved_while_convs_run divides the same algorithmic flops by the UNION of the launches' "
                                                       "[start, stop] intervals (same HIP events)",
                               "avg_launch_us": r["avg_launch_us"], "launches_per_step": r["launches_per_frame"],
                               "conv_ms_per_step": r["conv_ms_per_frame"], "algorithmic_gflop_per_frame": r["gflop_per_frame"] / seqs,
                               "whole_frame_tflops_on_min_schedule": MIN_SCHEDULE_GFLOP * value / world / 1e3,
                               "whole_frame_frac": MIN_SCHEDULE_GFLOP * value / world / 1e3 / PEAK_FP32_MFMA_TFLOPS}
        # per-step completion intervals (HIP events on the issuing stream): from the timed run itself when it has >= 200
        # steps, else from an extra pass of `percentile_frames` steps of the same loop
        ft = res.get("frame_ms")
        if ft is None and n_pct:
            evs = []
            torch.cuda.synchronize()
            with torch.cuda.stream(main_stream):
                e0 = torch.cuda.Event(enable_timing=True)
                e0.record(main_stream)
                evs.append(e0)
                run(total + n_roof, total + n_roof + n_pct, evs)
                rn.flush()
            torch.cuda.synchronize()
            ft = np.array([evs[i].elapsed_time(evs[i + 1]) for i in range(len(evs) - 1)])
        if ft is not None and len(ft):
            out["frame_time_ms"] = {"steps": int(len(ft)), "mean": float(ft.mean()), "p50": float(np.percentile(ft, 50)),
                                    "p99": float(np.percentile(ft, 99)), "max": float(ft.max()),
                                    "how": "HIP event after every step (one frame of each of the %d sequences) on the issuing stream; "
                                           "intervals between consecutive events = time from a sequence's frame to its next" % seqs}
        if n_h2d:
            # PCIe-inclusive rate (never `value`): the same steps with every frame's inputs uploaded from pinned host memory inside the clock
            base = total + n_roof + n_pct
            pinned = {r: {s_: rn.frames[r][s_] for s_ in range(base, base + n_h2d)} for r in range(seqs)}
            pinned["stack"] = {s_: {k: torch.stack([rn.frames[r][s_][k] for r in range(seqs)]).cpu().pin_memory() for k in rn.frames[0][s_]}
                               for s_ in range(base, base + n_h2d)}
            torch.cuda.synchronize()
            with torch.cuda.stream(main_stream):
                rn.step_with_upload(base, pinned)                  # (first touch of the pinned buffers)
                torch.cuda.synchronize()
                t0h = time.perf_counter()
                for s_ in range(base + 1, base + n_h2d):
                    rn.step_with_upload(s_, pinned)
                rn.flush()
            torch.cuda.synchronize()
            dth = time.perf_counter() - t0h
            nb = sum(v.numel() * v.element_size() for v in pinned["stack"][base].values()) // seqs
            out["pcie_inclusive"] = {"value": (n_h2d - 1) * args.batch * seqs / dth, "unit": "adapted frames/s", "steps": n_h2d - 1,
                                     "ms_per_step": dth * 1e3 / (n_h2d - 1), "h2d_bytes_per_frame": nb,
                                     "note": "the headline loop with each frame's inputs (image, 2-D keypoints, ground-truth pose / shape / gender) "
                                             "uploaded from pinned host memory (one stacked buffer per input kind and step) on the issuing stream inside the clock, as the reference moves its "
                                             "batch every frame (dynaboa_benchmark.py:86); `value` above has the inputs resident in HBM"}
            del pinned
        if args.full and world == 1 and not args.no_sub_records and simple and args.batch == 1:
            del rn, run, res
            torch.cuda.empty_cache()
            reps = {}
            for S in [int(x) for x in args.replicas.split(",") if x.strip()]:
                if S == seqs:
                    continue
                try:
                    reps[f"S{S}"] = replica_run(device, S, max(12, args.steps // 2), 4, args.batch, args.inner_step)
                except Exception as e:      # noqa: BLE001
                    reps[f"S{S}"] = dict(value=None, error=f"{type(e).__name__}: {e}")
                torch.cuda.empty_cache()
            out["sequences_per_gpu_sweep"] = dict(
                note="aggregate frames/s with S independent sequences adapted in lockstep on this ONE GPU (batch 1 each, own weights / "
                     "Adam state / records; every launch of the per-frame chain covers all S); S1 = one sequence alone (the latency "
                     "configuration); the headline `value` uses S = %d" % seqs, **reps)
            out["second_order"] = sub_record(device, "second_order", 8, 2, 1, args.inner_step,
                                             "configs[1] second-order arm: one sequence, second_order=1, exact Hessian-vector products "
                                             "(tangent passes through the network, forward-over-reverse, both halves of every tangent pair in one conv launch; the default)", second_order=1,
                                             hvp="exact")
            # the two literal readings of BASELINE's metric as first-class keys: ONE bs=1 stream, first order and second order
            s1 = reps.get("S1") or {}
            out["single_stream"] = dict(value=s1.get("value"), unit="adapted frames/s", ms_per_step=s1.get("ms_per_step"),
                                        roofline=s1.get("roofline"), hbm_view=s1.get("hbm_view"),
                                        note="ONE sequence on the GPU, batch 1, 3 inner + 1 outer step, first order, frame losses: the literal "
                                             "'bs=1' reading of the metric (= sequences_per_gpu_sweep.S1)")
            s5 = reps.get("S5") or {}
            out["pw3d_operating_point"] = dict(value=s5.get("value"), unit="adapted frames/s", sequences_per_gpu=5, ms_per_step=s5.get("ms_per_step"),
                                               note="ceil(37 / 8) = 5 sequences per GPU: what an 8-GPU sharded run of the real 3DPW test stream (~37 "
                                                    "person tracks) keeps in flight per GPU (= sequences_per_gpu_sweep.S5; with --gpus N > 1 the timed loop "
                                                    "is re-run at ceil(37 / N) on all ranks)")
            if args.all_sub_records:
                out["second_order_fd_hvp"] = sub_record(device, "second_order_fd_hvp", 12, 3, 1, args.inner_step,
                                                        "the same with --hvp fd: Hessian-vector products as central differences of two "
                                                        "first-order gradients of the level (+2 forward+backward per inner step)",
                                                        second_order=1, hvp="fd")
            out["batch8_exemplars"] = sub_record(device, "batch8_exemplars", 10, 3, 8, args.inner_step,
                                                 "configs[2]: batch 8, lower+upper level labelled exemplars mixed in (S=8 per level), "
                                                 "first-order, frame losses + label term", retrieval=1, lower_level_mixtrain=1,
                                                 upper_level_mixtrain=1, sample_num=8)
            # configs[4] arms at batch 16 (one sequence): the throughput schedule (igemm_tp kernels, materialised dy) is the default from
            # batch 8 on (switch tp_batch_min = 8, round 5: measured crossover); the bf16 arm runs the bf16 form of the same kernel
            out["batch16_fp32_vs_bf16"] = dict(
                fp32=sub_record(device, "b16_fp32", 10, 3, 16, args.inner_step, "configs[4] arm: batch 16, first-order, frame losses, "
                                "fp32 MFMA (exact)", roofline_peak=PEAK_FP32_MFMA_TFLOPS),
                bf16=sub_record(device, "b16_bf16", 10, 3, 16, args.inner_step, "configs[4] arm: batch 16, first-order, frame losses, "
                                "bf16 MFMA for the convolutions, OPERAND ROUNDING ONLY: fp32 tensors in HBM and fp32 LDS tiles, operands rounded "
                                "to bf16 in registers right before v_mfma_f32_32x32x16_bf16 (fp32 master weights / activations / statistics / "
                                "accumulators) - NOT a bf16 data path: operand traffic is that of the fp32 kernel, so the arm is bound by loads / "
                                "LDS / fp32 GroupNorm + optimiser traffic, not by the bf16 matrix roof (VERDICT r5 item 9)",
                                roofline_peak=PEAK_BF16_MFMA_TFLOPS, bf16_mfma=1))
            __import__("dynaboa_amd.hmr", fromlist=["get_layout"]).get_layout(16).set_bf16(False)
            if args.all_sub_records:
                out["bf16_S32"] = sub_record(
                    device, "bf16_S32", 10, 3, 1, args.inner_step, "the headline workload (32 sequences in lockstep, first-order, frame losses) with the "
                    "convolutions on the bf16 matrix cores - NOT the parity configuration (operands rounded to bf16; fp32 master weights / activations / "
                    "statistics / accumulators)", roofline_peak=PEAK_BF16_MFMA_TFLOPS, seqs=32, bf16_mfma=1)
                __import__("dynaboa_amd.hmr", fromlist=["get_layout"]).get_layout(1).set_bf16(False)
            torch.cuda.empty_cache()
            out["batch16_first_vs_second_order"] = dict(
                first_order=dict(value=out["batch16_fp32_vs_bf16"]["fp32"].get("value"), unit="adapted frames/s",
                                 note="= batch16_fp32_vs_bf16.fp32"),
                second_order=sub_record(device, "b16_so", 6, 2, 16, args.inner_step, "configs[4] arm: batch 16, SECOND-order outer gradient "
                                        "(exact Hessian-vector products), frame losses, fp32", second_order=1, hvp="exact"))
            from dynaboa_amd import _lib as _L
            if args.all_sub_records:
                out["batch16_fp32_vs_bf16"]["fp32_latency_schedule"] = sub_record(
                    device, "b16_fp32_lat", 10, 3, 16, args.inner_step, "configs[4] arm: batch 16, fp32, the latency schedule (64x64 kernel, "
                    "GroupNorm backward in the loaders) that batches below 8 use (switch tp_batch_min = 0)", roofline_peak=PEAK_FP32_MFMA_TFLOPS,
                    tp_batch_min=0)
            out["full_default_losses"] = sub_record(device, "full_default_losses", 24, 6, 1, 1,
                                                    "the reference's default flags (inner_step 1, teacher + motion + labelled exemplars + "
                                                    "dynamic-BOA gate), ONE sequence - the configuration of the reference's published run",
                                                    full_losses=1)
            torch.cuda.empty_cache()
            out["full_default_losses_S32"] = sub_record(
                device, "full_default_losses_S32", 10, 3, 1, 1, "the reference's default flags (inner_step 1, teacher + motion + labelled "
                "exemplars + dynamic-BOA gate decided per sequence) for 32 sequences in lockstep on this GPU: teacher forward, history-frame "
                "pass and exemplar pass are replica-batched launches; a sequence whose gate has closed leaves the launch set of the "
                "remaining extra steps", roofline_peak=PEAK_FP32_MFMA_TFLOPS, seqs=32, full_losses=1)
            torch.cuda.empty_cache()
            # every default-term-set record above and below has each sequence's retrieval() upload its own exemplar copy from
            # (pinned) host memory inside the clock, as the reference does per level (base_adaptor.py:82-96).  This one is the round-5
            # arrangement, labelled: the step's exemplars resident on the device and shared by all 32 sequences
            out["full_default_losses_S32_exemplars_resident"] = sub_record(
                device, "full_default_losses_S32_exemplars_resident", 10, 3, 1, 1, "full_default_losses_S32 with EXEMPLARS RESIDENT: one generation + "
                "one upload per step shared by all 32 sequences (synthetic exemplars depend on the step only) - NOT what the reference does; "
                "round 5's 385 frames/s was measured this way", roofline_peak=None, seqs=32, full_losses=1, resident_exemplars=1)
            torch.cuda.empty_cache()
            # the same two configurations with the dynamic loop actually ENTERED: threshold calibrated on this stream
            try:
                thr, dtab = calibrate_gate_threshold(device)
                note = ("the reference's default flags with cos_sim_threshold = %.3e (calibrated on this synthetic stream so that the dynamic-BOA "
                        "loop takes 2-3 extra upper-level steps per frame, as on real video; with the default 3.1e-4 it never opens here)" % thr)
                out["full_default_losses_dynamic"] = sub_record(device, "full_default_losses_dynamic", 16, 4, 1, 1, note, full_losses=1,
                                                                cos_sim_threshold=thr)
                torch.cuda.empty_cache()
                out["full_default_losses_dynamic_S32"] = sub_record(device, "full_default_losses_dynamic_S32", 8, 2, 1, 1, note + "; 32 sequences in "
                                                                    "lockstep, the gate decided per sequence", roofline_peak=None,
                                                                    seqs=32, full_losses=1, cos_sim_threshold=thr)
                out["full_default_losses_dynamic"]["calibration"] = dtab
            except Exception as e:      # noqa: BLE001
                out["full_default_losses_dynamic"] = dict(value=None, error=f"{type(e).__name__}: {e}")
            torch.cuda.empty_cache()
            out["second_order_full_losses_exact_hvp"] = sub_record(
                device, "so_full_exact", 4, 1, 1, 1, "the reference's default term set in second-order mode with exact Hessian-vector "
                "products for every level (--hvp_terms all, the default: multi-pass form; parity: tests/test_adaptation_gpu.py "
                "test_second_order_full_loss_set_matches_reference_second_order)", full_losses=1, second_order=1, hvp="exact", hvp_terms="all")
    # N > 1: what the real 3DPW test stream can supply - 24 files / ~37 person tracks (utils/data_preprocess/pw3d.py:71-77) shared by
    # N ranks is ceil(37 / N) sequences per GPU, not 32; the same timed loop at that size (all ranks, barrier + max as above)
    if args.full and dist is not None and simple and args.batch == 1 and not args.no_sub_records:
        s_real = -(-37 // world)
        try:
            del rn
            torch.cuda.empty_cache()
            rn2 = Runner(device, s_real, args.batch, args.inner_step, 4 + 12, rank=rank, frame_base=500)
            r2 = timed_stream(rn2, 4, 12, chain_stream(device), dist)
            t = torch.tensor([r2["dt"]], device=device, dtype=torch.float64)
            dist.all_reduce(t, op=dist.ReduceOp.MAX)
            if rank == 0:
                out["pw3d_operating_point"] = {"value": 12 * s_real * world / float(t.item()), "unit": "adapted frames/s", "sequences_per_gpu": s_real,
                                               "ms_per_step": float(t.item()) * 1e3 / 12, "steps": 12, "warmup": 4,
                                               "note": "the timed loop with ceil(37 / n_gpus) sequences per GPU: 3DPW test has ~37 person tracks, so this - not "
                                                       "32 per GPU - is what a sharded run of the real stream can keep in flight"}
            del rn2
        except Exception as e:      # noqa: BLE001
            if rank == 0:
                out["pw3d_operating_point"] = dict(value=None, error=f"{type(e).__name__}: {e}")
    if rank == 0:
        if args.full and not args.no_cpu_baseline and world == 1:          # reported baseline: rank 0 at N=1 only
            out["cpu_baseline"] = cpu_baseline(inner_step=args.inner_step)
        # the literal one-stream readings as scalars right behind `value` (full records further down the line)
        front = ("metric", "value", "unit")
        line = {k: out[k] for k in front if k in out}
        if isinstance(out.get("single_stream"), dict):
            line["single_stream_frames_per_s"] = out["single_stream"].get("value")
        if isinstance(out.get("second_order"), dict):
            line["second_order_single_stream_frames_per_s"] = out["second_order"].get("value")
        line.update({k: v for k, v in out.items() if k not in front})
        print(json.dumps(line))
    if dist is not None:
        dist.barrier()
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
