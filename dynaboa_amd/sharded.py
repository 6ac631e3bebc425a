"""The sharded driver: the 3DPW test stream split by SEQUENCE over processes (one per GPU) and, inside a process, over sequence
replicas stepped in lockstep (dynaboa_amd.native_step.ReplicaGroup).

Reference: dynaboa_benchmark.py:83-123 walks ONE stream over all ``3dpw_<seq>_<pid>.npz`` files in order (boa_dataset/pw3d.py:19-35);
every frame's update depends on what the previous frame left, so the only parallel axis is the sequence.  Here
  * ``--num_shards N --shard_rank r`` (default 1 / 0 = the reference's single stream, the parity mode) assigns whole sequences to
    ranks with dynaboa_amd.sharding.assign_sequences over the files in the reference's order;
  * ``--seqs_per_gpu S`` adapts S of a rank's sequences at once, each with its own weights / Adam state / teacher / history /
    records (starting from the same checkpoint), in waves of S; sequences have different lengths - one whose stream has ended
    leaves the launch set (dyb_stepper_set_active), the others are not held back;
  * at the end every rank holds (global frame index, mpjpe, pampjpe, pve) of all frames: ONE ragged all_gather (RCCL over xGMI on
    the GPUs, gloo in the CPU tests), no collective on the data path.
With N > 1 or S > 1 every sequence starts from the checkpoint - what each has adapted on differs from the reference's single
stream, stated in DESIGN.md 6."""
from __future__ import annotations

import os
from typing import Callable, Dict, List, Optional, Sequence

import numpy as np
import torch

from .sharding import assign_sequences, gather_frame_metrics


class SequenceSpec:
    """One sequence of the stream: `frames()` yields its batches in order, `first` is the global index of its first frame."""

    def __init__(self, name: str, first: int, nframes: int, frames: Callable[[], object]):
        self.name, self.first, self.nframes, self.frames = name, int(first), int(nframes), frames


def pw3d_sequences(options, device) -> List[SequenceSpec]:
    """The reference's stream as sequences: one per 3dpw_<seq>_<pid>.npz, in the reference's file order."""
    from . import datasets as D
    ds = D.PW3D(options, img_dir=getattr(options, "pw3d_root", None) or D.PW3D_ROOT, device=device)
    out = []
    for s in ds.sequences:
        idx = list(range(s["first"], s["first"] + s["frames"]))
        out.append(SequenceSpec(s["file"], s["first"], s["frames"],
                                (lambda idx=idx: D.FrameLoader(ds, batch_size=options.batch_size, workers=4, indices=idx))))
    return out


def run_sharded(options, sequences: Sequence[SequenceSpec], make_adaptor: Callable[[], object], num_shards: int = 1, shard_rank: int = 0,
                seqs_per_gpu: int = 1, group=None) -> Dict[str, np.ndarray]:
    """Adapt this rank's sequences (waves of `seqs_per_gpu` in lockstep) and gather every rank's per-frame errors.
    make_adaptor() -> a fresh dynaboa_amd.benchmark.Adaptor at the base checkpoint.
    -> dict(global_index, mpjpe, pampjpe, pve): arrays over ALL frames of ALL ranks, sorted by global index, plus 'owned'
    (this rank's sequence indices) and 'frames_local'.  With options.seq_metrics the gathered row is 8 wide (+ accel, accel_counted,
    pck, auc): the dict gains those arrays and 'per_sequence' (one dict per sequence of the whole stream, in stream order), which
    every rank recomputes from the gathered rows - no second collective - and rank 0 writes the report files."""
    from . import native_step as NS
    from .base_adaptor import close_overlays
    seqm = bool(getattr(options, "seq_metrics", 0))
    W = 8 if seqm else 4
    owned = assign_sequences([s.nframes for s in sequences], num_shards)[shard_rank]
    B = int(getattr(options, "batch_size", 1))
    rows: List[np.ndarray] = []                      # (global frame index, mpjpe, pampjpe, pve) per frame
    # longest first inside a rank: a wave's sequences then have similar lengths (fewer idle replica slots at its tail)
    order = sorted(owned, key=lambda i: (-sequences[i].nframes, i))
    S = max(1, int(seqs_per_gpu))
    if S > 1 and B > 1 and any(sequences[i].nframes % B for i in owned):
        # a replica group stages B samples per sequence and step: a last, partial batch would be read past its end
        raise ValueError("seqs_per_gpu > 1 needs sequence lengths that are multiples of batch_size (or batch_size 1)")
    for w0 in range(0, len(order), S):
        wave = [sequences[i] for i in order[w0:w0 + S]]
        steps = max(-(-s.nframes // B) for s in wave)
        ads = [make_adaptor() for _ in wave]
        for a, s in zip(ads, wave):
            a.options.deferred_metrics = 1
            # --overlay_video 1: video/{prefix}_{sequence name}.avi (3DPW names its sequences by their .npz files' paths)
            a.sequence_name = os.path.splitext(os.path.basename(str(s.name)))[0]
            if seqm:
                a.options.seq_metrics, a._seq_report, a.seq_names = 1, False, [s.name]      # one report, for the whole run (below)
        # several sequences per GPU share one exppath: result files (--native_results 1 with --save_res / --dump_predictions) carry the
        # GLOBAL frame index - unique, and the reference's single-stream numbering.  Naming only: history / motion keep the local step
        number = S > 1 and bool(getattr(ads[0].options, "native_results", 0))
        if len(wave) == 1:
            def numbered(seq=wave[0], ad=ads[0]):
                for k, b in enumerate(seq.frames()):
                    ad._result_step = seq.first + k * B
                    yield b
            res = ads[0].excute(numbered() if number else wave[0].frames(), nframes=steps, **(dict(seq_lengths=[wave[0].nframes]) if seqm else {}))
            per_seq = [res]
        else:
            grp = NS.ReplicaGroup(ads, steps)
            if seqm:
                for a, s in zip(ads, wave):
                    a._seq_lengths, a._seq_names = None, [s.name]
            its = [iter(s.frames()) for s in wave]
            try:
                for step in range(steps):
                    batches = []
                    for it in its:
                        b = next(it, None)
                        if b is not None:
                            dev = ads[0].device
                            b = {k: v.to(dev) if isinstance(v, torch.Tensor) else v for k, v in b.items()}
                            if seqm:
                                ads[len(batches)].note_frame_names(b)
                        batches.append(b)
                    grp.step(batches, step, result_steps=[s.first + step * B for s in wave] if number else None)
            finally:
                close_overlays(ads)                        # a sequence's video stays open across the wave's steps and ends with it
            per_seq = grp.flush_metrics()
        for s, res in zip(wave, per_seq):
            mp = np.concatenate([np.ravel(np.asarray(x, np.float64)) for x in res["mpjpe"]]) if len(res["mpjpe"]) else np.zeros(0)
            pa = np.concatenate([np.ravel(np.asarray(x, np.float64)) for x in res["pampjpe"]]) if len(res["pampjpe"]) else np.zeros(0)
            pve_b = np.ravel(np.asarray(res["pve"], np.float64))                      # one value per batch (mean over it)
            if mp.shape[0] != s.nframes:             # a missing frame record must not be papered over
                raise RuntimeError(f"sequence {s.name}: {mp.shape[0]} frame records for {s.nframes} frames")
            n = s.nframes
            pve = np.repeat(pve_b, B)[:n] if pve_b.size else np.zeros(n)
            gi = np.arange(s.first, s.first + n, dtype=np.float64)
            cols = [gi, mp[:n], pa[:n], pve]
            if seqm:
                if len(res["pck"]) != n:
                    raise RuntimeError(f"sequence {s.name}: {len(res['pck'])} sequence-metric rows for {n} frames")
                cols += [np.asarray(res[k], np.float64) for k in ("accel", "accel_counted", "pck", "auc")]
            rows.append(np.stack(cols, 1))
        del ads
    local = np.concatenate(rows, 0) if rows else np.zeros((0, W))
    dev = torch.device("cuda", torch.cuda.current_device()) if (torch.cuda.is_available() and torch.distributed.is_available()
                                                                  and torch.distributed.is_initialized()
                                                                  and torch.distributed.get_backend(group) == "nccl") else torch.device("cpu")
    allr = gather_frame_metrics(torch.from_numpy(local).to(dev).flatten(), group).cpu().numpy().reshape(-1, W)
    allr = allr[np.argsort(allr[:, 0], kind="stable")]
    out = dict(global_index=allr[:, 0].astype(np.int64), mpjpe=allr[:, 1], pampjpe=allr[:, 2], pve=allr[:, 3], owned=owned,
               frames_local=int(local.shape[0]))
    if seqm:
        out.update(accel=allr[:, 4], accel_counted=allr[:, 5] > 0.5, pck=allr[:, 6], auc=allr[:, 7],
                   per_sequence=per_sequence_from_rows(sequences, allr))
        if shard_rank == 0:
            from .benchmark import write_sequence_report
            write_sequence_report(os.path.join(getattr(options, "expdir", "exps"), getattr(options, "expname", "run")), options, out)
    return out


def per_sequence_from_rows(sequences: Sequence[SequenceSpec], allr: np.ndarray) -> List[dict]:
    """The report's per-sequence dicts from the gathered 8-wide frame rows (global index, mpjpe, pampjpe, pve, accel,
    accel_counted, pck, auc): means in double over the sequence's frames, the acceleration error over its counted triples."""
    out = []
    gi = allr[:, 0]
    mean = lambda v: float(np.mean(v)) if len(v) else 0.0
    for s in sequences:
        r = allr[(gi >= s.first) & (gi < s.first + s.nframes)]
        c = r[:, 5] > 0.5
        out.append(dict(name=str(s.name), frames=int(r.shape[0]), mpjpe=mean(r[:, 1]), pampjpe=mean(r[:, 2]), pck=mean(r[:, 6]),
                        auc=mean(r[:, 7]), accel=mean(r[c, 4]), triples=int(c.sum())))
    return out


def main(options):
    """`python -m dynaboa_amd.benchmark --num_shards N [--shard_rank r] [--seqs_per_gpu S]`; under torchrun the rank / world size come
    from the environment (RANK, WORLD_SIZE, LOCAL_RANK) and the final gather runs over RCCL."""
    import torch.distributed as dist
    from . import benchmark as DB
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if world > 1 and not dist.is_initialized():
        torch.cuda.set_device(int(os.environ.get("LOCAL_RANK", "0")))
        dist.init_process_group("nccl")
    rank = int(os.environ.get("RANK", options.shard_rank))
    nsh = world if world > 1 else int(options.num_shards)
    dev = torch.device("cuda", torch.cuda.current_device())
    seqs = pw3d_sequences(options, dev)
    if int(options.seqs_per_gpu) > 1:
        # several sequences per launch: the throughput policy unless bit-identity with sequences adapted alone is asked for
        from . import native_step as NS
        NS.set_replica_policy(getattr(options, "replica_policy", "throughput") != "bitexact")
    res = run_sharded(options, seqs, lambda: DB.Adaptor(options, device=dev), nsh, rank, int(options.seqs_per_gpu))
    if rank == 0:
        print(f"frames:{len(res['mpjpe'])} MPJPE:{np.mean(res['mpjpe'])}, PAMPJPE:{np.mean(res['pampjpe'])}, PVE:{np.mean(res['pve'])}")
        if getattr(options, "seq_metrics", 0):
            print(DB.sequence_line(res))
    return res
