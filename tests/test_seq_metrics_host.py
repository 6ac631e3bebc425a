"""--seq_metrics: the host side.  flush_metrics_of, run_sharded, the report files and the flag handling on the emulator library with
CPU tensors (the `emu_lib` pattern of tests/test_host_emu.py); marked gpu, Adaptor.excute end to end on cuda:0 on the native stepper
and on the autograd path, and run_sharded with two sequences per launch against one."""
import ctypes
import csv
import json
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from dynaboa_amd import pose_utils as PU


@pytest.fixture
def emu_lib():
    """The emulator library as dynaboa_amd's library for ONE test (the build is cached): the tests marked gpu further down run in the
    same module and must find the real library again."""
    from emu.build_emu import build
    from dynaboa_amd import _abi, _lib
    lib = _abi.bind(ctypes.CDLL(build()))
    saved = _lib._lib
    _lib.use_library(lib)
    yield lib
    _lib._lib = saved


OLD_KEYS = {"mpjpe", "pampjpe", "pve", "records"}
NEW_KEYS = {"accel", "accel_counted", "pck", "auc", "per_sequence"}


def _joints(rng, B, sigma):
    gt = rng.normal(0, 0.3, (B, 14, 3)).astype(np.float32)
    return torch.from_numpy((gt + rng.normal(0, sigma, gt.shape)).astype(np.float32)), torch.from_numpy(gt)


def _record(rng, step, tag, B, sigma):
    pred, gt = _joints(rng, B, sigma)
    return dict(step=step, tag=tag, pred=pred, gt=gt, mpjpe=(pred - gt).norm(dim=-1).mean(dim=-1), pve=torch.tensor(float(rng.random())))


class _Stub:
    """What flush_metrics_of reads of an adaptor: deferred records, no stepper, no side stream."""

    def __init__(self, seq_metrics, pending, expname="stub", **attrs):
        self._native, self._side, self._pending = None, None, list(pending)
        self.options = SimpleNamespace(seq_metrics=seq_metrics, expname=expname)
        for k, v in attrs.items():
            setattr(self, k, v)


def _three_adaptors(seq_metrics, B):
    """-> (stubs, per stub the indices of the records a frame's result comes from), every record a batch of B (one flush stacks the
    records of all its adaptors).  Stub 0: five steps with lower-level records in between and step 2's final repeated twice (the
    dynamic loop: the last counts); stub 1: three steps, two lower-level records each; stub 2: two steps (no triple at B = 1), an
    untagged record in between."""
    rng = np.random.default_rng(190)
    a, sel_a = [], []
    for step in range(5):
        a.append(_record(rng, step, ('lower', 0), B, 0.05))
        for k in range(3 if step == 2 else 1):
            a.append(_record(rng, step, ('final', k), B, 0.02 + 0.01 * step))
        sel_a.append(len(a) - 1)
    b, sel_b = [], []
    for step in range(3):
        b.append(_record(rng, step, ('lower', 0), B, 0.2))
        b.append(_record(rng, step, ('lower', 1), B, 0.2))
        b.append(_record(rng, step, ('final', 0), B, 0.1))
        sel_b.append(len(b) - 1)
    c = [_record(rng, 0, ('final', 0), B, 0.01), _record(rng, 0, None, B, 0.5), _record(rng, 1, ('final', 0), B, 0.01)]
    return [_Stub(seq_metrics, a), _Stub(seq_metrics, b), _Stub(seq_metrics, c)], [sel_a, sel_b, [0, 2]]


def _expected(rec, sel):
    """The NumPy functions on the selected records, step-major and then batch."""
    p = torch.cat([rec[i]['pred'] for i in sel]).numpy().astype(np.float64)
    g = torch.cat([rec[i]['gt'] for i in sel]).numpy().astype(np.float64)
    n = len(p)
    accel, counted = np.zeros(n), np.zeros(n, bool)
    if n >= 3:
        accel[1:-1], counted[1:-1] = PU.compute_error_accel(g, p) * 1000, True
    auc = np.mean([PU.compute_pck(p, g, t) for t in PU.AUC_THRESHOLDS], 0)
    return dict(accel=accel, accel_counted=counted, pck=PU.compute_pck(p, g, 0.15), auc=auc,
                mpjpe=np.linalg.norm(p - g, axis=-1).mean(-1) * 1000, pampjpe=PU.reconstruction_error(p, g, reduction=None) * 1000)


def test_parser_default_is_off_and_internet_refuses_the_flag():
    from dynaboa_amd import benchmark as DB, internet as I
    assert DB.parser.parse_args([]).seq_metrics == 0 and DB.frame_only_options().seq_metrics == 0
    assert I.parser.parse_args([]).seq_metrics == 0
    with pytest.raises(ValueError, match="ground truth"):
        I.run_driver(I.parser.parse_args(["--seq_metrics", "1"]))
    with pytest.raises(ValueError, match="ground truth"):
        I.Adaptor(I.parser.parse_args(["--seq_metrics", "1"]))


@pytest.mark.parametrize("B", [1, 2])
def test_flush_off_has_exactly_todays_keys(emu_lib, B):
    from dynaboa_amd import benchmark as DB
    stubs, sel = _three_adaptors(0, B)
    recs = [list(s._pending) for s in stubs]
    outs = DB.flush_metrics_of(stubs)
    assert all(set(o) == OLD_KEYS for o in outs)
    for o, rec, s in zip(outs, recs, sel):
        assert len(o["records"]) == len(rec) and len(o["mpjpe"]) == len(s)
        for k, i in enumerate(s):                                             # the last final record of every step
            assert np.array_equal(o["mpjpe"][k], o["records"][i]["mpjpe"]) and o["pve"][k] == o["records"][i]["pve"]
    assert [s._pending for s in stubs] == [[], [], []]


@pytest.mark.parametrize("B", [1, 2])
def test_flush_on_adds_the_sequence_metrics_and_leaves_the_old_keys(emu_lib, B):
    from dynaboa_amd import benchmark as DB
    off_stubs, sel = _three_adaptors(0, B)
    on_stubs, _ = _three_adaptors(1, B)
    recs = [list(s._pending) for s in on_stubs]
    off, on = DB.flush_metrics_of(off_stubs), DB.flush_metrics_of(on_stubs)
    tight = lambda a, b: np.all(np.abs(np.asarray(a, np.float64) - b) <= 1e-4 + 3 * 2.0 ** -24 * np.abs(b))      # mm
    for k, (o0, o1, rec, s) in enumerate(zip(off, on, recs, sel)):
        assert set(o1) == OLD_KEYS | NEW_KEYS
        for key in ("mpjpe", "pampjpe"):                                      # the old keys: what the flag-off call returns, bit for bit
            assert len(o0[key]) == len(o1[key]) and all(np.array_equal(x, y) for x, y in zip(o0[key], o1[key]))
        assert o0["pve"] == o1["pve"] and len(o0["records"]) == len(o1["records"])
        for r0, r1 in zip(o0["records"], o1["records"]):
            assert r0["step"] == r1["step"] and r0["tag"] == r1["tag"] and r0["pve"] == r1["pve"]
            assert np.array_equal(r0["mpjpe"], r1["mpjpe"]) and np.array_equal(r0["pampjpe"], r1["pampjpe"])
        e = _expected(rec, s)
        assert o1["accel_counted"].dtype == bool and np.array_equal(o1["accel_counted"], e["accel_counted"])
        assert tight(o1["accel"], e["accel"]) and (o1["accel"][~e["accel_counted"]] == 0).all()
        assert np.abs(o1["pck"] - e["pck"]).max() <= 1e-6 and np.abs(o1["auc"] - e["auc"]).max() <= 1e-6
        (row,) = o1["per_sequence"]                                           # one sequence per adaptor by default
        assert set(row) == {"name", "frames", "mpjpe", "pampjpe", "pck", "auc", "accel", "triples"}
        assert row["frames"] == len(e["pck"]) and row["triples"] == int(e["accel_counted"].sum()) and row["name"] == f"stub_{k}_0"
        assert tight(row["mpjpe"], e["mpjpe"].mean()) and abs(row["pampjpe"] - e["pampjpe"].mean()) <= 2e-2 + 1e-4 * e["pampjpe"].max()
        assert abs(row["pck"] - e["pck"].mean()) <= 1e-6 and abs(row["auc"] - e["auc"].mean()) <= 1e-6
        assert tight(row["accel"], e["accel"][e["accel_counted"]].mean() if row["triples"] else 0.0)
    assert [r["triples"] for o in on for r in o["per_sequence"]] == [5 * B - 2, 3 * B - 2, 2 * B - 2]


def test_flush_splits_an_adaptor_into_its_sequences_and_reads_frame_ids(emu_lib):
    """`_seq_lengths` cuts one adaptor's frames into sequences (no triple crosses the cut); frame ids parsed from imgname drop the
    triples that straddle a gap; one name that does not parse and the ids are left out."""
    from dynaboa_amd import benchmark as DB
    rng = np.random.default_rng(191)
    recs = [_record(rng, s, ('final', 0), 1, 0.03) for s in range(9)]
    names = [f"imageFiles/courtyard_00/image_{i:05d}.jpg" for i in (0, 1, 2, 3, 10, 11, 12, 13, 14)]
    out = DB.flush_metrics_of([_Stub(1, recs, _seq_lengths=[4, 5], _seq_names=["a", "b"], _frame_names=names)])[0]
    assert out["accel_counted"].tolist() == [False, True, True, False, False, True, True, True, False]
    assert [(r["name"], r["frames"], r["triples"]) for r in out["per_sequence"]] == [("a", 4, 2), ("b", 5, 3)]
    out = DB.flush_metrics_of([_Stub(1, recs, _frame_names=names)])[0]         # one sequence: the gap 3 -> 10 takes two triples
    assert out["accel_counted"].tolist() == [False, True, True, False, False, True, True, True, False]
    out = DB.flush_metrics_of([_Stub(1, recs, _frame_names=names[:-1] + ["last.jpg"])])[0]
    assert out["accel_counted"].tolist() == [False] + [True] * 7 + [False]
    with pytest.raises(RuntimeError, match="sequence lengths"):
        DB.flush_metrics_of([_Stub(1, recs, _seq_lengths=[4, 4])])


class _ShardStub(_Stub):
    """An adaptor for run_sharded: excute() 'adapts' by recording the joints its frames carry and flushing them."""

    def __init__(self, expdir):
        super().__init__(1, [])
        self.options = SimpleNamespace(seq_metrics=1, deferred_metrics=1, batch_size=1, expdir=str(expdir), expname="run")
        self.device = torch.device("cpu")

    def excute(self, frames, nframes=None, seq_lengths=None):
        from dynaboa_amd import benchmark as DB
        self._seq_lengths, self._seq_names = seq_lengths, getattr(self, "seq_names", None)
        self._pending = [dict(step=k, tag=('final', 0), **b) for k, b in enumerate(frames)]
        return DB.flush_metrics_of([self])[0]


def test_run_sharded_reports_per_sequence_and_writes_the_files(emu_lib, tmp_path):
    from dynaboa_amd.sharded import SequenceSpec, run_sharded
    rng = np.random.default_rng(192)
    lens, sigma = [5, 2, 7, 1, 3], [0.02, 0.3, 0.05, 0.01, 0.1]
    data, specs, first = [], [], 0
    for k, n in enumerate(lens):
        frames = []
        for _ in range(n):
            r = _record(rng, 0, None, 1, sigma[k])
            frames.append({q: r[q] for q in ("pred", "gt", "mpjpe", "pve")})
        data.append(frames)
        specs.append(SequenceSpec(f"seq{k}", first, n, (lambda frames=frames: frames)))
        first += n
    o = SimpleNamespace(batch_size=1, seq_metrics=1, expdir=str(tmp_path), expname="run")
    res = run_sharded(o, specs, lambda: _ShardStub(tmp_path))
    n = sum(lens)
    assert res["global_index"].tolist() == list(range(n)) and all(len(res[k]) == n for k in ("mpjpe", "pampjpe", "pve", "accel", "pck", "auc"))
    assert res["accel_counted"].dtype == bool and int(res["accel_counted"].sum()) == 3 + 0 + 5 + 0 + 1
    assert [r["name"] for r in res["per_sequence"]] == [f"seq{k}" for k in range(5)]
    first = 0
    for k, (ln, row) in enumerate(zip(lens, res["per_sequence"])):
        p = torch.cat([f["pred"] for f in data[k]]).numpy().astype(np.float64)
        g = torch.cat([f["gt"] for f in data[k]]).numpy().astype(np.float64)
        assert row["frames"] == ln and row["triples"] == max(ln - 2, 0)
        assert row["mpjpe"] == pytest.approx(np.linalg.norm(p - g, axis=-1).mean() * 1000, rel=1e-6)
        assert row["pampjpe"] == pytest.approx(PU.reconstruction_error(p, g) * 1000, rel=1e-4, abs=2e-2)
        assert row["pck"] == pytest.approx(PU.compute_pck(p, g, 0.15).mean(), abs=1e-6)
        assert row["accel"] == pytest.approx(PU.compute_error_accel(g, p).mean() * 1000 if ln >= 3 else 0.0, rel=1e-6)
        assert np.array_equal(res["accel_counted"][first:first + ln], [0 < i < ln - 1 for i in range(ln)])      # none crosses a sequence
        first += ln
    # the files: at the top of the experiment folder; the CSV worst PA-MPJPE first
    m = json.load(open(tmp_path / "run" / "metrics.json"))
    assert m["sequences"] == 5 and m["flags"]["seq_metrics"] == 1 and m["overall"]["frames"] == n and m["overall"]["triples"] == 9
    assert m["overall"]["mpjpe"] == pytest.approx(res["mpjpe"].mean()) and m["overall"]["pck"] == pytest.approx(res["pck"].mean())
    assert m["overall"]["accel"] == pytest.approx(res["accel"][res["accel_counted"]].mean())
    assert m["sequence_mean"]["pampjpe"] == pytest.approx(np.mean([r["pampjpe"] for r in res["per_sequence"]]))
    assert m["sequence_mean"]["accel"] == pytest.approx(np.mean([r["accel"] for r in res["per_sequence"] if r["triples"]]))
    rows = list(csv.DictReader(open(tmp_path / "run" / "metrics_per_sequence.csv")))
    assert sorted(r["name"] for r in rows) == [f"seq{k}" for k in range(5)]
    pa = [float(r["pampjpe"]) for r in rows]
    assert pa == sorted(pa, reverse=True) and rows[0]["name"] == "seq1"
    assert sorted(os.listdir(tmp_path / "run")) == ["metrics.json", "metrics_per_sequence.csv"]
    # flag off: the 4-wide row and today's keys
    o.seq_metrics = 0

    def plain():
        s = _ShardStub(tmp_path)
        s.options.seq_metrics = 0
        return s
    res0 = run_sharded(o, specs, plain)
    assert set(res0) == {"global_index", "mpjpe", "pampjpe", "pve", "owned", "frames_local"}
    assert np.array_equal(res0["mpjpe"], res["mpjpe"]) and np.array_equal(res0["pampjpe"], res["pampjpe"])


def test_sequence_metrics_device_wrapper(emu_lib):
    """Tensors in, tensors out, the column names exported; lengths that do not tile the frames are refused."""
    rng = np.random.default_rng(193)
    pred, gt = _joints(rng, 7, 0.05)
    frame, seq = PU.sequence_metrics_device(pred, gt, [3, 0, 4], valid=torch.tensor([1, 1, 1, 1, 1, 0, 1], dtype=torch.bool))
    assert tuple(frame.shape) == (7, PU.FRAME_FLOATS) and tuple(seq.shape) == (4, PU.SEQ_FLOATS)
    assert frame[:, PU.FRAME_ACCEL_COUNTED].tolist() == [0, 1, 0, 0, 0, 0, 0]
    assert seq[:, PU.SEQ_FRAMES].tolist() == [3, 0, 4, 7] and seq[:, PU.SEQ_TRIPLES].tolist() == [1, 0, 0, 1]
    e = PU.compute_error_accel(gt[:3].numpy().astype(np.float64), pred[:3].numpy().astype(np.float64))
    assert float(seq[0, PU.SEQ_ACCEL]) == pytest.approx(e[0], rel=1e-6)
    with pytest.raises(ValueError):
        PU.sequence_metrics_device(pred, gt, [3, 3])


# ------------------------------------------------------------------------------------------------ on the device
FRAME_ONLY = dict(retrieval=0, lower_level_mixtrain=0, upper_level_mixtrain=0, use_meanteacher=0, use_motion=0,
                  dynamic_boa=0, use_temporal_losses_upper=0, inner_step=1)


def _excute(expdir, nframes=4, **over):
    from dynaboa_amd import _lib, assets, benchmark as DB
    from dynaboa_amd.base_adaptor import synthetic_bundle
    assert _lib.load()._name == _lib.LIB_PATH                  # the device library, not a host build an earlier test installed
    o = DB.parser.parse_args([])
    for k, v in {**FRAME_ONLY, "deferred_metrics": 1, "expdir": str(expdir), "expname": "seqm", **over}.items():
        setattr(o, k, v)
    ad = DB.Adaptor(o, synthetic_bundle(seed=22, identity_pose=False, randomize_norm=True, smpl_seed=0), device="cuda:0")
    res = ad.excute([assets.make_frame(step, 1, seed=22) for step in range(nframes)], nframes=nframes)
    return ad, res


@pytest.mark.gpu
@pytest.mark.parametrize("native_step", [1, 0])
def test_excute_with_seq_metrics_on_the_device(tmp_path, native_step):
    """Adaptor.excute on 4 synthetic frames with --seq_metrics 1, on the native stepper and on the autograd path: mpjpe / pampjpe /
    pve equal the flag-off run exactly, accel has 2 counted triples and equals the NumPy function on the records' joints,
    metrics.json exists."""
    ad0, off = _excute(tmp_path / "off", native_step=native_step, seq_metrics=0)
    spy = {}
    from dynaboa_amd import benchmark as DB
    inner = DB._sequence_metrics_of

    def keep(adaptors, recs):
        spy["pred"] = torch.cat([r["pred"] for r in recs[0] if r["tag"][0] == "final"]).cpu().numpy().astype(np.float64)
        spy["gt"] = torch.cat([r["gt"] for r in recs[0] if r["tag"][0] == "final"]).cpu().numpy().astype(np.float64)
        return inner(adaptors, recs)
    DB._sequence_metrics_of = keep
    try:
        ad1, on = _excute(tmp_path / "on", native_step=native_step, seq_metrics=1, deferred_metrics=0)      # (forced back to 1)
    finally:
        DB._sequence_metrics_of = inner
    assert (ad1._native is not None) == bool(native_step) == (ad0._native is not None) and ad1.options.deferred_metrics == 1
    assert set(off) == {"mpjpe", "pampjpe", "pve"} and set(on) == set(off) | NEW_KEYS
    for k in ("mpjpe", "pampjpe"):
        assert len(on[k]) == 4 and all(np.array_equal(a, b) for a, b in zip(on[k], off[k]))
    assert on["pve"] == off["pve"]
    assert on["accel_counted"].tolist() == [False, True, True, False] and (on["accel"][[0, 3]] == 0).all()
    e = PU.compute_error_accel(spy["gt"], spy["pred"]) * 1000
    assert np.abs(on["accel"][1:3] - e).max() <= 1e-4 + 3 * 2.0 ** -24 * e.max()
    assert np.abs(on["pck"] - PU.compute_pck(spy["pred"], spy["gt"], 0.15)).max() <= 1e-6
    (row,) = on["per_sequence"]
    assert row["frames"] == 4 and row["triples"] == 2 and row["name"] == "seqm"
    assert row["pampjpe"] == pytest.approx(np.mean(np.concatenate(on["pampjpe"])), rel=1e-5)
    m = json.load(open(tmp_path / "on" / "seqm" / "metrics.json"))
    assert m["overall"]["triples"] == 2 and m["overall"]["accel"] == pytest.approx(float(on["accel"][1:3].mean()))
    assert os.path.exists(tmp_path / "on" / "seqm" / "metrics_per_sequence.csv")
    assert not os.path.exists(tmp_path / "off" / "seqm" / "metrics.json")


@pytest.mark.gpu
def test_run_sharded_with_seq_metrics_in_a_replica_group_on_the_device(tmp_path):
    """run_sharded over three synthetic sequences of 4, 3 and 2 frames: two at a time in a ReplicaGroup (one flush, one
    dyb_seq_metrics call over both adaptors) against one at a time - the same per-frame columns and per-sequence rows, no triple
    across two sequences, one report for the whole run."""
    from dynaboa_amd import _lib, assets, benchmark as DB
    from dynaboa_amd.base_adaptor import synthetic_bundle
    from dynaboa_amd.sharded import SequenceSpec, run_sharded
    assert _lib.load()._name == _lib.LIB_PATH
    lens = [4, 3, 2]
    frames = [[{k: v.to("cuda:0") for k, v in assets.make_frame(100 * r + s, 1, seed=22).items()} for s in range(n)] for r, n in enumerate(lens)]
    specs, first = [], 0
    for k, n in enumerate(lens):
        specs.append(SequenceSpec(f"s{k}", first, n, (lambda k=k: frames[k])))
        first += n
    out = {}
    for S in (1, 2):
        o = DB.frame_only_options(inner_step=1, seq_metrics=1, expdir=str(tmp_path), expname=f"S{S}")
        out[S] = run_sharded(o, specs, lambda: DB.Adaptor(o, synthetic_bundle(seed=22, identity_pose=False, randomize_norm=True, smpl_seed=0),
                                                          device="cuda:0"), seqs_per_gpu=S)
        assert sorted(os.listdir(tmp_path / f"S{S}")) == ["metrics.json", "metrics_per_sequence.csv"]
    one, two = out[1], out[2]
    assert two["accel_counted"].tolist() == [False, True, True, False, False, True, False, False, False] == one["accel_counted"].tolist()
    assert [(r["name"], r["frames"], r["triples"]) for r in two["per_sequence"]] == [("s0", 4, 2), ("s1", 3, 1), ("s2", 2, 0)]
    for k in ("mpjpe", "pampjpe", "accel", "pck", "auc"):
        np.testing.assert_allclose(two[k], one[k], rtol=2e-5, atol=1e-6)
    for a, b in zip(one["per_sequence"], two["per_sequence"]):
        for k in ("mpjpe", "pampjpe", "pck", "auc", "accel"):
            assert a[k] == pytest.approx(b[k], rel=2e-5, abs=1e-6)
    assert json.load(open(tmp_path / "S2" / "metrics.json"))["overall"]["triples"] == 3
