"""What tests/test_group_side_emu.py and tests/test_group_side_gpu.py share: a replica group of the frame-loss stepper stepped through a
few frames with the stepper option "group_side" (adapt_step.hip) off or on, and everything it leaves behind as tensors to compare bit
for bit.  The group is driven through NativeStepper.adapt_frames directly - every frame step, then ONE join - so that with the option
on nothing but the stepper's own events orders a frame's final inference against the frames that follow it."""
import torch

INNER = 1          # one lower level + the outer level: the smallest schedule with fused fast-weight AND fused Adam epilogues


def make_group(S, nframes, side, device):
    from dynaboa_amd import benchmark as DB, native_step as NS
    from dynaboa_amd.base_adaptor import synthetic_bundle
    ads = []
    for r in range(S):
        o = DB.frame_only_options(inner_step=INNER)
        o.deferred_metrics = 1
        o.native_results, o.dump_predictions = 1, 1          # the result ring (the group is stepped below the code that writes the dumps)
        o.group_side = side
        ads.append(DB.Adaptor(o, synthetic_bundle(seed=22 + r, identity_pose=False, randomize_norm=True, smpl_seed=0), device=device))
    grp = NS.ReplicaGroup(ads, nframes)
    assert grp.stepper.S == S and grp.stepper.results is not None
    assert grp.stepper.group_side == side and grp.stepper.use_side == side
    return grp


def frames_for(S, nframes, device):
    from dynaboa_amd import assets
    return [[{k: v.to(device) for k, v in assets.make_frame(100 * r + s, 1, seed=22).items()} for s in range(nframes)] for r in range(S)]


def step_all(grp, frames, nframes, leave=None):
    """nframes frame steps, then one join.  leave = (step, replica): that sequence sits out from that step on."""
    ns, S = grp.stepper, grp.stepper.S
    for step in range(nframes):
        if leave is not None and step == leave[0]:
            ns.set_active([r for r in range(S) if r != leave[1]])
        ns.adapt_frames([frames[r][step] for r in range(S)])
    ns.join()


def collect(grp, sample=None):
    """theta / both Adam moments (whole, or at `sample` seeded indices), records, loss rows, result-ring rows and output(k, r)."""
    ns = grp.stepper
    if sample is not None:                                  # `sample` indices per sequence, seeded
        idx = torch.randint(0, ns.theta.shape[1], (int(sample),), generator=torch.Generator().manual_seed(1818)).to(ns.theta.device)
    cut = (lambda t: t.clone()) if sample is None else (lambda t: t[:, idx].clone())
    row = dict(theta=cut(ns.theta), exp_avg=cut(ns.m), exp_avg_sq=cut(ns.v), records=ns.records.clone(), loss_log=ns.loss_log.clone(),
               results=ns.results.clone())
    for which in range(4):
        for r in range(ns.S):
            row[f"output/{which}/{r}"] = ns.output(which, r).clone()
    return row


def assert_identical(a, b):
    assert a.keys() == b.keys()
    for k in a:
        assert torch.equal(a[k], b[k]), k
