#!/usr/bin/env python3
"""Where the weight gradients of one steady-state frame step run, from a rocprofv3 kernel trace of bench.py (python
tools/defer_window.py <kernel_trace.csv> <out.txt>): the step is the window between two Adam bursts (as tools/frame_timeline.py); on the
main queue every backward phase (first GroupNorm-backward kernel .. last data gradient before the next forward convolution) and
every forward phase (first .. last forward convolution of a pass) are located; reported are the backward and forward spans, the
in-path time of the GroupNorm-backward and data-gradient families, the auxiliary queue's busy / idle time, and how many
weight-gradient / regressor launches of the auxiliary queue START inside a forward phase ("wgrad_defer": the deferred set; the forward
waits for it before layer4, so what starts inside a forward phase runs beside stem .. layer3)."""
import csv
import sys
from collections import defaultdict


def main(path, out):
    rows = []
    with open(path) as f:
        for r in csv.DictReader(f):
            rows.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Kernel_Name"].replace("void ", ""), r.get("Queue_Id", "?")))
    rows.sort()
    ad_all = [i for i, r in enumerate(rows) if r[2].startswith(("adam_kernel", "adam_segs_kernel"))]
    ad = [i for n, i in enumerate(ad_all) if n == 0 or rows[i][0] - rows[ad_all[n - 1]][0] > 5_000_000]
    i0, i1 = ad[len(ad) // 2], ad[len(ad) // 2 + 1]
    seq = rows[i0:i1]
    t0 = seq[0][0]
    span = seq[-1][1] - t0
    byq = defaultdict(list)
    for r in seq:
        byq[r[3]].append(r)
    main_q = max(byq, key=lambda q: len(byq[q]))
    mq = byq[main_q]
    aux = [r for q, rs in byq.items() if q != main_q for r in rs]
    is_fwd = lambda k: k.startswith("igemm_tp_kernel<0")
    is_dgrad = lambda k: k.startswith("igemm_tp_kernel<1")
    is_gnb = lambda k: k.startswith("gn_bwd")
    is_wg = lambda k: k.startswith("igemm_tp_kernel<2") or k.startswith("linear_outer")
    # backward phases and forward phases of the main queue
    bwd, fwd, cur_b, cur_f = [], [], None, None
    for s, e, k, _ in mq:
        if is_gnb(k) or is_dgrad(k):
            if cur_b is None:
                cur_b = [s, e]
            cur_b[1] = e
            if cur_f is not None:
                fwd.append(cur_f)
                cur_f = None
        elif is_fwd(k):
            if cur_b is not None:
                bwd.append(cur_b)
                cur_b = None
            if cur_f is None:
                cur_f = [s, e]
            cur_f[1] = e
    if cur_b is not None:
        bwd.append(cur_b)
    if cur_f is not None:
        fwd.append(cur_f)
    L = [f"frame step: {len(seq)} kernels, span {span/1e3:.1f} us; main queue {main_q}: {len(mq)} kernels"]
    L.append("backward phases on the main queue (first GroupNorm-backward kernel .. last data gradient), us: " +
             ", ".join(f"{(b[1]-b[0])/1e3:.0f}" for b in bwd) + f"; sum {sum(b[1]-b[0] for b in bwd)/1e3:.0f}")
    L.append("forward phases on the main queue (first .. last forward convolution), us: " +
             ", ".join(f"{(b[1]-b[0])/1e3:.0f}" for b in fwd) + f"; sum {sum(b[1]-b[0] for b in fwd)/1e3:.0f}")
    gnb = sum(e - s for s, e, k, _ in mq if is_gnb(k))
    dg = sum(e - s for s, e, k, _ in mq if is_dgrad(k))
    fw = sum(e - s for s, e, k, _ in mq if is_fwd(k))
    L.append(f"in-path kernel time, main queue: GroupNorm backward {gnb/1e3:.0f} us, data gradients {dg/1e3:.0f} us, forward convolutions {fw/1e3:.0f} us")
    busy = sum(e - s for s, e, *_ in aux)
    wg = [r for r in aux if is_wg(r[2])]
    L.append(f"auxiliary queue(s): {len(aux)} kernels, busy {busy/1e3:.0f} us, idle {(span-busy)/1e3:.0f} us; weight-gradient + regressor "
             f"launches {len(wg)}, {sum(e-s for s,e,*_ in wg)/1e3:.0f} us")
    inside = [r for r in wg if any(f[0] <= r[0] <= f[1] for f in fwd)]
    inb = [r for r in wg if any(b[0] <= r[0] <= b[1] for b in bwd)]
    L.append(f"  starting inside a forward phase: {len(inside)} launches, {sum(e-s for s,e,*_ in inside)/1e3:.0f} us; inside a backward phase: "
             f"{len(inb)} launches, {sum(e-s for s,e,*_ in inb)/1e3:.0f} us; elsewhere: {len(wg)-len(inside)-len(inb)}")
    for n, f in enumerate(fwd):
        rs = [r for r in wg if f[0] <= r[0] <= f[1]]
        if rs:
            L.append(f"  forward {n} ({(f[0]-t0)/1e3:.0f} .. {(f[1]-t0)/1e3:.0f} us): {len(rs)} launches from {(rs[0][0]-t0)/1e3:.0f} to "
                     f"{(max(r[1] for r in rs)-t0)/1e3:.0f} us")
    open(out, "w").write("\n".join(L) + "\n")
    print("\n".join(L))


if __name__ == "__main__":
    main(sys.argv[1], sys.argv[2])
