#!/usr/bin/env python3
"""Full training step (graph-replayed DataParallelTrainer, one GPU) on the 14 x 14 stress grid (224 x 224 images: n = 196 objects,
padded to njp = 224 pair rows per (question, i) group on the chain path) at B = 32: ir-fp (question at g layer 2) in "auto" -- now the
f16s chain -- and in "fp32" (the per-layer kernels: what "auto" resolved to before the padded axis covered it), beside original-fp
in "auto" (the stress shape of bench.py).  The arms are ALTERNATED over `--repeats` rounds in one process, so drift of the box hits
all of them alike; per arm the median q/s and the spread (min .. max) over the rounds are printed, and one JSON line at the end.

    python tools/time_ir_padded.py [--steps 20] [--warmup 5] [--repeats 3]"""
import argparse
import json
import os
import sys

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

ARMS = [("ir-fp", "auto"), ("ir-fp", "fp32"), ("original-fp", "auto")]
HW, N = 224, 196


class Args:
    qdict_size, adict_size = 82, 28


def make_arm(pkg, dp, T, cfg, precision, B):
    from oracle import formula
    torch.manual_seed(0)
    m = pkg.RN(Args, dict(formula.HYP[cfg], precision=precision, dropout=0.0)).cuda()
    assert m.rl.resolved_precision(B, N, 26) == ("f16s" if precision == "auto" else precision)
    opt = torch.optim.Adam(m.parameters(), lr=1e-5)
    tr = dp.DataParallelTrainer(m, opt, clip_norm=50.0, use_graph=True)
    img, q, y = T.load_tensor_data(next(iter(T.SyntheticClevr(B, B, hw=HW, seed=7))), "cuda")
    return tr, (img, q, y)


def time_arm(tr, batch, steps, warmup):
    for _ in range(warmup):
        tr.step(*batch)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(steps):
        loss = tr.step(*batch)
    e1.record()
    torch.cuda.synchronize()
    assert torch.isfinite(loss).all()
    return e0.elapsed_time(e1) / steps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--batch", type=int, default=32)
    a = ap.parse_args()
    import relationnetworks_clevr_amd as pkg
    import relationnetworks_clevr_amd.train as T
    from relationnetworks_clevr_amd import dp
    pkg.rn_hip.load()
    torch.cuda.set_device(0)
    arms = {arm: make_arm(pkg, dp, T, arm[0], arm[1], a.batch) for arm in ARMS}
    ms = {arm: [] for arm in ARMS}
    for r in range(a.repeats):
        order = ARMS if r % 2 == 0 else ARMS[::-1]
        for arm in order:
            ms[arm].append(time_arm(*arms[arm], a.steps, a.warmup))
    out = {}
    for arm in ARMS:
        qps = np.array([a.batch * 1000.0 / t for t in ms[arm]])
        key = "%s_%s" % arm
        out[key] = dict(qps_median=float(np.median(qps)), qps_min=float(qps.min()), qps_max=float(qps.max()),
                        ms_median=float(np.median(ms[arm])), spread_pct=float(100.0 * (qps.max() - qps.min()) / np.median(qps)))
        print("%-18s %8.1f q/s  (%.1f .. %.1f, spread %.1f %%)  %.3f ms/step" % (key, out[key]["qps_median"], qps.min(), qps.max(),
                                                                               out[key]["spread_pct"], out[key]["ms_median"]))
    out["ir-fp_auto_over_fp32"] = out["ir-fp_auto"]["qps_median"] / out["ir-fp_fp32"]["qps_median"]
    out["ir-fp_over_original-fp"] = out["ir-fp_auto"]["qps_median"] / out["original-fp_auto"]["qps_median"]
    print(json.dumps(dict(batch=a.batch, n=N, steps=a.steps, warmup=a.warmup, repeats=a.repeats, arms=out)))


if __name__ == "__main__":
    main()
