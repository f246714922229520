#!/usr/bin/env python
"""Time of the neural acoustic models' scoring launch (launch_gmm's MLP branch: jd_mlp_kernel) against the same forward pass in
torch f32 on the same device (GPU box):  python tools/mlp_bench.py [--iters N] [--warmup W] [--json]
8192 rows (a batch's table) and 64 rows (a streaming push) of 351 -> 512 -> 512 -> 45, sigmoid.  Device events around each launch
(jd_debug_mlp_time), the median of `iters` warm launches; torch: events around linear / sigmoid / log_softmax, the same median.
FLOP = 2 x rows x weights (the products' multiply-adds; activations and the log-softmax are not counted)."""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
from juicer_amd import capi  # noqa: E402

IN_DIM, WIDTHS = 351, (512, 512, 45)


def make(seed=0):
    rng = np.random.default_rng(seed)
    layers, k = [], IN_DIM
    for i, n in enumerate(WIDTHS):
        layers.append(((rng.standard_normal((n, k)) / np.sqrt(k)).astype(np.float32), (rng.standard_normal(n) * 0.1).astype(np.float32),
                       capi.ACT_SIGMOID if i < len(WIDTHS) - 1 else capi.ACT_LINEAR))
        k = n
    pr = rng.uniform(0.5, 2.0, WIDTHS[-1])
    return layers, (pr / pr.sum()).astype(np.float32)


def torch_ms(layers, log_prior, x, warmup, iters):
    dev = torch.device("cuda")
    ws = [(torch.from_numpy(w).to(dev), torch.from_numpy(b).to(dev)) for w, b, _ in layers]
    lp = torch.from_numpy(log_prior).to(dev)
    xd = torch.from_numpy(x).to(dev)

    def fwd():
        a = xd
        for i, (w, b) in enumerate(ws):
            a = torch.nn.functional.linear(a, w, b)
            if i < len(ws) - 1:
                a = torch.sigmoid(a)
        return torch.log_softmax(a, dim=1) - lp

    ms = []
    with torch.no_grad():
        for i in range(warmup + iters):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            out = fwd()
            e1.record()
            e1.synchronize()
            if i >= warmup:
                ms.append(e0.elapsed_time(e1))
    return float(np.median(ms)), out.cpu().numpy()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--json", action="store_true")
    args = ap.parse_args()
    assert args.iters >= 20, "the median of at least 20 warm launches"
    if not torch.cuda.is_available():
        sys.exit("mlp_bench: no GPU (a time is a measurement on the device)")
    torch.backends.cuda.matmul.allow_tf32 = False
    layers, pr = make()
    models = capi.Models.from_mlp(pr, 3, layers)
    weights = sum(w.size for w, _, _ in layers)
    res = []
    for rows in (8192, 64):
        x = np.random.default_rng(rows).standard_normal((rows, IN_DIM)).astype(np.float32)
        ms = float(np.median(models.mlp_time(x, warmup=args.warmup, iters=args.iters)))
        t_ms, t_out = torch_ms(layers, np.log(pr), x, args.warmup, args.iters)
        ours = models.score_frames(x)
        flop = 2.0 * rows * weights
        res.append(dict(rows=rows, ms=ms, tflops=flop / ms / 1e9, torch_ms=t_ms, torch_tflops=flop / t_ms / 1e9, ratio=ms / t_ms,
                        max_abs_diff_vs_torch=float(np.abs(ours - t_out).max())))
    if args.json:
        print(json.dumps(res))
    else:
        for r in res:
            print("%5d rows: jd_mlp_kernel %.4f ms (%.2f TFLOP/s)   torch f32 %.4f ms (%.2f TFLOP/s)   ratio %.2f   max |diff| %.2e"
                  % (r["rows"], r["ms"], r["tflops"], r["torch_ms"], r["torch_tflops"], r["ratio"], r["max_abs_diff_vs_torch"]))


if __name__ == "__main__":
    main()
