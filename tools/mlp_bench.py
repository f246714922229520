#!/usr/bin/env python
"""Time of the neural acoustic models' scoring launch (launch_gmm's MLP branch: jd_mlp_kernel) against the same forward pass in
torch f32 on the same device (GPU box):  python tools/mlp_bench.py [--tied] [--bf16 [--runs R]] [--iters N] [--warmup W] [--json]
8192 rows (a batch's table) and 64 rows (a streaming push) of 351 -> 512 -> 512 -> 45, sigmoid; with --tied, of the tied-state
networks 351 -> 1024 -> 1024 -> 3000 and 351 -> 1024 -> 1024 -> 8192, sigmoid (jd_am_create_mlp_tied: jd_mlp_tied_kernel).  Device events around each launch
(jd_debug_mlp_time), the median of `iters` warm launches; torch: events around linear / sigmoid / log_softmax, the same median.
FLOP = 2 x rows x weights (the products' multiply-adds; activations and the log-softmax are not counted).
--bf16: beside them the bf16 model of the same network (jd_am_mlp_to_bf16: jd_mlp_bf16_kernel / jd_mlp_tied_bf16_kernel) and torch in
bf16 - the f32 and the bf16 kernel alternate, R runs each (at least 3); the median over the runs' medians, and their spread
(least .. greatest), are reported.
--splice [--runs R] [--lib PATH]: the 39 x 9 network as it is on caller-spliced vectors of 351 values, and its model spliced (4, 4)
(jd_am_mlp_splice: the window is gathered in the kernel's input stage) on the same frames as raw vectors of 39 values - one utterance -
alternating, R runs each; the median of the runs' medians, the spread, and the bytes each variant copies to the device for the rows.
--lib: another build of libjuicer_amd.so, the parent commit's for instance - one that knows no splicing reports the unspliced figures
alone, which is what this commit's unspliced figures are held against."""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
from juicer_amd import capi  # noqa: E402

IN_DIM, WIDTHS = 351, (512, 512, 45)


TIED_WIDTHS = ((1024, 1024, 3000), (1024, 1024, 8192))          # 3000: the tied states of BASELINE configs[1]


def make(seed=0, widths=WIDTHS):
    rng = np.random.default_rng(seed)
    layers, k = [], IN_DIM
    for i, n in enumerate(widths):
        layers.append(((rng.standard_normal((n, k)) / np.sqrt(k)).astype(np.float32), (rng.standard_normal(n) * 0.1).astype(np.float32),
                       capi.ACT_SIGMOID if i < len(widths) - 1 else capi.ACT_LINEAR))
        k = n
    pr = rng.uniform(0.5, 2.0, widths[-1])
    return layers, (pr / pr.sum()).astype(np.float32)


def flat_topology(n_gmm):
    """GMM models of n_gmm tied states, one 3-state HMM each: the least topology that carries n_gmm outputs"""
    from juicer_amd import synth
    hg = np.full((n_gmm, 3), -1, np.int32)
    hg[:, 1] = np.arange(n_gmm)
    tp = np.zeros((1, 3, 3), np.float32)
    tp[0, 0, 1], tp[0, 1, 1], tp[0, 1, 2] = 1.0, 0.5, 0.5
    am = synth.SynthAM(D=1, n_gmm=n_gmm, max_mix=1, n_mix=np.ones(n_gmm, np.int32), weight=np.ones((n_gmm, 1), np.float32),
                       mean=np.zeros((n_gmm, 1, 1), np.float32), var=np.ones((n_gmm, 1, 1), np.float32), n_hmm=n_gmm, max_n=3,
                       hmm_nstates=np.full(n_gmm, 3, np.int32), hmm_gmm=hg, hmm_tm=np.zeros(n_gmm, np.int32), n_tm=1,
                       tm_nstates=np.full(1, 3, np.int32), transp=tp)
    return capi.Models.from_htk(am)


def flop_of(rows, weights):
    return 2.0 * rows * weights


def torch_ms(layers, log_prior, x, warmup, iters, dtype=torch.float32):
    dev = torch.device("cuda")
    ws = [(torch.from_numpy(w).to(dev).to(dtype), torch.from_numpy(b).to(dev).to(dtype)) for w, b, _ in layers]
    lp = torch.from_numpy(log_prior).to(dev)
    xd = torch.from_numpy(x).to(dev).to(dtype)

    def fwd():
        a = xd
        for i, (w, b) in enumerate(ws):
            a = torch.nn.functional.linear(a, w, b)
            if i < len(ws) - 1:
                a = torch.sigmoid(a)
        return torch.log_softmax(a.float(), dim=1) - lp

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


def splice_bench(args):
    """the unspliced kernel on caller-spliced vectors against the spliced kernel on raw frames, alternating"""
    left = right = 4
    D = IN_DIM // (left + right + 1)
    layers, pr = make()
    parent = capi.Models.from_mlp(pr, 3, layers)
    spl = parent.splice(left, right) if hasattr(capi.lib(), "jd_am_mlp_splice") else None
    res = []
    for rows in (8192, 64):
        f = np.random.default_rng(rows).standard_normal((rows, D)).astype(np.float32)
        idx = np.clip(np.arange(rows)[:, None] + np.arange(left + right + 1)[None, :] - left, 0, rows - 1)
        x = np.ascontiguousarray(f[idx].reshape(rows, IN_DIM))
        a, b = [], []
        for r in range(args.runs):
            a.append(float(np.median(parent.mlp_time(x, warmup=args.warmup, iters=args.iters))))
            if spl is not None:
                b.append(float(np.median(spl.mlp_time(f, warmup=args.warmup, iters=args.iters))))
        out = dict(net="-".join(str(v) for v in (IN_DIM,) + WIDTHS), rows=rows, iters=args.iters, runs=args.runs, lib=capi.LIB_PATH,
                   caller_spliced_ms=float(np.median(a)), caller_spliced_spread=[min(a), max(a)], caller_spliced_bytes=int(x.nbytes))
        if spl is not None:
            out.update(spliced_ms=float(np.median(b)), spliced_spread=[min(b), max(b)], spliced_bytes=int(f.nbytes) + 8 * rows,
                       equal=bool(np.array_equal(spl.score_frames(f).view(np.uint32), parent.score_frames(x).view(np.uint32))))
        res.append(out)
    if args.json:
        print(json.dumps(res))
        return
    for r in res:
        line = "%s, %5d rows: caller-spliced %.4f ms [%.4f .. %.4f], %d bytes to the device" % (r["net"], r["rows"], r["caller_spliced_ms"],
                                                                                                *r["caller_spliced_spread"], r["caller_spliced_bytes"])
        if "spliced_ms" in r:
            line += "   spliced (4, 4) %.4f ms [%.4f .. %.4f], %d bytes   spliced / caller-spliced %.3f   equal %s" % (
                r["spliced_ms"], *r["spliced_spread"], r["spliced_bytes"], r["spliced_ms"] / r["caller_spliced_ms"], r["equal"])
        print(line)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--json", action="store_true")
    ap.add_argument("--tied", action="store_true", help="the tied-state networks (jd_mlp_tied_kernel)")
    ap.add_argument("--bf16", action="store_true", help="also the bf16 model of the same network and torch in bf16")
    ap.add_argument("--runs", type=int, default=3, help="--bf16 / --splice: runs of each kernel, alternating")
    ap.add_argument("--splice", action="store_true", help="the network on caller-spliced vectors and its spliced model on raw frames")
    ap.add_argument("--lib", help="--splice: the libjuicer_amd.so to load instead of this tree's")
    args = ap.parse_args()
    if args.lib:
        capi.LIB_PATH = os.path.abspath(args.lib)
    assert args.runs >= 3, "at least three runs each"
    assert args.iters >= 20, "the median of at least 20 warm launches"
    if not torch.cuda.is_available():
        sys.exit("mlp_bench: no GPU (a time is a measurement on the device)")
    torch.backends.cuda.matmul.allow_tf32 = False
    if args.splice:
        return splice_bench(args)
    res = []
    for widths in (TIED_WIDTHS if args.tied else (WIDTHS,)):
        layers, pr = make(widths=widths)
        models = capi.Models.from_mlp_tied(flat_topology(widths[-1]), pr, layers) if args.tied else capi.Models.from_mlp(pr, 3, layers)
        weights = sum(w.size for w, _, _ in layers)
        for rows in (8192, 64):
            x = np.random.default_rng(rows).standard_normal((rows, IN_DIM)).astype(np.float32)
            ms = float(np.median(models.mlp_time(x, warmup=args.warmup, iters=args.iters)))
            t_ms, t_out = torch_ms(layers, np.log(pr), x, args.warmup, args.iters)
            ours = models.score_frames(x)
            flop = 2.0 * rows * weights
            if args.bf16:
                q = models.to_bf16()
                f32_runs, bf16_runs = [ms], []
                for r in range(args.runs):
                    if r:
                        f32_runs.append(float(np.median(models.mlp_time(x, warmup=args.warmup, iters=args.iters))))
                    bf16_runs.append(float(np.median(q.mlp_time(x, warmup=args.warmup, iters=args.iters))))
                tb_ms, tb_out = torch_ms(layers, np.log(pr), x, args.warmup, args.iters, torch.bfloat16)
                res.append(dict(net="-".join(str(v) for v in (IN_DIM,) + tuple(widths)), rows=rows, iters=args.iters, runs=args.runs,
                                f32_ms=float(np.median(f32_runs)), f32_spread=[min(f32_runs), max(f32_runs)],
                                bf16_ms=float(np.median(bf16_runs)), bf16_spread=[min(bf16_runs), max(bf16_runs)],
                                bf16_tflops=flop_of(rows, weights) / float(np.median(bf16_runs)) / 1e9,
                                speedup=float(np.median(f32_runs)) / float(np.median(bf16_runs)), torch_f32_ms=t_ms, torch_bf16_ms=tb_ms,
                                ratio_vs_torch_bf16=float(np.median(bf16_runs)) / tb_ms,
                                max_abs_diff_bf16_vs_f32=float(np.abs(q.score_frames(x) - ours).max()),
                                max_abs_diff_torch_bf16_vs_f32=float(np.abs(tb_out - t_out).max())))
                continue
            res.append(dict(net="-".join(str(v) for v in (IN_DIM,) + tuple(widths)), rows=rows, iters=args.iters, ms=ms, tflops=flop / ms / 1e9,
                            torch_ms=t_ms, torch_tflops=flop / t_ms / 1e9, ratio=ms / t_ms,
                            max_abs_diff_vs_torch=float(np.abs(ours - t_out).max())))
    if args.json:
        print(json.dumps(res))
    elif args.bf16:
        for r in res:
            print("%s, %5d rows: f32 kernel %.4f ms [%.4f .. %.4f]   bf16 kernel %.4f ms [%.4f .. %.4f] (%.2f TFLOP/s)   f32 / bf16 %.2f   "
                  "torch f32 %.4f ms, bf16 %.4f ms   bf16 kernel / torch bf16 %.2f   max |bf16 - f32| %.2e (torch's %.2e)"
                  % (r["net"], r["rows"], r["f32_ms"], *r["f32_spread"], r["bf16_ms"], *r["bf16_spread"], r["bf16_tflops"], r["speedup"],
                     r["torch_f32_ms"], r["torch_bf16_ms"], r["ratio_vs_torch_bf16"], r["max_abs_diff_bf16_vs_f32"],
                     r["max_abs_diff_torch_bf16_vs_f32"]))
    else:
        for r in res:
            print("%s, %5d rows: %s %.4f ms (%.2f TFLOP/s)   torch f32 %.4f ms (%.2f TFLOP/s)   ratio %.2f   max |diff| %.2e"
                  % (r["net"], r["rows"], "jd_mlp_tied_kernel" if args.tied else "jd_mlp_kernel", r["ms"], r["tflops"], r["torch_ms"],
                     r["torch_tflops"], r["ratio"], r["max_abs_diff_vs_torch"]))


if __name__ == "__main__":
    main()
