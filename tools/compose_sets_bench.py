#!/usr/bin/env python
"""Label-set look-ahead (JD_LOOKAHEAD_SETS) at the size of bench.py's configs[4] leg: C.L (20 k-word lexicon tree) o G (back-off
trigram), composed on the device with the look-ahead on intervals and on sets, for the generator's own word numbering (where the two
are the same thing) and for a randomly renumbered vocabulary (synth.permute_words).  Prints composed sizes,
compose times (alternating runs, --reps each), the host time of the set computation alone, and frames/s of decoding the same
utterances on each composed graph; one JSON line at the end.

The pair is the one bench.py's compose_leg builds for configs[4] (make_cl_g: 20000 words, 40 successors, 200000 trigram
histories, 8 trigram successors, tee model; G loaded with scale 10; beam 200; 64 utterances of 8 words) - the 8.4 M-arc composed
graph of the README's configs[4] row.  (synth.config_c4 is the already-composed configs[3] graph and has no separate G.)  The
comparison here is sets against intervals inside one build; against another commit, run the tool in both trees alternately.

  python tools/compose_sets_bench.py [--words 20000 --succ 40 --tri 200000] [--reps 5] [--utts 64]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from juicer_amd import capi, synth  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--words", type=int, default=20000)
ap.add_argument("--succ", type=int, default=40)
ap.add_argument("--tri", type=int, default=200000)
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--utts", type=int, default=64)
ap.add_argument("--mix", type=int, default=16)
args = ap.parse_args()

am = synth.make_models(0, n_gmm=3000, n_hmm=2000, n_mix=args.mix, n_tm=8, sep=0.6, with_tee=True)
cl, g = synth.make_cl_g(0, am, n_words=args.words, n_succ=args.succ, n_tri=args.tri, n_succ3=8, with_sp=True)
feats = [synth.sample_utterance(100 + u, g, am, 8)[0] for u in range(args.utts)]
frames = sum(f.shape[0] for f in feats)
models = capi.Models.from_htk(am)
out = {"cl_arcs": int(cl.n_arcs), "g_arcs": int(g.n_arcs), "frames": frames, "reps": args.reps}
ref_labels = None
for name, (xcl, xg) in (("generator numbering", (cl, g)), ("renumbered", synth.permute_words(cl, g, synth.random_word_permutation(cl, g, 1)))):
    ncl, ng = capi.Network.from_synth(xcl, 1.0, 0.0), capi.Network.from_synth(xg, 10.0, 0.0)
    t0 = time.perf_counter()
    rp, labels, _ = ncl.label_sets()
    t_sets = time.perf_counter() - t0                                  # (the set computation plus writing every set out)
    row = {"label_sets_host_seconds": round(t_sets, 4), "set_entries": int(labels.shape[0])}
    modes = [False, True]
    try:
        capi.Network.compose(ncl, ng, max_states=1 << 27, max_arcs=1 << 28)    # warm-up: allocator, code objects
    except capi.JuicerAmdError as e:                                   # the loose intervals of a renumbered vocabulary: too large to hold
        t0 = time.perf_counter()
        try:
            capi.Network.compose(ncl, ng, max_states=1 << 27, max_arcs=1 << 28)
        except capi.JuicerAmdError:
            pass
        row["intervals"] = {"error": str(e), "seconds_until_error": round(time.perf_counter() - t0, 3)}
        print("%-20s intervals: %s (after %.2f s)" % (name, e, time.perf_counter() - t0), flush=True)
        modes = [True]
        capi.Network.compose(ncl, ng, max_states=1 << 27, max_arcs=1 << 28, lookahead_sets=True)
    times = {False: [], True: []}
    nets = {}
    for _ in range(args.reps):
        for sets in modes:                                             # alternating
            t0 = time.perf_counter()
            nets[sets] = capi.Network.compose(ncl, ng, max_states=1 << 27, max_arcs=1 << 28, lookahead_sets=sets)
            times[sets].append(time.perf_counter() - t0)
    for sets in modes:
        net = nets[sets]
        dec = capi.Decoder(net, models, main_beam=200.0, max_streams=len(feats))
        hyps = dec.decode_batch(feats)                                 # warm-up
        best = None
        for _ in range(3):
            t0 = time.perf_counter()
            hyps = dec.decode_batch(feats)
            dt = time.perf_counter() - t0
            best = dt if best is None else min(best, dt)
        lab = [h.label.tolist() for h in hyps]
        if ref_labels is None:
            ref_labels = lab
        t = times[sets]
        row["sets" if sets else "intervals"] = {
            "states": net.n_states, "arcs": net.n_arcs, "compose_seconds_median": round(statistics.median(t), 4),
            "compose_seconds_min": round(min(t), 4), "compose_seconds_max": round(max(t), 4),
            "decode_frames_per_s": round(frames / best, 1), "same_words_as_first": lab == ref_labels}
        print("%-20s %-9s %9d states %10d arcs  compose median %.3f s [%.3f .. %.3f]  decode %.0f frames/s  same words: %s" % (
            name, "sets" if sets else "intervals", net.n_states, net.n_arcs, statistics.median(t), min(t), max(t), frames / best, lab == ref_labels),
            flush=True)
        del dec
    print("%-20s label sets on the host: %.3f s" % (name, t_sets), flush=True)
    out[name] = row
    del nets
print(json.dumps(out))
