"""The streaming interface on the device tied to the pure functions it calls (juicer_amd/csrc/jd_push.h: push_chunk_frames, push_round_plan,
push_after, push_book_collection): a decoder with JD_VERBOSE=1 prints what those were given beside what they returned - a "push:" line per chunk
or round, per control block read behind a launch, per collection booked - and tests/push_driver.cpp, built with plain g++ as
tests/test_push_cpu.py builds it, makes exactly those decisions of those inputs.  The same frames go through jd_streams_push (uneven sizes per
stream, calls that skip a stream, calls that list one without frames) and through jd_stream_push, stream by stream, under PARTIAL_DECODING with
intervals 1 and 150: collections, partial lists after every call and the hypotheses are the same, bit for bit, and the oracle's.

The decoder lives in a child process of its own (the lines go to stderr), under a time limit of its own."""
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from push_cases import AFTER_IN, AFTER_OUT, build_driver, j, run_driver

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
ROTATIONS = ((2, 3), (3, 2), (2, 1))                                    # a stream's input: two of the configuration's utterances, one after the other
SIZES = (37, 64, 150)                                                   # frames per call of stream 0, 1, 2
INTERVALS = (1, 150)
CHUNK = re.compile(r"push: chunk stream (-?\d+) Fc (-?\d+) left (-?\d+) interval (-?\d+) last_collect (-?\d+) T (-?\d+) -> n (-?\d+)")
ROUND = re.compile(r"push: round T (\S+) last_collect (\S+) work (\S+) target (\S+) out (\S+) -> act (\S+) limit (\S+) hT (\S+) f_end (-?\d+) s_lo (-?\d+) s_hi (-?\d+)")
AFTER = re.compile(r"push: after stream (-?\d+) " + " ".join(k + r" (-?\d+)" for k in AFTER_IN) + " -> " + " ".join(k + r" (-?\d+)" for k in AFTER_OUT))
BOOK = re.compile(r"push: book stream (-?\d+) at (-?\d+) last_trace (-?\d+) interval (-?\d+) -> due (-?\d+) last_collect (-?\d+) n_collect (-?\d+)")


def calls_of(lengths):
    """The calls: per call a list of (stream, lo, hi) - stream k advances by SIZES[k] frames per call it takes part in, is left out of some calls
    (not listed) and listed without frames in others."""
    pos, calls, c = [0] * len(lengths), [], 0
    while any(p < T for p, T in zip(pos, lengths)):
        call = []
        for k, T in enumerate(lengths):
            if pos[k] >= T or (c + k) % 3 == 0:
                continue                                                # through, or not listed
            hi = pos[k] if (c + 2 * k) % 5 == 0 else min(T, pos[k] + SIZES[k])     # (listed, n_frames = 0)
            call.append((k, pos[k], hi))
            pos[k] = hi
        c += 1
        if call:
            calls.append(call)
    return calls


# three streams of the small tree-hub configuration; per interval the calls once through jd_streams_push and once through jd_stream_push.  Every
# run: a marker on stderr, then after every call each stream's (partial list, collection info), then the hypotheses, and the launches counted
CHILD = r"""
import json, sys
import numpy as np
from juicer_amd import capi, synth
am, net, feats, _ = synth.config_small(hub="tree")
gnet, gam = capi.Network.from_synth(net), capi.Models.from_htk(am)
arg = json.loads(sys.argv[1])
xs = [np.concatenate([feats[i] for i in rot]) for rot in arg["rotations"]]
runs = []
for interval in arg["intervals"]:
    for many in (1, 0):
        gd = capi.Decoder(gnet, gam, max_streams=3, main_beam=150.0)
        gd.set_partial_interval(interval)
        for s in range(3):
            gd.stream_init(s)
        sys.stderr.write("push-test: run interval %d many %d\n" % (interval, many)); sys.stderr.flush()
        trail = []
        for call in arg["calls"]:
            if many:
                gd.streams_push([k for k, _, _ in call], [xs[k][lo:hi] for k, lo, hi in call])
            else:
                for k, lo, hi in call:
                    gd.stream_push(k, xs[k][lo:hi])
            trail.append([[gd.stream_partial(s)[1], list(gd.stream_collect_info(s))] for s in range(3)])
        t = gd.last_timing()
        hyps = []
        for s in range(3):
            g = gd.stream_finish(s)
            hyps.append([int(g.n), g.label.tolist(), g.time.tolist()] + [np.asarray(getattr(g, f), np.float32).view(np.uint32).tolist() for f in ("score", "ac", "lm")]
                        + [gd.stream_partial(s)[1]])
        gd.close()
        runs.append({"interval": interval, "many": many, "trail": trail, "hyps": hyps, "launches": [t["search_launches"], t["relaunches"], t["trace_launches"]]})
print(json.dumps(runs))
"""


@pytest.fixture(scope="module")
def inputs(built):
    from juicer_amd import synth
    feats = synth.config_small(hub="tree")[2]
    xs = [np.concatenate([feats[i] for i in rot]) for rot in ROTATIONS]
    assert all(x.shape[0] > 202 for x in xs)                            # two frame-rule collections at least
    return xs, calls_of([x.shape[0] for x in xs])


@pytest.fixture(scope="module")
def oracle(built, inputs):
    """per interval and stream: (snapshots, final list, collect frames) - computed once, shared, never changed"""
    from juicer_amd import synth
    from oracle.oracle import OracleAM, OracleDecoder, OracleNet
    am, net, _, _ = synth.config_small(hub="tree")
    od = OracleDecoder(OracleNet(net), OracleAM(am), main_beam=150.0)
    ora = {}
    for interval in INTERVALS:
        ora[interval] = []
        for x in inputs[0]:
            snaps, final = od.decode_partial(x, interval=interval)
            ora[interval].append((snaps, final, list(od.collect_frames)))
    return ora


@pytest.fixture(scope="module")
def child(built, inputs):
    """(the runs the child printed, its decoders' stderr cut at the runs' markers)"""
    env = dict(os.environ, JD_VERBOSE="1", PYTHONPATH=ROOT)
    arg = json.dumps({"rotations": ROTATIONS, "intervals": INTERVALS, "calls": inputs[1]})
    r = subprocess.run(["timeout", "-k", "10", "180", sys.executable, "-c", CHILD, arg], capture_output=True, text=True, env=env, cwd=ROOT)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
    runs = json.loads(r.stdout.splitlines()[-1])
    parts = re.split(r"push-test: run interval \d+ many \d\n", r.stderr)[1:]
    assert len(parts) == len(runs) == 2 * len(INTERVALS)
    return runs, parts


def ints(s):
    return [] if s == "-" else [int(x) for x in s.split(",")]


def pairs(lst):
    return [(int(l), int(f)) for l, f in lst]


def test_printed_decisions_are_the_pure_functions(child, inputs, tmp_path_factory):
    runs, parts = child
    driver = build_driver(str(tmp_path_factory.mktemp("push_gpu") / "push_driver"))
    n_frames = sum(hi - lo for call in inputs[1] for _, lo, hi in call)
    for run, err in zip(runs, parts):
        chunks, rounds, afters, books = CHUNK.findall(err), ROUND.findall(err), AFTER.findall(err), BOOK.findall(err)
        where = (run["interval"], run["many"])
        lines, want = [], []
        for s, Fc, left, interval, lc, T, n in chunks:
            lines.append(j("chunk", Fc, left, interval, lc, T)); want.append([int(n)])
        for T, lc, work, target, out, act, limit, hT, f_end, s_lo, s_hi in rounds:
            lines.append(j("round", len(ints(T)), list(zip(ints(T), ints(lc))), len(ints(work)), list(zip(ints(work), ints(target), ints(out)))))
            want.append([len(ints(act))] + ints(act) + ints(limit) + [l - ints(T)[ints(work)[k]] for k, l in zip(ints(act), ints(limit))] + [int(f_end), int(s_lo), int(s_hi)] + ints(hT))
        for a in afters:
            v = dict(zip(AFTER_IN, (int(x) for x in a[1:1 + len(AFTER_IN)])))
            lines.append(j("after", [v[k] for k in AFTER_IN], -1, 1)); want.append([int(x) for x in a[1 + len(AFTER_IN):]])
        for s, at, lt, interval, due, lc, nc in books:
            lines.append(j("book", at, lt, interval, int(nc) - 1)); want.append([int(due), int(lc), int(nc)])
        got = run_driver(driver, lines)
        for l, w, g in zip(lines, want, got):
            assert g[:len(w)] == w, (where, l, w, g)
        # what was printed is what the run did: one path prints chunks, the other rounds; every frame pushed is in a chunk; a line per collection
        assert (len(chunks) > 0, len(rounds) > 0) == ((False, True) if run["many"] else (True, False)), where
        if not run["many"]:
            assert sum(int(c[6]) for c in chunks) == n_frames and all(int(c[3]) == run["interval"] for c in chunks), where
        assert len(books) == sum(run["trail"][-1][s][1][0] for s in range(3)) and len(afters) >= len(books), where
        assert all(int(a[8]) == 0 for a in afters) if run["many"] else True, where     # by_flag: never in the many-stream path


def test_both_paths_agree_bit_for_bit(child):
    runs, _ = child
    by = {(r["interval"], r["many"]): r for r in runs}
    for interval in INTERVALS:
        one, many = by[(interval, 0)], by[(interval, 1)]
        assert len(one["trail"]) == len(many["trail"])
        for c, (a, b) in enumerate(zip(one["trail"], many["trail"])):
            assert a == b, (interval, "call", c)
        assert one["hyps"] == many["hyps"], interval                    # labels, times, the bits of the scores, the completed lists


def test_both_paths_are_the_oracle_s(child, inputs, oracle):
    runs, _ = child
    xs, calls = inputs
    for run in runs:
        ora = oracle[run["interval"]]
        at = [-1] * 3
        for call, after in zip(calls, run["trail"]):
            for k, lo, hi in call:
                at[k] = hi - 1
            for s in range(3):
                snaps, _, cframes = ora[s]
                due = [f for f in sorted(snaps) if f <= at[s]]
                done = [f for f in cframes if f <= at[s]]
                where = (run["interval"], run["many"], s, at[s])
                assert pairs(after[s][0]) == (pairs(snaps[due[-1]][1]) if due else []), where
                assert after[s][1] == [len(done), done[-1] if done else -1], where
        for s in range(3):
            n, label, time = run["hyps"][s][:3]
            final = pairs(run["hyps"][s][6])
            assert final == pairs(ora[s][1]) == list(zip(label[::-1], time[::-1])) and n == len(final), (run["interval"], run["many"], s)
            assert len(ora[s][2]) >= 2 and ora[s][2] == list(range(100, xs[s].shape[0], 101))     # the frame rule alone, twice at least
