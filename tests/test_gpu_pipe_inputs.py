"""The device path of the slot pipeline (JD_FLOW_RESIDENT) tied to the pure functions it calls (juicer_amd/csrc/jd_pipe.h: pipe_size, pipe_size_piece,
pipe_enqueue): a decoder with JD_VERBOSE=1 prints what those were given beside what they returned - when the pipeline is sized, and with every
announcement - and tests/pipe_driver.cpp, built with plain g++ as tests/test_pipe_cpu.py builds it, makes exactly those decisions of those inputs.
Every batch handed back prints what the pump did for it; what of that does not depend on timing is checked: the tables, the order of taking, the
scoring pieces and - where no slot stopped for a Path collection - the commands.  The same batches through FLOW_SERIAL give the same hypotheses,
bit for bit.

The decoder lives in a child process of its own (the lines go to stderr), under a time limit of its own."""
import json
import os
import re
import subprocess
import sys

import pytest

from pipe_cases import SIZE_IN, SIZE_OUT, build_driver, run_driver

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CHUNK = 16
SIZE = re.compile(r"pipe: size " + " ".join(k + r" (-?\d+)" for k in SIZE_IN) + " -> " + " ".join(k + r" (-?\d+)" for k in SIZE_OUT))
ANNOUNCE = re.compile(r"pipe: announce K (\d+) table_rows (\d+) used (\S+) T (\S+) -> table (\d+) row0 (\S+) order (\S+)")
BACK = re.compile(r"pipe: back serial (\d+) table (\d+) utts (\d+) commands (\d+) pieces (\d+) -> (-?\d+)")
# utterances of 17, 1 and 40 frames; of exactly a chunk and 33; of 9 and 16 - cut from the toy configuration's one feature matrix
CUTS = {"A": [(0, 17), (17, 18), (18, 58)], "B": [(58, 74), (74, 107)], "C": [(100, 109), (30, 46)]}

# the smallest synthetic network and models of the suite, four streams, two slots, three tables, commands of 16 frames:
# announce A, announce B, decode A, announce C, decode B, decode C - then the same three batches one after the other (FLOW_SERIAL)
CHILD = r"""
import json, sys
import numpy as np
import torch
from juicer_amd import capi, synth
am, net, feats, _ = synth.config_toy()
gnet, gam = capi.Network.from_synth(net), capi.Models.from_htk(am)
x = feats[0]
cuts = json.loads(sys.argv[1])
dev = torch.device("cuda", 0)
buf = {}
for n, c in cuts.items():
    batch = [x[a:b] for a, b in c]
    offs = np.zeros(len(batch) + 1, dtype=np.int64)
    offs[1:] = np.cumsum([b.shape[0] for b in batch])
    buf[n] = torch.from_numpy(np.concatenate(batch)).to(dev), offs
gd = capi.Decoder(gnet, gam, max_streams=4)
gd.set_pipeline(capi.FLOW_RESIDENT, 3, 2)
hyps = {"resident": [], "serial": []}
def announce(n):
    gd.prefetch_scores(buf[n][0].data_ptr(), buf[n][1], 0)
def decode(n, into):
    hs = gd.decode_batch_device(buf[n][0].data_ptr(), buf[n][1], 0)
    hyps[into].append([n, gd.last_timing()["prefetched"]] + [[int(h.n), np.asarray(h.label).tolist(), np.asarray(h.time).tolist()] +
                      [np.asarray(getattr(h, f), np.float32).view(np.uint32).tolist() for f in ("score", "ac", "lm")] for h in hs])
announce("A"); announce("B"); decode("A", "resident"); announce("C"); decode("B", "resident"); decode("C", "resident")
stats = gd.pipeline_stats()
gd.set_pipeline(capi.FLOW_SERIAL)
for n in "ABC":
    decode(n, "serial")
gd.close()
print(json.dumps({"hyps": hyps, "stats": stats}))
"""


@pytest.fixture(scope="module")
def child(built):
    """(what the child printed, its decoder's stderr)"""
    env = dict(os.environ, JD_VERBOSE="1", JD_DEV="1", JD_PIPE_CHUNK=str(CHUNK), PYTHONPATH=ROOT)
    r = subprocess.run(["timeout", "-k", "10", "120", sys.executable, "-c", CHILD, json.dumps(CUTS)], capture_output=True, text=True, env=env, cwd=ROOT)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
    return json.loads(r.stdout.splitlines()[-1]), r.stderr


def ints(s):
    return [] if s == "-" else [int(x) for x in s.split(",")]


def test_printed_decisions_are_the_pure_functions(child, tmp_path_factory):
    info, err = child
    lens = {n: [b - a for a, b in c] for n, c in CUTS.items()}
    size, announced, back = SIZE.findall(err), ANNOUNCE.findall(err), BACK.findall(err)
    assert len(size) == 1 and len(announced) == 3 and len(back) == 3, err[-3000:]
    driver = build_driver(str(tmp_path_factory.mktemp("pipe_gpu") / "pipe_driver"))
    # the sizing: what pipe_fill gave pipe_size / pipe_size_piece, and what they returned
    sized = dict(zip(SIZE_IN + ["out_" + k for k in SIZE_OUT], (int(v) for v in size[0])))
    assert run_driver(driver, ["size " + " ".join(size[0][:len(SIZE_IN)])]) == [[sized["out_" + k] for k in SIZE_OUT]]
    assert (sized["depth"], sized["slots"], sized["streams"], sized["utts"], sized["rows"], sized["chunk"]) == (3, 2, 4, 3, sum(lens["A"]), CHUNK)
    assert (sized["out_K"], sized["out_n_slots"], sized["out_chunk"], sized["out_max_batch"]) == (3, 2, CHUNK, 6)
    # the announcements: tables in use and lengths in, table / first rows / order out
    out = run_driver(driver, ["enqueue %s %s %s %d %s" % (K, rows, " ".join(map(str, ints(used))), len(ints(T)), " ".join(map(str, ints(T))))
                              for K, rows, used, T, _, _, _ in announced])
    for (K, rows, used, T, table, row0, order), o, name in zip(announced, out, "ABC"):
        assert ints(T) == lens[name] and int(rows) == sized["out_table_rows"], (name, T)
        assert [int(table)] + ints(row0) + ints(order) == o, (name, o)
        assert ints(order) == sorted(range(len(lens[name])), key=lambda u: -lens[name][u]), name      # longest first (stable)
    assert [int(a[4]) for a in announced] == [0, 1, 0]                  # tables 0, 1, then the one A freed
    assert [ints(a[2]) for a in announced] == [[0, 0, 0], [1, 0, 0], [0, 1, 0]]
    # the batches handed back: serial numbers and tables; pieces and commands as the lengths say
    assert info["stats"]["collections"] == 0, "slots stopped for %d Path collection(s): the commands cannot be counted" % info["stats"]["collections"]
    for (serial, table, utts, commands, pieces, rc), name, k in zip(back, "ABC", range(3)):
        assert (int(serial), int(table), int(utts), int(rc)) == (k, [0, 1, 0][k], len(lens[name]), 0), name
        assert int(pieces) == -(-sum(lens[name]) // sized["out_piece_rows"]), name
        assert int(commands) == sum(max(1, -(-T // CHUNK)) for T in lens[name]), name
    assert info["stats"]["batches_back"] == 3 and info["stats"]["utts_through"] == sum(len(l) for l in lens.values())


def test_resident_flow_gives_the_serial_flow_s_hypotheses(child):
    info, _ = child
    res, ser = info["hyps"]["resident"], info["hyps"]["serial"]
    assert [h[0] for h in res] == ["A", "B", "C"] == [h[0] for h in ser]
    assert [h[1] for h in res] == [1, 1, 1] and [h[1] for h in ser] == [0, 0, 0]
    for r, s in zip(res, ser):
        assert r[2:] == s[2:], r[0]                                     # labels, times and the bits of the scores
        assert len(r) - 2 == len(CUTS[r[0]])
