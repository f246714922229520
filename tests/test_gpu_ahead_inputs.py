"""The device path of decode_wave tied to the pure functions it calls (juicer_amd/csrc/jd_ahead.h: ahead_claim, ahead_place, ahead_table_need,
ahead_table_take): a decoder with JD_VERBOSE=1 prints, wave by wave, what those were given - the queue of batches ahead, the wave, the
decoder's streams and slab - beside what they returned, and tests/ahead_driver.cpp, built with plain g++ as tests/test_ahead_cpu.py builds
it, makes exactly those decisions of those inputs.  Nothing here depends on timing: whether a batch behind had been started is read from the
line (its bank), not assumed.

The decoder lives in a child process of its own (the lines go to stderr), under a time limit of its own."""
import json
import os
import re
import subprocess
import sys

import pytest

from ahead_cases import WAVE_OUT, build_driver, run_driver

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
IN = ["q", "retry", "nb", "n_chunks", "max_rows", "streams", "pipeline", "lazy", "G", "ll_cap"]
LINE = re.compile(r"ahead: " + " ".join(k + r" (\S+)" for k in IN) + " -> " + " ".join(k + r" (-?\d+)" for k in WAVE_OUT))

# the smallest synthetic network and models of the suite, four streams (two banks of two), three batches of two utterances of a few frames:
# announce B, announce C, decode A, announce A, decode B, decode A (not the announced batch: C is), an empty announcement
CHILD = r"""
import json, sys
import numpy as np
import torch
from juicer_amd import capi, synth
am, net, feats, _ = synth.config_toy()
gnet, gam = capi.Network.from_synth(net), capi.Models.from_htk(am)
x = feats[0]
cuts = {"A": [(0, 4), (4, 9)], "B": [(10, 13), (13, 19)], "C": [(20, 25), (25, 28)]}
dev = torch.device("cuda", 0)
buf = {}
for n, c in cuts.items():
    batch = [x[a:b] for a, b in c]
    offs = np.zeros(len(batch) + 1, dtype=np.int64)
    offs[1:] = np.cumsum([b.shape[0] for b in batch])
    buf[n] = torch.from_numpy(np.concatenate(batch)).to(dev), offs
gd = capi.Decoder(gnet, gam, max_streams=4)
hyps = []
def announce(n):
    gd.prefetch_scores(buf[n][0].data_ptr(), buf[n][1], 0)
def decode(n):
    hs = gd.decode_batch_device(buf[n][0].data_ptr(), buf[n][1], 0)
    hyps.append([n, gd.last_timing()["prefetched"]] + [[int(h.n), np.asarray(h.label).tolist(), np.asarray(h.time).tolist()] +
                [np.asarray(getattr(h, f), np.float32).view(np.uint32).tolist() for f in ("score", "ac", "lm")] for h in hs])
announce("B"); announce("C"); decode("A"); announce("A"); decode("B"); decode("A")
gd.prefetch_scores(0, None)
gd.close()
print(json.dumps({"n_gmm": gam.n_gmms, "hyps": hyps}))
"""


@pytest.fixture(scope="module")
def child(built):
    """(what the child printed, the 'ahead:' lines of its decoder as {name: text})"""
    env = dict(os.environ, JD_VERBOSE="1", PYTHONPATH=ROOT)
    r = subprocess.run(["timeout", "-k", "10", "120", sys.executable, "-c", CHILD], capture_output=True, text=True, env=env, cwd=ROOT)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
    return json.loads(r.stdout.splitlines()[-1]), [dict(zip(IN + WAVE_OUT, m.groups())) for m in LINE.finditer(r.stderr)]


def test_printed_decisions_are_the_pure_functions(child, tmp_path_factory):
    info, lines = child
    assert len(lines) == 3                                             # one per wave decoded
    driver = build_driver(str(tmp_path_factory.mktemp("ahead_gpu") / "ahead_driver"))
    out = run_driver(driver, ["wave " + " ".join(l[k] for k in IN) for l in lines])
    for l, o in zip(lines, out):
        assert [int(l[k]) for k in WAVE_OUT] == o, (l, dict(zip(WAVE_OUT, o)))
        assert (int(l["streams"]), int(l["nb"]), int(l["n_chunks"]), int(l["G"]), int(l["retry"])) == (4, 2, 1, info["n_gmm"], 0), l
    first, second, third = lines
    # A: nothing had been scored yet - B and C wait, announced; on a bank
    assert first["q"].count(";") == 1 and all(e.startswith("1,") for e in first["q"].split(";"))
    assert (first["mine"], first["drop"], first["pipe"]) == ("0", "0", "1")
    # B: the announced batch at the head of the queue, its table scored beside A
    assert second["q"].split(";")[0].startswith("2,") and second["q"].split(";")[0].endswith(",1") and second["mine"] == "1"
    # A again: C is the batch at the head - what was worked ahead is dropped
    assert (third["mine"], third["drop"]) == ("0", "1") and third["q"].split(";")[0].endswith(",0")


def test_results_do_not_depend_on_working_ahead(child):
    info, _ = child
    names = [h[0] for h in info["hyps"]]
    assert names == ["A", "B", "A"] and [h[1] for h in info["hyps"]] == [0, 1, 0]
    assert info["hyps"][0][2:] == info["hyps"][2][2:] and all(len(h) == 4 for h in info["hyps"])
