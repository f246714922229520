"""The device path of ensure_arenas tied to the pure function it calls (juicer_amd/csrc/jd_arena.h: arena_caps): a decoder with
JD_VERBOSE=1 prints what arena_caps was given - the free and the cached bytes, the fraction, the fit passes - beside the capacities it
allocated, and tests/arena_driver.cpp, built with plain g++ as tests/test_arena_cpu.py builds it, makes exactly those capacities of
those inputs.  Free memory on a shared machine varies: nothing of it is assumed here.

Each decoder lives in a child process of its own (the line goes to stderr, and a slab cached by an earlier test is not this test's
business), under a time limit of its own; the second child starts only when the first has ended well."""
import json
import os
import re
import subprocess
import sys

import pytest

from arena_cases import CAPS_OUT, build_driver, caps_line, run_driver

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SET = dict(max_slots=1000, max_items=100, max_paths=1 << 15)
LINE = re.compile(r"arenas: slots (\d+), items (\d+), Path records (\d+) per stream x (\d+) streams in [0-9.]+ s "
                  r"\(free (\d+), cached (\d+) bytes, fraction (\S+), (\d+) fit passes\)")

# the smallest synthetic network and models of the suite, two streams, one utterance of 3 frames; with "default" a second decoder after
# the first one's end, which finds the first one's slab cached
CHILD = r"""
import json, sys
import numpy as np
from juicer_amd import capi, synth
am, net, feats, _ = synth.config_toy()
gnet, gam = capi.Network.from_synth(net), capi.Models.from_htk(am)
kw = json.loads(sys.argv[1])
hyps = []
for rep in range(2 if not kw else 1):
    gd = capi.Decoder(gnet, gam, max_streams=2, **kw)
    h = gd.decode_batch([feats[0][:3]])[0]
    hyps.append([int(h.n), np.asarray(h.label).tolist(), np.asarray(h.time).tolist()] +
                [np.asarray(getattr(h, f), np.float32).view(np.uint32).tolist() for f in ("score", "ac", "lm")])
    gd.close()
print(json.dumps({"n_arcs": gnet.n_arcs, "n_states": gnet.n_states, "n_gmm": gam.n_gmms, "max_n": gam.max_states, "hyps": hyps}))
"""


@pytest.fixture(scope="module")
def children(built):
    """{case: (what the child printed, the 'arenas:' lines of its decoders)}"""
    env = dict(os.environ, JD_VERBOSE="1", PYTHONPATH=ROOT)
    out = {}
    for case, kw in (("default", {}), ("set", SET)):
        r = subprocess.run(["timeout", "-k", "10", "120", sys.executable, "-c", CHILD, json.dumps(kw)], capture_output=True, text=True, env=env, cwd=ROOT)
        assert r.returncode == 0, (case, r.returncode, r.stdout[-2000:], r.stderr[-2000:])
        out[case] = json.loads(r.stdout.splitlines()[-1]), [m.groups() for m in LINE.finditer(r.stderr)]
    return out


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    with open(os.path.join(HERE, "golden", "arena_golden.json")) as f:
        sizes = json.load(f)["sizes"]
    return build_driver(str(tmp_path_factory.mktemp("arena_gpu") / "arena_driver")), sizes


def check(driver, info, line, kw):
    """the printed capacities are what the CPU driver makes of the printed inputs; returns the inputs and the driver's output"""
    exe, sizes = driver
    slots, items, paths, B, free_b, cached_b, frac, passes = line
    i = {"free_bytes": int(free_b), "cached_bytes": int(cached_b), "mem_fraction": frac, "B": int(B), "n_arcs": info["n_arcs"],
         "n_states": info["n_states"], "Fc": 128, "n_gmm": info["n_gmm"], "max_n": info["max_n"], "cap_slots": kw.get("max_slots", 0),
         "cap_items": kw.get("max_items", 0), "cap_paths": kw.get("max_paths", 0), "slots_hint": 0}
    assert float(frac) == 0.7 and int(B) == 2                          # (the first attempt's fraction: nothing had to be halved)
    o = dict(zip(CAPS_OUT, run_driver(exe, [caps_line(i, sizes)])[0]))
    assert o["status"] == 0
    assert (o["cap_slots"], o["cap_items"], o["cap_paths"], o["passes"]) == (int(slots), int(items), int(paths), int(passes)), (i, o)
    return i, o


def test_default_capacities_are_the_pure_functions(children, driver):
    info, lines = children["default"]
    assert len(lines) == 2 and len(info["hyps"]) == 2
    first, o = check(driver, info, lines[0], {})
    second, _ = check(driver, info, lines[1], {})
    assert first["cached_bytes"] == 0 and first["free_bytes"] > 0
    assert second["cached_bytes"] == o["bytes"] * 2                    # the second decoder finds the first one's slab: its two streams' bytes
    assert info["hyps"][0] == info["hyps"][1]


def test_set_capacities_are_the_pure_functions(children, driver):
    info, lines = children["set"]
    assert len(lines) == 1
    _, o = check(driver, info, lines[0], SET)
    # whatever the free memory: slots rounded down to 64, items raised to a cluster's least, the Path records as set
    assert (o["cap_slots"], o["cap_items"], o["cap_paths"]) == (960, 64 * driver[1]["sw"], 1 << 15)
    assert info["hyps"] == children["default"][0]["hyps"][:1]
