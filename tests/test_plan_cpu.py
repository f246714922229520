"""The cluster plan of a search launch (juicer_amd/csrc/jd_plan.h) on the CPU: tests/plan_driver.cpp, compiled with plain g++, is held
to tests/golden/plan_golden.json - the plans the lines of launch_search that jd_plan.h replaced made of the same inputs, recorded from
the commit named in the file - integer by integer, and the same plans are checked for what a legal plan is.

Three branches the planner has cannot be reached through plan_clusters, so no case reaches them (they stay in the code as they were):
- an eighth running out of room in the XCD packing: the unpacked clusters never add up to more than the grid, a cluster that is placed
  takes at most its unpacked size and at least one workgroup, so while a cluster is left to place an eighth has room left;
- a second round of the largest-remainder passes that deals anything: the bisection ends with wants that add up to the grid (left-overs:
  the sum of the fractions, fewer than the streams with one, each of which is below its cap) or with every stream at its cap (nothing
  to deal: the rounds run, cases "bisect_all_capped*");
- the overshoot trim with weights a decoder can see: it needs a tau beyond the bisection's 1e15 us, i.e. streams of some 1e14 frames
  (cases "bisect_overshoot_trim*" do that).
"""
import json
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SCALARS = ["n_work", "has_weight", "n_bg", "nwg_all", "max_cw", "fg_cw_cap", "bg_cw_cap", "bg_weight_m", "weighted", "plan_mode", "plan_min_cw",
           "a_m", "b_m", "a2_m", "b2_m", "load_scale_m", "gmm_ms_per_wg_m", "xl_ok", "xl_slack_m", "rebalance", "bg_rebalance", "rebalance_frac_m",
           "rebalance_min_us_m"]


def _line(c):
    v = dict(c, has_weight=0 if c["weight_m"] is None else 1, n_bg=len(c["bg_left_m"]))
    w = c["weight_m"] if c["weight_m"] is not None else [0] * c["n_work"]
    return " ".join(str(x) for x in [v[k] for k in SCALARS] + w + c["bg_left_m"])


def _run(driver, inputs):
    text = "%d\n" % len(inputs) + "\n".join(_line(c) for c in inputs) + "\n"
    lines = subprocess.run([driver], input=text, capture_output=True, text=True, check=True).stdout.splitlines()
    assert len(lines) == len(inputs)
    outs = []
    for l in lines:
        o = [int(x) for x in l.split()]
        assert len(o) == 7 + 4 * o[6]
        outs.append({"weighted": o[0], "xl": o[1], "grid": o[2], "Cw": o[3], "n_slots": o[4], "rebalance_at": o[5],
                     "items": [o[7 + 4 * i:11 + 4 * i] for i in range(o[6])]})
    return outs


@pytest.fixture(scope="module")
def plans(tmp_path_factory):
    """[(name, input, golden output, output, output with XCD-local launches off)]"""
    gxx = shutil.which("g++")
    assert gxx, "g++ not found"
    driver = str(tmp_path_factory.mktemp("plan") / "plan_driver")
    subprocess.check_call([gxx, "-std=c++17", "-Wall", "-Werror", "-ffp-contract=off", "-I", os.path.join(ROOT, "juicer_amd", "csrc"),
                           "-o", driver, os.path.join(HERE, "plan_driver.cpp")])
    with open(os.path.join(HERE, "golden", "plan_golden.json")) as f:
        doc = json.load(f)
    inputs = []
    for c in doc["cases"]:
        i = dict(doc["defaults"], **c["in"])
        if i["weight_m"] is not None:
            i["n_work"] = len(i["weight_m"])
        inputs.append(i)
    outs = _run(driver, inputs)
    plain = _run(driver, [dict(i, xl_ok=0) for i in inputs])           # (the unpacked plan, to tell what the packing did)
    return [(c["name"], i, c["out"], o, p) for c, i, o, p in zip(doc["cases"], inputs, outs, plain)]


def test_plan_matches_recorded(plans):
    assert len(plans) >= 100
    bad = [name for name, _, want, got, _ in plans if want != got]
    for name, _, want, got, _ in plans:
        if want != got:
            print(name, "recorded", want, "now", got)
    assert not bad


def _caps(i):
    n_bg = len(i["bg_left_m"])
    mcw = min(i["max_cw"], i["fg_cw_cap"]) if n_bg else i["max_cw"]
    return mcw, max(1, min(i["bg_cw_cap"], i["max_cw"]))


def test_plan_is_legal(plans):
    for name, i, _, o, _ in plans:
        n_work, n_bg, nwg_all = i["n_work"], len(i["bg_left_m"]), i["nwg_all"]
        items = o["items"]
        assert o["grid"] <= nwg_all, name
        assert len(items) == (n_work + n_bg if o["weighted"] else n_work), name
        assert sorted(it[0] for it in items) == list(range(len(items))), name
        # foreground flags on exactly the streams of the running batch
        assert all(fg == (1 if idx < n_work else 0) for idx, _, _, fg in items), name
        mcw, mcw_bg = _caps(i)
        for idx, first, cw, fg in items:
            assert cw >= 1, name
            assert cw <= (mcw if fg else mcw_bg) if o["weighted"] else cw == o["Cw"], name
        # disjoint, inside the grid.  (Uniform clusters with more streams than clusters - n_slots < n_work - are numbered past the
        # grid as they always were: the kernel's clusters take the streams in turn and do not read these positions.)
        in_turn = not o["weighted"] and o["n_slots"] < n_work
        end = 0
        for idx, first, cw, fg in sorted(items, key=lambda it: it[1]):
            assert first >= end, name
            end = first + cw
            assert in_turn or end <= o["grid"], name
        if o["xl"]:
            bin_ = (o["grid"] if not o["weighted"] else nwg_all) // 8
            assert (o["grid"] if not o["weighted"] else nwg_all) % 8 == 0, name
            assert [it[1] for it in items] == sorted(it[1] for it in items), name
            for idx, first, cw, fg in items:
                assert first // bin_ == (first + cw - 1) // bin_, name
        if not o["weighted"]:
            assert o["rebalance_at"] == 0 and o["n_slots"] >= 1, name
        else:
            assert o["n_slots"] == 0, name


def _finish_us(i, frames_m, cw):
    greedy = i["plan_mode"] == 1
    a, b = (i["a2_m"], i["b2_m"]) if greedy else (i["a_m"], i["b_m"])
    return max(frames_m / 1000.0, 1.0) * (a / 1000.0 + b / 1000.0 * (i["load_scale_m"] / 1000.0) / cw)


def _branches(name, i, o, plain):
    """the branches of the planner a case reaches, told from its input and its plans"""
    n_work, n_bg, nwg_all = i["n_work"], len(i["bg_left_m"]), i["nwg_all"]
    nwg = nwg_all - n_bg
    w = i["weight_m"]
    got = set()
    if not o["weighted"]:
        if w is None:
            got.add("uniform: no weights")
        elif not i["weighted"]:
            got.add("uniform: weighted off")
        elif n_work == 1 and n_bg == 0:
            got.add("uniform: one stream, no background")
        elif i["max_cw"] == 1:
            got.add("uniform: max_cw 1")
        elif nwg < 2 * n_work:
            got.add("uniform: nwg < 2 n_work")
        if i["xl_ok"] and o["Cw"] > 1:
            got.add("uniform: XCD-local" if o["xl"] else "uniform: not XCD-local")
        return got
    mcw, mcw_bg = _caps(i)
    cw = {idx: c for idx, _, c, _ in plain["items"]}                   # the unpacked clusters
    fg_sum = sum(cw[k] for k in range(n_work))
    if i["plan_mode"] == 0:
        caps_sum = n_work * mcw + n_bg * mcw_bg
        if len(set(w)) == 1:
            got.add("bisection: equal weights")
        if n_work > 2 and max(w) == 10 * min(w) and sorted(w)[-2] == min(w):
            got.add("bisection: one stream ten times longer")
        if min(w) == 0 and any(0 < x < 1000 for x in w):
            got.add("bisection: weights of 0 and below 1")
        if caps_sum < nwg + n_bg and all(cw[k] == (mcw if k < n_work else mcw_bg) for k in cw):
            got.add("bisection: every want above the cap")
            got.add("bisection: remainder passes go round more than once")
        if min(w) >= 10 ** 17 and caps_sum > nwg + n_bg and sum(cw.values()) == nwg + n_bg:
            got.add("bisection: overshoot trim")
    else:
        last = max(range(n_work), key=lambda k: _finish_us(i, w[k], cw[k]))
        if n_bg == 0 and fg_sum < nwg and i["gmm_ms_per_wg_m"] == 0 and cw[last] == mcw:
            got.add("greedy: stops at mcw")
        if n_bg == 0 and fg_sum < nwg and i["gmm_ms_per_wg_m"] > 0 and cw[last] < mcw:
            got.add("greedy: stops at the scoring cut-off")
        if n_bg == 0 and fg_sum == nwg:
            got.add("greedy: the full grid")
        if i["plan_min_cw"] > nwg // n_work:
            got.add("greedy: plan_min_cw above nwg / n_work")
        if n_bg > 0 and fg_sum == nwg and all(cw[k] == 1 for k in range(n_work, n_work + n_bg)):
            got.add("background, greedy: a spare of 0")
    if n_bg > 0:
        mode = "bisection" if i["plan_mode"] == 0 else "greedy"
        if n_bg == 1:
            got.add("background, %s: n_bg 1" % mode)
        if n_bg == nwg_all // 4:
            got.add("background, %s: n_bg nwg_all / 4" % mode)
        if i["fg_cw_cap"] < i["max_cw"] and any(cw[k] == i["fg_cw_cap"] for k in range(n_work)):
            got.add("background, %s: fg_cw_cap binds" % mode)
    if i["xl_ok"] and nwg_all % 8 == 0:
        packed = {idx: c for idx, _, c, _ in o["items"]}
        if o["xl"]:
            got.add("packing: accepted")
            if any(packed[k] > cw[k] for k in cw):
                got.add("packing: left-over room to the latest finisher")
        elif i["xl_slack_m"] == 1000 and max(cw.values()) > nwg_all // 8:
            got.add("packing: rejected by xl_slack")
    else:
        got.add("packing: skipped, nwg_all & 7" if i["xl_ok"] else "packing: skipped, xl_ok off")
    if o["rebalance_at"] > 0:
        got.add("re-plan: on")
    elif i["rebalance"]:
        if n_work < 4:
            got.add("re-plan: off, n_work < 4")
        elif n_bg > 0 and not i["bg_rebalance"]:
            got.add("re-plan: off, background")
        else:
            got.add("re-plan: off, rebalance_min_us")
    return got


BRANCHES = [
    "uniform: no weights", "uniform: weighted off", "uniform: one stream, no background", "uniform: max_cw 1", "uniform: nwg < 2 n_work",
    "uniform: XCD-local", "uniform: not XCD-local",
    "bisection: equal weights", "bisection: one stream ten times longer", "bisection: weights of 0 and below 1",
    "bisection: every want above the cap", "bisection: overshoot trim", "bisection: remainder passes go round more than once",
    "greedy: stops at mcw", "greedy: stops at the scoring cut-off", "greedy: the full grid", "greedy: plan_min_cw above nwg / n_work",
    "background, bisection: n_bg 1", "background, bisection: n_bg nwg_all / 4", "background, bisection: fg_cw_cap binds",
    "background, greedy: n_bg 1", "background, greedy: n_bg nwg_all / 4", "background, greedy: fg_cw_cap binds", "background, greedy: a spare of 0",
    "packing: accepted", "packing: rejected by xl_slack", "packing: skipped, nwg_all & 7", "packing: skipped, xl_ok off",
    "packing: left-over room to the latest finisher",
    "re-plan: on", "re-plan: off, n_work < 4", "re-plan: off, background", "re-plan: off, rebalance_min_us",
]


def test_plan_cases_reach_every_branch(plans):
    count = {b: 0 for b in BRANCHES}
    for name, i, _, o, plain in plans:
        for b in _branches(name, i, o, plain):
            count[b] += 1
    assert [b for b in BRANCHES if count[b] == 0] == []
    assert {i["nwg_all"] for _, i, _, _, _ in plans} == {8, 16, 64, 250, 256, 248}
