"""The geometry of the resident search kernels (juicer_amd/csrc/jd_plan.h: plan_resident) on the CPU: tests/res_plan_driver.cpp, compiled
with plain g++, is held to tests/golden/res_plan_golden.json - what the lines of jd_res_start that plan_resident replaced made of the same
inputs, recorded from the commit named in the file - integer by integer and verdict by verdict, and every plan that is ok is checked for
what a legal one is.
"""
import json
import os
import re
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "juicer_amd", "csrc")
IN = ["n_cus", "n_streams", "rows_per_buf", "max_cw", "cap_slots", "cap_items", "pipeline", "free_cus", "slot", "xl", "keep_se"]
CONSTS = ["SW", "WG_PER_CU", "SLOT_WG_PER_CU", "GMM_ROWS2", "RES_RING_W"]
OUT = ["rows", "Cw", "slot", "xl", "park_cus", "park_fill"]
VERDICTS = ["ok", "limits", "clusters", "slots"]                       # (ResPlanVerdict, in its order)


@pytest.fixture(scope="module")
def plans(tmp_path_factory):
    """(the build's constants as recorded, [(name, input, golden output, output)])"""
    gxx = shutil.which("g++")
    assert gxx, "g++ not found"
    driver = str(tmp_path_factory.mktemp("res_plan") / "res_plan_driver")
    subprocess.check_call([gxx, "-std=c++17", "-Wall", "-Werror", "-I", CSRC, "-o", driver, os.path.join(HERE, "res_plan_driver.cpp")])
    with open(os.path.join(HERE, "golden", "res_plan_golden.json")) as f:
        doc = json.load(f)
    assert re.fullmatch(r"[0-9a-f]{7,40}", doc["commit"])
    inputs = [dict(doc["defaults"], **c["in"]) for c in doc["cases"]]
    text = "%d\n" % len(inputs) + "\n".join(" ".join(str(x) for x in [i[k] for k in IN] + [doc["consts"][k] for k in CONSTS]) for i in inputs) + "\n"
    lines = subprocess.run([driver], input=text, capture_output=True, text=True, check=True).stdout.splitlines()
    assert len(lines) == len(inputs)
    outs = []
    for l in lines:
        o = [int(x) for x in l.split()]
        assert len(o) == 1 + len(OUT)
        outs.append(dict({"verdict": VERDICTS[o[0]]}, **dict(zip(OUT, o[1:]))))
    return doc["consts"], [(c["name"], i, c["out"], o) for c, i, o in zip(doc["cases"], inputs, outs)]


def test_res_plan_matches_recorded(plans):
    _, cases = plans
    assert len(cases) >= 60
    bad = [name for name, _, want, got in cases if want != got]
    for name, _, want, got in cases:
        if want != got:
            print(name, "recorded", want, "now", got)
    assert not bad


def test_res_plan_is_legal(plans):
    _, cases = plans
    n_ok = 0
    for name, i, _, o in cases:
        if o["verdict"] != "ok":
            continue
        n_ok += 1
        assert 1 <= o["Cw"] <= i["max_cw"], name
        assert not o["slot"] or o["Cw"] == 1, name
        assert not o["xl"] or o["Cw"] == 1, name
        assert o["park_cus"] % 32 == 0 and 0 <= o["park_cus"] < i["n_cus"], name
        assert o["park_fill"] <= i["n_streams"], name
    assert n_ok >= 60


def test_res_plan_constants_are_the_builds(plans):
    """the constants the golden was recorded with are those the kernels are compiled with"""
    consts, _ = plans

    def define(header, name):
        with open(os.path.join(CSRC, header)) as f:
            m = re.search(r"^#define %s (\d+)\b" % name, f.read(), re.M)
        assert m, (header, name)
        return int(m.group(1))

    sw = define("jd_search.h", "SW")
    assert consts == {"SW": sw, "WG_PER_CU": define("jd_search.h", "WG_PER_CU"), "SLOT_WG_PER_CU": define("jd_slot.h", "SLOT_WPE") * 4 // sw,
                      "GMM_ROWS2": define("jd_score_plan.h", "GMM_ROWS2"), "RES_RING_W": define("jd_host_resident.h", "RES_RING_W")}


def test_res_plan_cases_cover_what_they_must(plans):
    consts, cases = plans
    per_cu, tile, ring = consts["SLOT_WG_PER_CU"], consts["GMM_ROWS2"], consts["RES_RING_W"]
    ins = [i for _, i, _, _ in cases]
    outs = {name: o for name, _, _, o in cases}
    seen = set()
    for name, i, _, o in cases:
        n, cus = i["n_streams"], i["n_cus"]
        tiles = 2 * n * ((i["rows_per_buf"] + tile - 1) // tile)
        cw_cap = max(1, min(i["cap_slots"] // (64 * consts["SW"]), i["cap_items"] // (512 * consts["SW"])))
        want = n * 8 // 5
        seen.add("verdict " + o["verdict"])
        seen.add("n_cus %d" % cus)
        seen.add("n_streams 1" if n == 1 else "n_streams 1024" if n == 1024 else "n_streams 1025" if n == 1025 else "")
        seen.add("slots fill the device" if n == cus * per_cu else "one slot too many" if n == cus * per_cu + 1 else "")
        seen.add("ring met exactly" if tiles == ring and n <= 1024 else "ring one tile over" if tiles == ring + 2 * n and n <= 1024 else "")
        seen.add("cw_cap below max_cw" if cw_cap < i["max_cw"] else "cw_cap above max_cw" if cw_cap > i["max_cw"] else "")
        if i["free_cus"] == -1:
            seen.add("free_cus lower clamp" if want < cus // 4 else "free_cus upper clamp" if want > cus // 2 else "free_cus between")
        if i["pipeline"] and n <= 4 and cus >= 64:
            assert o["Cw"] == 1, name
            seen.add("pipeline, few streams")
        for k in ("free_cus", "slot", "xl", "keep_se"):
            if i[k] == -1:
                seen.add(k + " unset")
        seen.add("free_cus %s range" % ("in" if 0 <= i["free_cus"] < cus else "out of") if i["free_cus"] != -1 else "")
        for k in ("slot", "xl"):
            seen.add("%s %s range" % (k, "in" if i[k] in (0, 1) else "out of") if i[k] != -1 else "")
        if i["keep_se"] != -1:
            in_range = 1 <= i["keep_se"] <= max(1, cus // 32)
            seen.add("keep_se in range" if in_range else "keep_se out of range")
            if in_range and o["slot"] and i["keep_se"] * 32 * per_cu < n:
                assert o["park_cus"] == 0, name
                seen.add("keep_se refused")
    want = ["verdict " + v for v in VERDICTS] + ["n_cus %d" % c for c in (256, 304, 64, 8)] + [
        "n_streams 1", "n_streams 1024", "n_streams 1025", "slots fill the device", "one slot too many", "ring met exactly", "ring one tile over",
        "cw_cap below max_cw", "cw_cap above max_cw", "free_cus lower clamp", "free_cus between", "free_cus upper clamp", "pipeline, few streams",
        "keep_se refused"] + ["%s %s" % (k, w) for k in ("free_cus", "slot", "xl", "keep_se") for w in ("unset", "in range", "out of range")]
    assert [w for w in want if w not in seen] == []
    for cus in (256, 304, 64, 8):                                      # the residency bound, at the bound and one above, on every chip
        assert outs["slots_fill_device_%d" % cus]["verdict"] == "ok" and outs["slots_one_too_many_%d" % cus]["verdict"] == "slots"
    assert any(i["n_streams"] == 1024 and o["verdict"] == "ok" for _, i, _, o in cases)
    assert all(o["verdict"] == "limits" for _, i, _, o in cases if i["n_streams"] == 1025)
    assert len(ins) == len({json.dumps(i, sort_keys=True) for i in ins})   # no case twice
