"""The plan of a scoring launch (juicer_amd/csrc/jd_score_plan.h) on the CPU: tests/score_plan_driver.cpp, compiled with plain g++, is held to
tests/golden/score_plan_golden.json - the kernel, grid, dynamic LDS and tile rows that the lines of launch_gmm, gmm_tiles128_occupancy and
score_tile_rows which jd_score_plan.h replaced made of the same inputs, recorded from the commit named in the file - integer by integer;
the same plans are checked for what a legal plan is; and the plan is held to the Python transcription of the rule that
tests/test_gpu_score_rows.py holds the device's own report to (tests/score_rows_cases.py).

Two things read as the code has them, not as a literal rule would:
- jd_hybrid_kernel's grid is one thread per cell whatever max_blocks says (launch_gmm never bounded it; score_rows_cases' case
  "c_max_blocks_ignored" is the device-side witness), so "grid <= max_blocks" is asserted of every other kernel and the hybrid grid
  is held to ceil(n_rows G / 256);
- jd_mlp_kernel's dynamic LDS is its network's (jd_mlp.h: jd_mlp_lds_bytes, tests/test_mlp_cpu.py), not the plan's: recorded and planned as 0."""
import json
import os
import re
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
FIELDS = ["model", "D", "G", "hybrid", "mlp", "fast", "n_rows", "max_blocks", "used_row_tiles", "has_list", "n_rt_list"]
OUT = ["verdict", "kernel", "grid", "lds_bytes", "list_tile_rows", "large_kernel", "large_lds_bytes", "tile_rows", "tile_states", "row_tiles", "tiles", "dp"]
OK, NOTHING, LIST_REFUSED = 0, 1, 2
# JD_KERNEL_* (include/juicer_amd.h)
(K_NONE, K_GENERIC, K_GMM39_16, K_GMM39_64, K_FAST39_16, K_FAST39_64, K_FAST_16, K_FAST_64, K_HYBRID, K_MLP) = range(10)
SIBLING_64 = {K_GMM39_16: K_GMM39_64, K_GMM39_64: K_GMM39_64, K_FAST39_16: K_FAST39_64, K_FAST39_64: K_FAST39_64, K_FAST_16: K_FAST_64,
              K_FAST_64: K_FAST_64}
SMALL = (K_GMM39_16, K_FAST39_16, K_FAST_16)
LDS_MAX = 160 * 1024                                       # gfx950: the LDS of a CU


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    gxx = shutil.which("g++")
    assert gxx, "g++ not found"
    exe = str(tmp_path_factory.mktemp("score_plan") / "score_plan_driver")
    subprocess.check_call([gxx, "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "juicer_amd", "csrc"), "-I", os.path.join(ROOT, "include"),
                           "-o", exe, os.path.join(HERE, "score_plan_driver.cpp")])
    return exe


def run(driver, inputs):
    """inputs: dicts of FIELDS[1:] -> dicts of OUT"""
    text = "".join(" ".join(str(i[f]) for f in FIELDS[1:]) + "\n" for i in inputs)
    lines = subprocess.run([driver], input=text, capture_output=True, text=True, check=True).stdout.splitlines()
    assert len(lines) == len(inputs)
    return [dict(zip(OUT, (int(x) for x in l.split()))) for l in lines]


@pytest.fixture(scope="module")
def plans(driver):
    """[(input, recorded out, recorded large, the driver's plan)]"""
    with open(os.path.join(HERE, "golden", "score_plan_golden.json")) as f:
        doc = json.load(f)
    assert re.fullmatch(r"[0-9a-f]{7,40}", doc["commit"]) and "verbatim" in doc["how"] and doc["fields"] == FIELDS
    inputs = [dict(zip(FIELDS, c["in"])) for c in doc["cases"]]
    return [(i, c["out"], c["large"], p) for i, c, p in zip(inputs, doc["cases"], run(driver, inputs))]


def test_plan_matches_recorded(plans):
    bad = []
    for i, want, large, p in plans:
        got = [p[k] for k in OUT[:5]], [p[k] for k in OUT[5:7]]
        if got != (want, large):
            bad.append(i)
            print(i, "recorded", want, large, "now", got)
    assert not bad


def test_recorded_cases_cover_what_they_must(plans):
    ins = [i for i, _, _, _ in plans]
    assert len(ins) >= 1000 and len({tuple(i.values()) for i in ins}) == len(ins)              # no case twice
    assert {want[1] for _, want, _, _ in plans} == set(range(10))                             # every JD_KERNEL_* value, "none" among them
    assert {want[0] for _, want, _, _ in plans} == {OK, NOTHING, LIST_REFUSED}
    # the models are the legal ones: a network's models are hybrid ones, the option is for neither
    assert {(i["model"], i["hybrid"], i["mlp"], i["fast"]) for i in ins} == {("exact", 0, 0, 0), ("fast", 0, 0, 1), ("hybrid", 1, 0, 0), ("mlp", 1, 1, 0)}
    for model in ("exact", "fast"):
        mine = [i for i in ins if i["model"] == model]
        assert {(i["D"], i["G"]) for i in mine} == {(D, G) for D in (13, 39, 40, 65) for G in (1, 16, 17, 64, 65, 150, 3000)}
        for D in (13, 39, 40, 65):
            for G in (1, 16, 17, 64, 65, 150, 3000):
                rows = {i["n_rows"] for i in mine if (i["D"], i["G"]) == (D, G) and not i["has_list"] and i["used_row_tiles"] < 0 and not i["max_blocks"]}
                edge = -(-1024 // -(-G // 64))                                                # row tiles: one less stays below 1024 tiles of 64 states
                assert {0, 1, 15, 16, 17, 63, 64, 65, 127, 128, 129, (edge - 1) * 128, edge * 128, (edge + 1) * 128} <= rows, (model, D, G)
    for model in ("hybrid", "mlp"):
        assert {i["G"] for i in ins if i["model"] == model} == {1, 16, 17, 64, 65, 150, 3000}
        assert {0, 1, 15, 16, 17, 129} <= {i["n_rows"] for i in ins if i["model"] == model}
    # the boundary by name: G = 64 at 1023 / 1024 / 1025 row tiles, G = 150 (three state groups) at 341 / 342
    for G, tiles in ((64, (1023, 1024, 1025)), (150, (341, 342))):
        for D in (39, 40):
            assert set(tiles) <= {i["n_rows"] // 128 for i in ins if (i["D"], i["G"], i["model"]) == (D, G, "fast") and i["n_rows"] % 128 == 0}
            assert {-1, 0} | set(tiles[:2]) <= {i["used_row_tiles"] for i in ins if (i["D"], i["G"], i["n_rows"]) == (D, G, 17)}
            assert set(tiles[:2]) <= {i["n_rt_list"] for i in ins if (i["D"], i["G"]) == (D, G) and i["has_list"]}
    # bounded grids: 1 and either side of the tiles; the refusal: the generic kernel with a list
    for i, want, _, p in plans:
        if i["max_blocks"] == 0 and want[0] == OK and i["G"] == 150 and i["D"] in (39, 40) and i["n_rows"] == 129 and i["used_row_tiles"] < 0:
            mbs = {j["max_blocks"] for j in ins if {k: v for k, v in j.items() if k != "max_blocks"} == {k: v for k, v in i.items() if k != "max_blocks"}}
            assert {0, 1, want[2] - 1, want[2], want[2] + 1} <= mbs, i
    assert {i["D"] for i, want, _, _ in plans if want[0] == LIST_REFUSED} == {13, 40, 65}
    assert all(i["model"] == "exact" and i["has_list"] for i, want, _, _ in plans if want[0] == LIST_REFUSED)


def test_plans_are_legal(plans):
    for i, _, _, p in plans:
        G, mb = i["G"], i["max_blocks"]
        assert p["lds_bytes"] <= LDS_MAX and p["large_lds_bytes"] <= LDS_MAX
        # the large-launch query: the 64-state sibling of what is planned, whatever the rows; none for the other kernels
        if p["verdict"] == OK:
            assert p["large_kernel"] == SIBLING_64.get(p["kernel"], K_NONE), i
            if p["large_kernel"]:
                assert p["large_lds_bytes"] == p["lds_bytes"]
        if p["verdict"] != OK:
            assert (p["verdict"] == NOTHING) == (i["n_rows"] <= 0)
            assert [p[k] for k in ("kernel", "grid", "lds_bytes", "tiles")] == [K_NONE, 0, 0, 0], i
            continue
        assert p["grid"] >= 1, i
        if mb == 0:
            assert p["grid"] == p["tiles"], i
        if p["kernel"] == K_HYBRID:
            assert p["grid"] == -(-i["n_rows"] * G // 256) and (p["tile_rows"], p["tile_states"], p["list_tile_rows"]) == (0, 0, 0), i
            continue
        if mb > 0:
            assert p["grid"] == min(mb, p["tiles"]) <= mb, i
        if p["kernel"] == K_MLP:
            assert (p["tile_rows"], p["tile_states"], p["list_tile_rows"]) == (16, 0, 0) and p["tiles"] == -(-i["n_rows"] // 16), i
            continue
        # the GMM kernels: row tiles x state groups; 16-state tiles exactly when the 64-state tiles are fewer than 1024
        assert p["tile_rows"] == p["list_tile_rows"] == (64 if p["kernel"] == K_GENERIC else 128), i
        row_tiles = i["n_rt_list"] if i["has_list"] else -(-i["n_rows"] // p["tile_rows"])
        assert p["row_tiles"] == row_tiles and p["tiles"] == row_tiles * -(-G // p["tile_states"]), i
        if p["kernel"] == K_GENERIC:
            assert p["tile_states"] == 64 and not i["has_list"] and p["dp"] == i["D"] | 1, i
        else:
            n64 = (i["used_row_tiles"] if i["used_row_tiles"] >= 0 else row_tiles) * -(-G // 64)
            assert (p["tile_states"] == 16) == (p["kernel"] in SMALL) == (n64 < 1024) and p["tile_states"] in (16, 64), i
        if p["kernel"] in (K_FAST_16, K_FAST_64):
            assert p["dp"] == -(-i["D"] // 8) * 8, i


def test_plan_agrees_with_the_score_rows_cases(built, driver):
    """the Python transcription (score_rows_cases: Case.kernel, Case.grid(), TILE_ROWS), which tests/test_gpu_score_rows.py holds the
    device's reported kernel and grid to, says what the plan says"""
    import score_rows_cases as sc
    ins = []
    for c in sc.CASES:
        m = sc.model(c.model_key)
        ins.append({"D": m.D, "G": m.G, "hybrid": int(m.kind == "hybrid"), "mlp": 0, "fast": int(c.mode == sc.SCORE_FAST), "n_rows": c.n_rows,
                    "max_blocks": c.max_blocks, "used_row_tiles": c.used_row_tiles, "has_list": int(c.rt_base is not None),
                    "n_rt_list": 0 if c.rt_base is None else len(c.rt_base)})
    assert len(ins) >= 100
    for c, p in zip(sc.CASES, run(driver, ins)):
        assert (p["verdict"], p["kernel"], p["grid"], p["tile_rows"], p["list_tile_rows"]) == (OK, c.kernel, c.grid(), sc.TILE_ROWS[c.kernel], c.h), c.id
        if c.kernel in sc.TILE_STATES:
            assert p["tile_states"] == sc.TILE_STATES[c.kernel], c.id
