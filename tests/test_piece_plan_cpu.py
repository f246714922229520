"""The rows of a scoring piece of the batch pipeline (juicer_amd/csrc/jd_plan.h: plan_piece_rows) and the scoring workgroups resident
beside the slots (plan_resident_scoring_wgs) on the CPU: tests/piece_plan_driver.cpp, compiled with plain g++ - and once more with the
address and undefined-behaviour sanitizers - against a brute-force restatement.
"""
import os
import random
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "juicer_amd", "csrc")
TILE = 128


def build(tmp, name, extra=()):
    gxx = shutil.which("g++")
    assert gxx, "g++ not found"
    exe = str(tmp / name)
    subprocess.check_call([gxx, "-std=c++17", "-Wall", "-Werror", "-g", *extra, "-I", CSRC, "-o", exe, os.path.join(HERE, "piece_plan_driver.cpp")])
    return exe


def run(exe, cases):
    text = "%d\n" % len(cases) + "\n".join("%s %d %d %d %d" % c for c in cases) + "\n"
    out = subprocess.run([exe], input=text, capture_output=True, text=True, check=True).stdout.split()
    assert len(out) == len(cases)
    return [int(x) for x in out]


def waste(rows, groups, wgs):
    """workgroup places of the piece's last round that stay empty"""
    return -(rows // TILE * groups) % wgs


def piece_cases():
    rng = random.Random(5)
    cases = [("p", 47, 512, 4096, 8192), ("p", 47, 512, 6144, 6144), ("p", 1, 512, 4096, 8192), ("p", 188, 512, 4096, 8192),
             ("p", 47, 1024, 4096, 8192), ("p", 47, 1, 4096, 8192), ("p", 3, 7, 128, 128), ("p", 47, 512, 4000, 8300),
             ("p", 64, 512, 128, 16384), ("p", 5, 512, 130, 250)]
    for _ in range(300):
        lo = rng.randrange(1, 9000)
        cases.append(("p", rng.randrange(1, 200), rng.randrange(1, 1300), lo, lo + rng.randrange(0, 9000)))
    return cases


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    return build(tmp_path_factory.mktemp("piece_plan"), "piece_plan_driver")


def test_piece_rows_are_legal_and_waste_least(driver):
    cases = piece_cases()
    for (_, groups, wgs, lo, hi), rows in zip(cases, run(driver, cases)):
        what = (groups, wgs, lo, hi, rows)
        t_lo, t_hi = max(1, -(-lo // TILE)), max(1, hi // TILE)
        t_hi = max(t_hi, t_lo)                                         # (no whole tile inside the bounds: the first one above lo)
        assert rows % TILE == 0 and t_lo * TILE <= rows <= t_hi * TILE, what
        if lo <= hi and -(-lo // TILE) <= hi // TILE:
            assert lo <= rows <= hi, what
        best = min(range(t_lo, t_hi + 1), key=lambda t: (waste(t * TILE, groups, wgs), t))   # least waste, then the smaller piece
        assert rows == best * TILE, what + (best * TILE,)


def test_piece_rows_of_the_headline(driver):
    """configs[1]: 47 groups of 64 states, two scoring workgroups beside the slot of each of 256 CUs.  6144 rows are 2256 tiles, 4.41
    rounds of 512 with 304 places of the fifth empty; 6912 rows are 2538 tiles, 22 places short of five full rounds."""
    rows, wgs = run(driver, [("p", 47, 512, 4096, 8192), ("w", 256, 256, 2, 4)])
    assert wgs == 512
    assert rows == 6912 and waste(rows, 47, 512) == 22 and waste(6144, 47, 512) == 304
    assert all(waste(r, 47, 512) >= 22 for r in range(4096, 8193, TILE))


def test_resident_scoring_workgroups(driver):
    cases = [("w", 256, 256, 2, 4), ("w", 256, 4, 2, 4), ("w", 256, 0, 2, 4), ("w", 256, 512, 2, 4), ("w", 256, 300, 2, 4),
             ("w", 256, 256, 2, 3), ("w", 8, 3, 2, 8), ("w", 256, 600, 2, 4), ("w", 0, 4, 2, 4), ("w", 256, 4, 0, 4)]
    want = [512, 4 * 2 + 252 * 4, 1024, 1, 44 * 0 + 212 * 2, 256, 3 * 4 + 5 * 8, 1, 1, 1]
    assert run(driver, cases) == want


def test_driver_under_sanitizers(tmp_path):
    """the same cases with -fsanitize=address,undefined: one run, the same answers, nothing reported"""
    exe = build(tmp_path, "piece_plan_driver_san", ("-fsanitize=address,undefined", "-fno-sanitize-recover=all"))
    cases = piece_cases() + [("w", 256, 256, 2, 4), ("w", 1, 2000000000, 1, 2000000000), ("p", 2000000, 1, 2000000000, 2147483647)]
    plain = run(build(tmp_path, "piece_plan_driver_plain"), cases)
    assert run(exe, cases) == plain
