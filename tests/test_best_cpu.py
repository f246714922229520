"""The current best hypothesis of live streams, as far as it can be held without a device: the decisions of juicer_amd/csrc/jd_best.h
(the request, k_best_many's buffer layout, what a reply means, the argument check, taking a list from the staging area or from the
result arrays, the word projection) through tests/best_driver.cpp - compiled with plain g++, and once more with
-fsanitize=address,undefined - against the same rules restated here; the C ABI's new entry points; and jd_best's layout in the
header against its ctypes mirror."""
import ctypes as C
import os
import shutil
import struct
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "juicer_amd", "csrc")
INCLUDE = os.path.join(ROOT, "include")

HEAD, FIELDS, SHARE = 12, 6, 64
NOT_FOUND, TOO_LONG, FROM_STAGE, FROM_RESULTS = range(4)
ARG_OK, ARG_BAD_STREAM, ARG_NOT_STARTED, ARG_RESIDENT = range(4)


def fbits(x):
    return struct.unpack("<i", struct.pack("<f", float(x)))[0]


def build_driver(path, extra=()):
    gxx = shutil.which("g++")
    assert gxx, "g++ not found"
    subprocess.check_call([gxx, "-std=c++17", "-Wall", "-Werror", *extra, "-I", CSRC, "-I", INCLUDE, "-o", path, os.path.join(HERE, "best_driver.cpp")])
    return path


def run_driver(driver, lines):
    out = subprocess.run([driver], input="\n".join(lines) + "\n", capture_output=True, text=True, check=True).stdout.splitlines()
    assert len(out) == len(lines)
    return [[int(x) for x in l.split()] for l in out]


def expect_lists(n, cap, labels, with_models=True):
    """what `stage` / `rows` print for records k = 0 .. n-1"""
    k = min(cap, n)
    out = [n] + [(100 + i) if with_models else 0 for i in range(k)] + labels[:k] + [200 + i for i in range(k)]
    for base in (300.0, 400.0, 500.0):
        out += [fbits(base + i) for i in range(k)]
    w = [i for i in range(n) if labels[i] != 0]
    kw = w[:min(cap, len(w))]
    out += [len(w)] + [labels[i] for i in kw] + [200 + i for i in kw]
    for base in (300.0, 400.0, 500.0):
        out += [fbits(base + i) for i in kw]
    return out


def cases():
    """[(line, expected output)]"""
    cs = []
    for s in (0, 3, 1023):
        cs.append(("request %d" % s, [s, 0, 0, 0]))
    for M, n, i in ((1, 1, 0), (4, 4, 3), (16, 5, 2), (1024, 1024, 1023)):
        per = HEAD + FIELDS * SHARE
        cs.append(("layout %d %d %d" % (M, n, i), [4 * M, per, 4 * M + per * M, per * n, HEAD * n + FIELDS * SHARE * i, HEAD, FIELDS, SHARE]))
        assert HEAD * n + FIELDS * SHARE * (i + 1) <= per * n          # (entry i's share ends inside what a launch of n entries writes)
    for found, n, cap, want in ((0, 0, 8192, NOT_FOUND), (0, 99999, 16, NOT_FOUND), (1, 0, 8192, FROM_STAGE), (1, 64, 8192, FROM_STAGE),
                                (1, 65, 8192, FROM_RESULTS), (1, 8192, 8192, FROM_RESULTS), (1, 8193, 8192, TOO_LONG), (1, 17, 16, TOO_LONG),
                                (1, 16, 16, FROM_STAGE), (1, 64, 32, TOO_LONG)):
        cs.append(("reply %d %d %d" % (found, n, cap), [want]))
    cs.append(("none 137", [0, 137, 0, 0, 0, 0, 0, 0, 0]))
    # check: M streams as (started, T, resident), then the list
    S3 = "3 1 10 0 1 0 0 0 0 0"                                        # stream 0 at frame 10, stream 1 begun, stream 2 not begun
    cs.append(("check %s 2 0 1" % S3, [ARG_OK, -1, 1, 0, 0]))
    cs.append(("check %s 2 1 0" % S3, [ARG_OK, -1, 1, 0, 1]))
    cs.append(("check %s 0" % S3, [ARG_OK, -1, 0]))
    cs.append(("check %s 2 0 0" % S3, [ARG_BAD_STREAM, 0, 1, 0, 0]))
    cs.append(("check %s 1 3" % S3, [ARG_BAD_STREAM, 3, 0]))
    cs.append(("check %s 1 -1" % S3, [ARG_BAD_STREAM, -1, 0]))
    cs.append(("check %s 2 0 2" % S3, [ARG_NOT_STARTED, 2, 1, 0, 0]))
    cs.append(("check 2 1 10 0 1 20 1 2 0 1", [ARG_RESIDENT, 1, 2, 0, 1, 0, 1]))
    for n, cap, labels in ((0, 4, []), (1, 4, [7]), (5, 5, [0, 3, 0, 0, 9]), (5, 2, [0, 3, 4, 0, 9]), (5, 0, [1, 2, 3, 4, 5]), (64, 64, [k % 3 for k in range(64)]),
                           (64, 100, [0] * 64), (7, 3, [0, 0, 0, 0, 5, 6, 7])):
        lab = " ".join(str(l) for l in labels)
        cs.append((("stage %d %d %s" % (n, cap, lab)).strip(), expect_lists(n, cap, labels)))
        cs.append((("rows %d %d 1 %s" % (n, cap, lab)).strip(), expect_lists(n, cap, labels)))
        cs.append((("rows %d %d 0 %s" % (n, cap, lab)).strip(), expect_lists(n, cap, labels, with_models=False)))
    cs.append(("rows 200 200 1 " + " ".join(str(k % 5) for k in range(200)), expect_lists(200, 200, [k % 5 for k in range(200)])))
    # a stream's record: the list is empty from init on; begin() marks the utterance as the resident kernel's, init() and a batch unmark it
    cs.append(("life", [5, 0, 0, 0, 5, 1, 5, 0, 0, 0, 0, 0]))
    return cs


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    return build_driver(str(tmp_path_factory.mktemp("best") / "best_driver"))


def test_driver_cases(driver):
    cs = cases()
    assert len({l for l, _ in cs}) == len(cs) >= 50
    out = run_driver(driver, [l for l, _ in cs])
    for (line, want), got in zip(cs, out):
        assert got == want, line


def test_driver_under_sanitizers(driver, tmp_path_factory):
    """every line once more through the driver built with -fsanitize=address,undefined, as a stand-alone program: the same output,
    nothing reported"""
    san = build_driver(str(tmp_path_factory.mktemp("best_san") / "best_driver_san"), ("-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"))
    lines = [l for l, _ in cases()]
    assert run_driver(san, lines) == run_driver(driver, lines)


@pytest.mark.parametrize("sym", ["jd_streams_best", "jd_stream_best_words", "jd_stream_best_models", "jd_dec_best_stats"])
def test_new_symbols_resolve(built, sym):
    from juicer_amd import capi
    assert sym in capi.EXPORTS
    assert hasattr(capi.lib(), sym)


def test_null_handles_and_bad_arguments_are_refused_with_a_message(built):
    from juicer_amd import capi
    L = capi.lib()
    n = C.c_int32(0)
    a, b = C.c_int64(0), C.c_int64(0)
    s = (C.c_int32 * 1)(0)
    out = (capi.CBest * 1)()
    nul = [None] * 6
    calls = (("jd_streams_best", lambda: L.jd_streams_best(None, C.c_int32(1), s, out)),
             ("jd_streams_best", lambda: L.jd_streams_best(None, C.c_int32(0), None, None)),
             ("jd_streams_best", lambda: L.jd_streams_best(None, C.c_int32(-1), s, out)),
             ("jd_stream_best_words", lambda: L.jd_stream_best_words(None, C.c_int32(0), C.c_int32(0), C.byref(n), *nul[:5])),
             ("jd_stream_best_models", lambda: L.jd_stream_best_models(None, C.c_int32(0), C.c_int32(0), C.byref(n), *nul)),
             ("jd_dec_best_stats", lambda: L.jd_dec_best_stats(None, C.byref(a), C.byref(b))))
    for what, call in calls:
        assert call() == capi.JD_EINVAL, what
        assert what in L.jd_last_error().decode(), what


def test_jd_best_layout_header_against_ctypes(tmp_path):
    """sizeof(jd_best) and the offset of every field: a C program compiled against the header, and the ctypes mirror"""
    from juicer_amd import capi
    cc = shutil.which("gcc") or shutil.which("cc")
    assert cc, "no C compiler"
    names = [f for f, _ in capi.CBest._fields_]
    assert names == ["found", "frame", "n_words", "n_records", "model", "state", "score", "ac", "lm"]
    src = tmp_path / "layout.c"
    src.write_text("#include <stddef.h>\n#include <stdio.h>\n#include \"juicer_amd.h\"\nint main(void)\n{\n    printf(\"%zu\", sizeof(jd_best));\n"
                   + "".join("    printf(\" %%zu\", offsetof(jd_best, %s));\n" % f for f in names) + "    printf(\"\\n\");\n    return 0;\n}\n")
    exe = tmp_path / "layout"
    subprocess.check_call([cc, "-std=c99", "-Wall", "-Werror", "-I", INCLUDE, "-o", str(exe), str(src)])
    got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert got == [C.sizeof(capi.CBest)] + [getattr(capi.CBest, f).offset for f in names] == [36] + [4 * k for k in range(9)]
