"""The end-of-utterance view (jd_streams_final) and the model-level traces for many streams (jd_streams_trace_models), as far as they
can be held without a device: the decisions of juicer_amd/csrc/jd_final.h and the model-trace functions of jd_push.h through
tests/final_driver.cpp - compiled with plain g++, and once more with -fsanitize=address,undefined as a stand-alone program - against
the same rules restated here; the C ABI's new entry points; and jd_final's layout in the header against its ctypes mirror."""
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

HEAD, FIELDS, SHARE, THREADS = 8, 6, 64, 256
NOT_FOUND, TOO_LONG, FROM_STAGE, FROM_RESULTS = range(4)
ARG_OK, ARG_BAD_STREAM, ARG_NOT_STARTED, ARG_RESIDENT = range(4)
# the model traces: PARTIAL_SHARE new words, and the model records they bring at DESIGN.md section 7's 59 : 17, rounded up to a multiple of 16
W_SHARE, PM_HEAD = 32, 4
PM_SHARE = -(-(-(-W_SHARE * 59 // 17)) // 4) * 4                  # (ceil(32 * 59 / 17) = 112 records: every field 448 bytes, a multiple of 16)
PM_NOT_FOUND, PM_TOO_LONG, PM_FROM_STAGE, PM_FROM_ARRAYS = range(4)
NEW_SYMBOLS = ["jd_streams_final", "jd_stream_final_words", "jd_stream_final_models", "jd_dec_final_stats", "jd_streams_trace_models"]


def fbits(x):
    return struct.unpack("<i", struct.pack("<f", float(x)))[0]


def build_driver(path, extra=()):
    gxx = shutil.which("g++")
    assert gxx, "g++ not found"
    subprocess.check_call([gxx, "-std=c++17", "-Wall", "-Werror", *extra, "-I", CSRC, "-I", INCLUDE, "-o", path, os.path.join(HERE, "final_driver.cpp")])
    return path


def run_driver(driver, lines):
    out = subprocess.run([driver], input="\n".join(lines) + "\n", capture_output=True, text=True, check=True).stdout.splitlines()
    assert len(out) == len(lines)
    return [[int(x) for x in l.split()] for l in out]


def expect_lists(n, cap, labels, with_models=True):
    """what `stage` / `rows` print for records k = 0 .. n-1: the list, then its word projection whose NEWEST entry carries the totals"""
    k = min(cap, n)
    out = [n] + [(100 + i) if with_models else 0 for i in range(k)] + labels[:k] + [200 + i for i in range(k)]
    for base in (300.0, 400.0, 500.0):
        out += [fbits(base + i) for i in range(k)]
    w = [i for i in range(n) if labels[i] != 0]
    kw = w[:min(cap, len(w))]
    out += [len(w)] + [labels[i] for i in kw] + [200 + i for i in kw]
    for base, tot in ((300.0, 7.0), (400.0, 8.0), (500.0, 9.0)):
        col = [fbits(base + i) for i in kw]
        if w and len(w) <= cap:
            col[-1] = fbits(tot)
        out += col
    return out


def pm_words(have, n, have_m, nm):
    """what `pm_take` / `pm_arrays` print: the word list, then the model list record by record"""
    out = [n]
    for k in range(n):
        out += [10 + k, 20 + k]
    out.append(nm)
    for k in range(nm):
        out += [k, 1000 + k, 2000 + k, fbits(3000 + k), fbits(4000 + k), fbits(5000 + k)]
    return out


def cases():
    """[(line, expected output)]"""
    assert PM_SHARE == 112
    cs = []
    for s in (0, 3, 1023):
        cs.append(("request %d" % s, [s, 0, 0, 0]))
    per = HEAD + FIELDS * SHARE
    pm_stage = 2 * W_SHARE + FIELDS * PM_SHARE
    pm_per = PM_HEAD + pm_stage
    for M, n, i in ((1, 1, 0), (4, 4, 3), (16, 5, 2), (1024, 1024, 1023)):
        cs.append(("layout %d %d %d" % (M, n, i), [4 * M, per, 4 * M + per * M, per * n, HEAD * n + FIELDS * SHARE * i, HEAD, FIELDS, SHARE, THREADS]))
        assert HEAD * n + FIELDS * SHARE * (i + 1) <= per * n          # (entry i's share ends inside what a launch of n entries writes)
        cs.append(("pm_layout %d %d %d" % (M, n, i), [4 * M, pm_per, 4 * M + pm_per * M, pm_per * n, PM_HEAD * n + pm_stage * i, 2 * W_SHARE,
                                                       2 * W_SHARE + FIELDS * PM_SHARE - 1, PM_HEAD, PM_SHARE, M * 6 * 100]))
        assert PM_HEAD * n + pm_stage * (i + 1) <= pm_per * n
    # n_records = 0, share, share + 1, res_cap, res_cap + 1
    for found, n, cap, want in ((0, 0, 8192, NOT_FOUND), (0, 99999, 16, NOT_FOUND), (1, 0, 8192, FROM_STAGE), (1, 64, 8192, FROM_STAGE),
                                (1, 65, 8192, FROM_RESULTS), (1, 8192, 8192, FROM_RESULTS), (1, 8193, 8192, TOO_LONG), (1, 17, 16, TOO_LONG),
                                (1, 16, 16, FROM_STAGE), (1, 64, 32, TOO_LONG), (1, 0, 16, FROM_STAGE)):
        cs.append(("reply %d %d %d" % (found, n, cap), [want]))
    cs.append(("none 137", [0, 137, 0, 0, 0, 0, 0]))
    # check: M streams as (started, T, resident), then the list - the four verdicts
    S3 = "3 1 10 0 1 0 0 0 0 0"                                        # stream 0 at frame 10, stream 1 begun, stream 2 not begun
    cs.append(("check %s 2 0 1" % S3, [ARG_OK, -1, 1, 0, 0]))
    cs.append(("check %s 2 1 0" % S3, [ARG_OK, -1, 1, 0, 1]))
    cs.append(("check %s 0" % S3, [ARG_OK, -1, 0]))
    cs.append(("check %s 2 0 0" % S3, [ARG_BAD_STREAM, 0, 1, 0, 0]))
    cs.append(("check %s 1 3" % S3, [ARG_BAD_STREAM, 3, 0]))
    cs.append(("check %s 1 -1" % S3, [ARG_BAD_STREAM, -1, 0]))
    cs.append(("check %s 2 0 2" % S3, [ARG_NOT_STARTED, 2, 1, 0, 0]))
    cs.append(("check 2 1 10 0 1 20 1 2 0 1", [ARG_RESIDENT, 1, 2, 0, 1, 0, 1]))
    for n, cap, labels in ((0, 4, []), (1, 4, [7]), (5, 5, [0, 3, 0, 0, 9]), (5, 5, [0, 3, 0, 9, 0]), (5, 2, [0, 3, 4, 0, 9]), (5, 0, [1, 2, 3, 4, 5]),
                           (64, 64, [k % 3 for k in range(64)]), (64, 100, [0] * 64), (7, 3, [0, 0, 0, 0, 5, 6, 7])):
        lab = " ".join(str(l) for l in labels)
        cs.append((("stage %d %d %s" % (n, cap, lab)).strip(), expect_lists(n, cap, labels)))
        cs.append((("rows %d %d 1 %s" % (n, cap, lab)).strip(), expect_lists(n, cap, labels)))
        cs.append((("rows %d %d 0 %s" % (n, cap, lab)).strip(), expect_lists(n, cap, labels, with_models=False)))
    cs.append(("rows 200 200 1 " + " ".join(str(k % 5) for k in range(200)), expect_lists(200, 200, [k % 5 for k in range(200)])))
    cs.append(("life", [5, 6, 0, 0]))
    # the model traces
    cs.append(("pm_request 0 0 0", [5, -1, 0, 0]))
    cs.append(("pm_request 3 11 77", [5, 77, 3, 11]))
    cap = 500
    for found, n, nm, have, have_m, want in (
            (0, 0, 0, 0, 0, PM_NOT_FOUND), (0, 5, 9, 5, 9, PM_NOT_FOUND),
            (1, 1, 1, 0, 0, PM_FROM_STAGE),                            # have / have_m at 0
            (1, 40, 120, 40, 120, PM_FROM_STAGE),                      # ... equal to the new length
            (1, 40, 120, 8, 8, PM_FROM_STAGE),                         # ... one share behind it (32 words, 112 records)
            (1, 40, 120, 7, 8, PM_FROM_ARRAYS), (1, 40, 120, 8, 7, PM_FROM_ARRAYS),   # ... and one more
            (1, 32, 112, 0, 0, PM_FROM_STAGE), (1, 33, 112, 0, 0, PM_FROM_ARRAYS), (1, 32, 113, 0, 0, PM_FROM_ARRAYS),
            (1, cap, cap, cap - 1, cap - 1, PM_FROM_STAGE), (1, cap + 1, cap, cap, cap, PM_TOO_LONG), (1, cap, cap + 1, cap, cap, PM_TOO_LONG),
            (1, 5, 9, 6, 9, PM_FROM_ARRAYS), (1, 5, 9, 5, 10, PM_FROM_ARRAYS)):
        cs.append(("pm_reply %d %d %d %d %d %d" % (found, n, nm, have, have_m, cap), [want]))
    for have, n, have_m, nm in ((0, 0, 0, 0), (0, 1, 0, 1), (0, 32, 0, 112), (3, 3, 7, 7), (8, 40, 8, 120), (5, 6, 100, 101), (2, 2, 4, 9)):
        cs.append(("pm_take %d %d %d %d" % (have, n, have_m, nm), pm_words(have, n, have_m, nm)))
    for n, nm in ((0, 0), (1, 1), (33, 113), (200, 450)):
        cs.append(("pm_arrays %d %d" % (n, nm), pm_words(0, n, 0, nm)))
    return cs


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    return build_driver(str(tmp_path_factory.mktemp("final") / "final_driver"))


def test_driver_cases(driver):
    cs = cases()
    assert len({l for l, _ in cs}) == len(cs) >= 70
    out = run_driver(driver, [l for l, _ in cs])
    for (line, want), got in zip(cs, out):
        assert got == want, line


def test_driver_under_sanitizers(driver, tmp_path_factory):
    """every line once more through the driver built with -fsanitize=address,undefined, as a stand-alone program: the same output,
    nothing reported"""
    san = build_driver(str(tmp_path_factory.mktemp("final_san") / "final_driver_san"), ("-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"))
    lines = [l for l, _ in cases()]
    assert run_driver(san, lines) == run_driver(driver, lines)


@pytest.mark.parametrize("sym", NEW_SYMBOLS)
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
    out = (capi.CFinal * 1)()
    nul = [None] * 6
    calls = (("jd_streams_final", lambda: L.jd_streams_final(None, C.c_int32(1), s, out)),
             ("jd_streams_final", lambda: L.jd_streams_final(None, C.c_int32(0), None, None)),
             ("jd_streams_final", lambda: L.jd_streams_final(None, C.c_int32(-1), s, out)),
             ("jd_stream_final_words", lambda: L.jd_stream_final_words(None, C.c_int32(0), C.c_int32(0), C.byref(n), *nul[:5])),
             ("jd_stream_final_models", lambda: L.jd_stream_final_models(None, C.c_int32(0), C.c_int32(0), C.byref(n), *nul)),
             ("jd_dec_final_stats", lambda: L.jd_dec_final_stats(None, C.byref(a), C.byref(b))),
             ("jd_streams_trace_models", lambda: L.jd_streams_trace_models(None, C.c_int32(1), s, None)),
             ("jd_streams_trace_models", lambda: L.jd_streams_trace_models(None, C.c_int32(-1), s, None)))
    for what, call in calls:
        assert call() == capi.JD_EINVAL, what
        assert what in L.jd_last_error().decode(), what


def test_jd_final_layout_header_against_ctypes(tmp_path):
    """sizeof(jd_final) and the offset of every field: a C program compiled against the header, and the ctypes mirror"""
    from juicer_amd import capi
    cc = shutil.which("gcc") or shutil.which("cc")
    assert cc, "no C compiler"
    names = [f for f, _ in capi.CFinal._fields_]
    assert names == ["found", "frame", "n_words", "n_records", "score", "ac", "lm"]
    src = tmp_path / "layout.c"
    src.write_text("#include <stddef.h>\n#include <stdio.h>\n#include \"juicer_amd.h\"\nint main(void)\n{\n    printf(\"%zu\", sizeof(jd_final));\n"
                   + "".join("    printf(\" %%zu\", offsetof(jd_final, %s));\n" % f for f in names) + "    printf(\"\\n\");\n    return 0;\n}\n")
    exe = tmp_path / "layout"
    subprocess.check_call([cc, "-std=c99", "-Wall", "-Werror", "-I", INCLUDE, "-o", str(exe), str(src)])
    got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert got == [C.sizeof(capi.CFinal)] + [getattr(capi.CFinal, f).offset for f in names] == [28] + [4 * k for k in range(7)]
