"""Model-level output on a Juicer harness's paths: the C++ adapter's DHHTYPE / LABDHHTYPE chain from finish()
(GpuWFSTDecoder::setModelLevelOutput) and jd_batch_test -modelLevelOutput (DecoderBatchTest's DBT_MODE_WFSTDECODE_PHONES),
both held to jd_dec_model_result of the same decode through the C ABI."""
import os
import struct
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DHH, LAB = 1, 2                 # DecHypHistPool.h:106-107
WM, MM = 1, 1 | 2
BEAM = 150.0


def _disk_case(tmp_path, which):
    from juicer_amd import io as jio, synth
    am, net, feats, _ = synth.config_small(n_utts=3) if which == "small" else synth.config_mixed(n_utts=3)
    d = tmp_path / which
    d.mkdir()
    jio.write_fsm(str(d / "g.fsm"), net)
    jio.write_mmf(str(d / "m.mmf"), am)
    files = []
    for u, x in enumerate(feats):
        jio.write_jdf(str(d / ("u%d.jdf" % u)), x)
        files.append(str(d / ("u%d.jdf" % u)))
    (d / "list.txt").write_text("".join(f + "\n" for f in files))
    return dict(fsm=str(d / "g.fsm"), mmf=str(d / "m.mmf"), list=str(d / "list.txt"), files=files, feats=feats, dir=d)


def _capi_stream(c, level, push=64):
    """the adapter's decode through the C ABI: one stream, the adapter's 64-frame pushes"""
    from juicer_amd import capi
    gnet, gam = capi.Network.from_fsm_file(c["fsm"]), capi.Models.from_mmf_file(c["mmf"])
    dec = capi.Decoder(gnet, gam, main_beam=BEAM, max_streams=1)
    dec.set_output_level(level)
    out = []
    for x in c["feats"]:
        dec.stream_init(0)
        for i in range(0, x.shape[0], push):
            dec.stream_push(0, x[i:i + push])
        out.append(dec.stream_finish(0))
    dec.close()
    return out, gam.hmm_names()


def _chain_of(m):
    """jd_model_hyp -> the records finish() gives, newest first: (type, state or label, time, score, ac, lm)"""
    recs = []
    for k in range(m.n):
        if m.model[k]:
            recs.append((DHH, int(m.model[k]), int(m.time[k]), m.score[k], m.ac[k], m.lm[k]))
        if m.label[k]:
            recs.append((LAB, int(m.label[k]), 0, np.float32(0), np.float32(0), np.float32(0)))
    return recs


def extract_phone_mode(recs):
    """DecoderSingleTest::extractResultsFromHypPhoneMode (DecoderSingleTest.cpp:471-565), restated over the chain
    (newest first): per phone index (state - 1), start, end, ac, lm (float32 differences), and word (label - 1 or -1)"""
    nP = sum(1 for r in recs if r[0] == DHH)
    nW = sum(1 for r in recs if r[0] == LAB)
    assert nP >= nW, "number of words exceeded num phones in result"
    if nP == 0:
        return None
    assert nW > 0, "no words found in result"
    ph, st, et, wd = [-1] * nP, [-1] * nP, [-1] * nP, [-1] * nP
    ac = [np.float32(-np.finfo(np.float32).max)] * nP
    lm = list(ac)
    p = w = nP - 1
    for r in recs:
        if r[0] == DHH:
            ph[p], ac[p], lm[p], et[p] = r[1] - 1, np.float32(r[4]), np.float32(r[5]), r[2]
            if p < nP - 1:
                st[p + 1] = et[p]
                ac[p + 1] = np.float32(ac[p + 1] - ac[p])
                lm[p + 1] = np.float32(lm[p + 1] - lm[p])
            p -= 1
        else:
            wd[w] = r[1] - 1
            w -= 1
    st[0] = 0
    return dict(phone=ph, start=st, end=et, ac=ac, lm=lm, word=wd)


def _read_driver(path, n_utts):
    out = []
    with open(path, "rb") as f:
        for _ in range(n_utts):
            n = struct.unpack("i", f.read(4))[0]
            tot = np.frombuffer(f.read(12), np.float32)
            recs = []
            for _ in range(max(n, 0)):
                t, i, tm = struct.unpack("3i", f.read(12))
                s = np.frombuffer(f.read(12), np.float32)
                recs.append((t, i, tm, s[0], s[1], s[2]))
            out.append((n, tot, recs))
        assert f.read() == b""
    return out


def _bits(x):
    return np.float32(x).view(np.int32)


def _same_recs(a, b, what):
    assert len(a) == len(b), what
    for k, (x, y) in enumerate(zip(a, b)):
        assert x[:3] == y[:3], "%s record %d: %s vs %s" % (what, k, x[:3], y[:3])
        assert all(_bits(p) == _bits(q) for p, q in zip(x[3:], y[3:])), "%s record %d scores" % (what, k)


@pytest.fixture(scope="module")
def driver(built, tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("adapter") / "adapter_models")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-o", exe,
                           os.path.join(ROOT, "tests", "adapter_models", "adapter_models.cpp"), "-L", os.path.join(ROOT, "juicer_amd"),
                           "-ljuicer_amd", "-Wl,-rpath," + os.path.join(ROOT, "juicer_amd"), "-Wl,-rpath-link,/opt/rocm/lib"])
    return exe


@pytest.mark.parametrize("which", ["small", "mixed"])
def test_adapter_model_chain(driver, tmp_path, which):
    c = _disk_case(tmp_path, which)
    n = len(c["feats"])
    for level in (MM, WM):
        out = str(tmp_path / ("chain%d.bin" % level))
        r = subprocess.run([driver, c["fsm"], c["mmf"], out, "1" if level == MM else "0", str(BEAM)] + c["files"],
                           capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr
        got = _read_driver(out, n)
        want, _ = _capi_stream(c, level)
        for u, ((gn, gtot, grecs), h) in enumerate(zip(got, want)):
            what = "%s utt %d level %d" % (which, u, level)
            assert h.n >= 0 and gn >= 0, what
            if level == WM:
                # word mode: today's chain - DHHTYPE records of the words, bit for bit
                exp = [(DHH, int(h.label[k]), int(h.time[k]), h.score[k], h.ac[k], h.lm[k]) for k in range(h.n)]
                _same_recs(grecs, exp, what)
                assert [_bits(v) for v in gtot] == [_bits(v) for v in (h.tot_score, h.tot_ac, h.tot_lm)], what
                continue
            m = h.models
            _same_recs(grecs, _chain_of(m), what)
            assert [_bits(v) for v in gtot] == [_bits(v) for v in (m.tot_score, m.tot_ac, m.tot_lm)], what
            # what DecoderSingleTest's phone mode makes of it
            res = extract_phone_mode(grecs)
            assert res is not None, what
            old = m.model[::-1]
            mods = old[old != 0]
            assert res["phone"] == (mods - 1).tolist(), what                         # phones = models - 1
            assert res["start"][0] == 0 and res["start"][1:] == res["end"][:-1], what
            ends = m.time[::-1][old != 0]
            assert res["end"] == ends.tolist(), what
            acs, lms = m.ac[::-1][old != 0], m.lm[::-1][old != 0]
            assert _bits(res["ac"][0]) == _bits(acs[0]) and _bits(res["lm"][0]) == _bits(lms[0]), what
            for p in range(1, len(mods)):
                assert _bits(res["ac"][p]) == _bits(np.float32(acs[p] - acs[p - 1])), what
                assert _bits(res["lm"][p]) == _bits(np.float32(lms[p] - lms[p - 1])), what
            words = (m.label[::-1][m.label[::-1] != 0] - 1).tolist()               # oldest first
            pad = len(mods) - len(words)
            assert res["word"] == [-1] * pad + words, what                           # word k from the end beside phone k from the end


# -- jd_batch_test -modelLevelOutput
def _run_tool(c, *extra, model=True, fmt="ref"):
    from juicer_amd import build as jbuild
    cmd = [jbuild.BATCH_TEST, "-fsmFName", c["fsm"], "-htkModelsFName", c["mmf"], "-inputFName", c["list"], "-mainBeam", str(BEAM),
           "-outputFormat", fmt] + (["-modelLevelOutput"] if model else []) + list(extra)
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    return r.stdout


def _hmm_time(t, fps=100):
    v = np.float32(1.0e7) / np.float32(fps) * np.float32(t)
    v = float(v)
    if v > 0:
        v += float(np.float32(1.0e7) / np.float32(fps))
    return "%.0f" % v


def _expected_phones(c, hyps, names, fmt):
    """DecoderBatchTest::outputResultPhones (DecoderBatchTest.cpp:528-645) of the C ABI's results"""
    lines = ["#!MLF!#"] if fmt in ("mlf", "xmlf") else []
    for u, h in enumerate(hyps):
        r = extract_phone_mode(_chain_of(h.models))
        n = len(r["phone"]) if r else 0
        ph = [names[r["phone"][j]] for j in range(n)]
        if fmt == "ref":
            lines.append("".join(p + " " for p in ph))
        elif fmt == "trans":
            lines.append("".join(p + " " for p in ph) + "(trans-%d)" % n)
        elif fmt in ("mlf", "xmlf"):
            lines.append('"*/u%d.rec"' % u)
            for j in range(n):
                if fmt == "mlf":
                    s = ph[j]
                else:
                    s = "%s %s %s %f" % (_hmm_time(r["start"][j]), _hmm_time(r["end"][j]), ph[j], float(np.float32(r["ac"][j] + r["lm"][j])))
                if r["word"][j] >= 0:
                    s += " %d" % r["word"][j]                                  # (no symbol table: the word id)
                lines.append(s)
            lines.append(".")
        else:
            lines.append(c["files"][u])
            lines.append("\tActual :    " + "".join(p + " " for p in ph) + "  [ " + "".join("%d " % (e + 1) for e in (r["end"] if r else []))
                         + "(%d) ]" % c["feats"][u].shape[0])
    return "\n".join(lines) + "\n"


def _expected_words(c, hyps, fmt):
    """word mode as jd_batch_test prints it (outputResult, DecoderBatchTest.cpp:339-430)"""
    lines = ["#!MLF!#"] if fmt == "xmlf" else []
    for u, h in enumerate(hyps):
        k = max(h.n, 0)
        lab, et = h.label[:k][::-1], h.time[:k][::-1]
        ac, lm = h.ac[:k][::-1], h.lm[:k][::-1]
        if fmt == "verbose":
            lines.append(c["files"][u])
            lines.append("\tActual :    " + "".join("%d " % (l - 1) for l in lab) + "  [ " + "".join("%d " % (e + 1) for e in et)
                         + "(%d) ]" % c["feats"][u].shape[0])
        else:
            lines.append('"*/u%d.rec"' % u)
            for w in range(k):
                st = 0 if w == 0 else et[w - 1]
                wac = np.float32(ac[w] - (ac[w - 1] if w else np.float32(0)))
                wlm = np.float32(lm[w] - (lm[w - 1] if w else np.float32(0)))
                lines.append("%s %s %d %f" % (_hmm_time(st), _hmm_time(et[w]), lab[w] - 1, float(np.float32(wac + wlm))))
            lines.append(".")
    return "\n".join(lines) + "\n"


def test_batch_test_model_level_output(built, tmp_path):
    from juicer_amd import capi
    c = _disk_case(tmp_path, "small")
    gnet, gam = capi.Network.from_fsm_file(c["fsm"]), capi.Models.from_mmf_file(c["mmf"])
    names = gam.hmm_names()
    assert names and len(names) == gam.n_hmms
    hyps = {}
    for level in (WM, MM):
        dec = capi.Decoder(gnet, gam, main_beam=BEAM, max_streams=len(c["feats"]))
        dec.set_output_level(level)
        hyps[level] = dec.decode_batch(c["feats"])
        dec.close()
    assert all(h.n > 0 and h.models.n > h.n for h in hyps[MM])
    for fmt in ("ref", "trans", "mlf", "xmlf", "verbose"):
        assert _run_tool(c, fmt=fmt) == _expected_phones(c, hyps[MM], names, fmt), fmt
    # the batch path in pieces, the adapter (the reference's serial protocol) and the resident slots: the same output
    want = _expected_phones(c, hyps[MM], names, "xmlf")
    for extra in (["-batch", "2"], ["-perFrameAdapter"], ["-residentSlots", "2"]):
        assert _run_tool(c, *extra, fmt="xmlf") == want, extra
    assert _run_tool(c, "-perFrameAdapter", fmt="verbose") == _expected_phones(c, hyps[MM], names, "verbose")
    # the phone-lookup options are accepted and change nothing
    assert _run_tool(c, "-monoListFName", "x", "-tiedListFName", "y", "-cdSepChars", "-+", "-silMonophone", "sil",
                     "-pauseMonophone", "sp", fmt="mlf") == _expected_phones(c, hyps[MM], names, "mlf")
    # without the flag: word mode as before
    for fmt in ("verbose", "xmlf"):
        assert _run_tool(c, model=False, fmt=fmt) == _expected_words(c, hyps[WM], fmt), fmt
        assert _run_tool(c, "-perFrameAdapter", model=False, fmt=fmt) == _expected_words(c, hyps[WM], fmt), fmt
