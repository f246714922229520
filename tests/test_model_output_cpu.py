"""Model-level output on the paths a Juicer harness uses, without a GPU: the HMM names the loaders keep (jd_am_hmm_name), the
model-level partial trace's declaration and argument checks (jd_stream_partial_models), the adapter's DHHTYPE / LABDHHTYPE chain
compiled in both of its branches, and jd_batch_test -modelLevelOutput's refusals (no kernel is launched here)."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INC = os.path.join(ROOT, "include")
NEW = ["jd_am_hmm_name", "jd_stream_partial_models"]


def test_new_symbols_declared_and_exported(built):
    from juicer_amd import capi
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(INC, "juicer_amd.h")).read(), flags=re.S)
    for s in NEW:
        assert re.search(r"\b%s\s*\(" % s, hdr), s
        assert s in capi.EXPORTS, s
        assert hasattr(capi.lib(), s), s


def test_new_calls_refuse_bad_arguments(built):
    from juicer_amd import capi, synth
    L = capi.lib()
    nm = C.c_char_p()
    assert L.jd_am_hmm_name(None, C.c_int32(0), C.byref(nm)) == capi.JD_EINVAL
    assert b"jd_am_hmm_name" in L.jd_last_error()
    m = capi.Models.from_htk(synth.config_toy()[0])
    for i in (-1, m.n_hmms):
        assert L.jd_am_hmm_name(m.h, C.c_int32(i), C.byref(nm)) == capi.JD_EINVAL, i
    assert L.jd_am_hmm_name(m.h, C.c_int32(0), None) == capi.JD_EINVAL
    n = C.c_int32(0)
    assert L.jd_stream_partial_models(None, C.c_int32(0), C.c_int32(1), C.c_int32(0), C.byref(n), None, None, None, None, None,
                                      None, None) == capi.JD_EINVAL
    assert b"jd_stream_partial_models" in L.jd_last_error()


def _mmf_names(path):
    return re.findall(r'~h "([^"]*)"', open(path).read())


def test_hmm_names_from_mmf_jmbi_and_arrays(built, tmp_path):
    from juicer_amd import capi, io as jio, synth
    from oracle import binfmt
    am = synth.make_models(5, n_gmm=12, n_hmm=9, n_mix=3, D=7, n_tm=4, with_tee=True)
    # arrays: no names
    m0 = capi.Models.from_htk(am)
    assert m0.hmm_names() is None
    nm = C.c_char_p(b"x")
    assert capi.lib().jd_am_hmm_name(m0.h, C.c_int32(0), C.byref(nm)) == capi.JD_OK and nm.value is None
    det, mean, ivar = m0.flat()
    assert capi.Models.from_flat(det, mean, ivar, m0.topology()[3]).hmm_names() is None
    # an unnamed JMBI (what jd_am_save_jmbi writes for array-built models) has none either
    m0.save_jmbi(str(tmp_path / "plain.bin"))
    assert capi.Models.from_jmbi_file(str(tmp_path / "plain.bin")).hmm_names() is None
    # MMF: the ~h names, in order of appearance
    jio.write_mmf(str(tmp_path / "m.mmf"), am)
    mm = capi.Models.from_mmf_file(str(tmp_path / "m.mmf"))
    want = _mmf_names(str(tmp_path / "m.mmf"))
    assert len(want) == am.n_hmm and mm.hmm_names() == want
    # JMBI: the JMHM records' names, as the restated reader sees them
    names = ["sil", "a-b+c", "sp"] + ["ph%02d" % h for h in range(3, am.n_hmm)]
    p = str(tmp_path / "named.bin")
    slv = (np.log(am.var.astype(np.float64)).sum(axis=2) + am.D * np.log(2 * np.pi)).astype(np.float32)
    lw = np.log(np.maximum(am.weight, 1e-30)).astype(np.float32)
    jio.write_jmbi(p, am, dict(sum_log_var=slv, log_weight=lw, trP=m0.trans()[0]), hmm_names=names)
    mj = capi.Models.from_jmbi_file(p)
    assert mj.hmm_names() == binfmt.read_jmbi(p)["hmm_names"] == names
    # ... and jd_am_save_jmbi writes them back: a save and a reload round-trip them, from either loader
    for src, expect in ((mj, names), (mm, want)):
        q = str(tmp_path / "again.bin")
        src.save_jmbi(q)
        assert binfmt.read_jmbi(q)["hmm_names"] == expect
        back = capi.Models.from_jmbi_file(q)
        assert back.hmm_names() == expect
        back.save_jmbi(str(tmp_path / "again2.bin"))
        assert open(q, "rb").read() == open(str(tmp_path / "again2.bin"), "rb").read()
    # the pointer stays valid while the handle lives
    p0 = C.c_char_p()
    capi.lib().jd_am_hmm_name(mj.h, C.c_int32(1), C.byref(p0))
    capi.lib().jd_am_hmm_name(mj.h, C.c_int32(2), C.byref(C.c_char_p()))
    assert p0.value == b"a-b+c"


# -- the adapter (include/juicer_amd_decoder.hpp)
STANDALONE = r"""
#include "juicer_amd_decoder.hpp"
#include <cstddef>
#include <type_traits>
static_assert(LABDHHTYPE == 2 && DHHTYPE == 1, "DecHypHistPool.h:106-107");
static_assert(std::is_same<decltype(JuicerAmd::LabDecHypHist::label), int>::value, "LabDecHypHist::label");
static_assert(offsetof(JuicerAmd::LabDecHypHist, prev) == offsetof(JuicerAmd::DecHypHist, prev), "shared head");
void f(JuicerAmd::GpuWFSTDecoder &d, JuicerAmd::GpuWFSTPooledDecoder &p) { d.setModelLevelOutput(true); (void)d.modelLevelOutput();
                                                                           p.setModelLevelOutput(false); }
int main() { return 0; }
"""

IN_TREE = r"""
#include "Decoder.h"
#include "DecHypHistPool.h"
#include "juicer_amd_decoder.hpp"
#include <type_traits>
static_assert(std::is_same<JuicerAmd::LabDecHypHist, Juicer::LabDecHypHist>::value, "Juicer's own LabDecHypHist");
static_assert(std::is_same<JuicerAmd::DecHyp, Juicer::DecHyp>::value, "Juicer's own DecHyp");
void f(JuicerAmd::GpuWFSTDecoder &d) { d.setModelLevelOutput(true); (void)d.modelLevelOutput(); }
"""


def test_adapter_compiles_with_model_level_output(tmp_path):
    """stand-alone (mirror LabDecHypHist), in the Juicer tree with DecHypHistPool.h (tests/mock_juicer_hist/: Juicer's
    declarations plus LabDecHypHist), and in the tree without it (tests/mock_juicer/, unchanged: setModelLevelOutput(true)
    then fails at run time)"""
    (tmp_path / "a.cpp").write_text(STANDALONE)
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-fsyntax-only", "-I", INC, str(tmp_path / "a.cpp")])
    subprocess.check_call(["g++", "-std=c++98", "-Wall", "-Werror", "-fsyntax-only", "-I", INC, "-x", "c++",
                           os.path.join(INC, "juicer_amd_decoder.hpp")])
    hist = os.path.join(ROOT, "tests", "mock_juicer_hist")
    (tmp_path / "b.cpp").write_text(IN_TREE)
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-fsyntax-only", "-I", hist, "-I", INC, str(tmp_path / "b.cpp")])
    subprocess.check_call(["g++", "-std=c++98", "-Wall", "-fsyntax-only", "-I", hist, "-I", INC, "-x", "c++",
                           "-include", "Decoder.h", "-include", "DecHypHistPool.h", os.path.join(INC, "juicer_amd_decoder.hpp")])
    mock = os.path.join(ROOT, "tests", "mock_juicer")
    (tmp_path / "c.cpp").write_text('#include "Decoder.h"\n#include "juicer_amd_decoder.hpp"\n'
                                    "void f(JuicerAmd::GpuWFSTDecoder &d) { d.setModelLevelOutput(false); }\n")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-fsyntax-only", "-I", mock, "-I", INC, str(tmp_path / "c.cpp")])


# -- jd_batch_test -modelLevelOutput
def _case_on_disk(tmp_path):
    from juicer_amd import io as jio, synth
    am, net, feats, _ = synth.config_toy()
    jio.write_fsm(str(tmp_path / "g.fsm"), net)
    jio.write_mmf(str(tmp_path / "m.mmf"), am)
    jio.write_jdam(str(tmp_path / "m.jdam"), am)
    jio.write_jdf(str(tmp_path / "u0.jdf"), feats[0])
    (tmp_path / "list.txt").write_text(str(tmp_path / "u0.jdf") + "\n")
    (tmp_path / "ref.txt").write_text("1 2\n")
    return [str(tmp_path / "g.fsm"), str(tmp_path / "m.mmf"), str(tmp_path / "list.txt")]


@pytest.mark.parametrize("extra, what", [(["-threads", "2"], "-threads"), (["-devices", "2"], "-devices"),
                                         (["-refFName", "REF"], "-refFName")])
def test_batch_test_refuses_what_cannot_give_models(built, tmp_path, extra, what):
    """refused with a message before anything touches a device (no GPU here: a device call would fail differently)"""
    from juicer_amd import build as jbuild
    fsm, mmf, lst = _case_on_disk(tmp_path)
    extra = [str(tmp_path / "ref.txt") if e == "REF" else e for e in extra]
    r = subprocess.run([jbuild.BATCH_TEST, "-fsmFName", fsm, "-htkModelsFName", mmf, "-inputFName", lst, "-mainBeam", "150",
                        "-modelLevelOutput"] + extra, capture_output=True, text=True, timeout=60)
    assert r.returncode != 0
    assert "-modelLevelOutput" in r.stderr and what in r.stderr, r.stderr
    assert r.stdout == ""


def test_batch_test_refuses_models_without_names(built, tmp_path):
    from juicer_amd import build as jbuild
    fsm, _, lst = _case_on_disk(tmp_path)
    r = subprocess.run([jbuild.BATCH_TEST, "-fsmFName", fsm, "-modelsFName", str(tmp_path / "m.jdam"), "-inputFName", lst,
                        "-mainBeam", "150", "-modelLevelOutput"], capture_output=True, text=True, timeout=60)
    assert r.returncode != 0 and "names" in r.stderr, r.stderr


def test_batch_test_usage_names_the_flag_and_the_accepted_options(built):
    from juicer_amd import build as jbuild
    r = subprocess.run([jbuild.BATCH_TEST], capture_output=True, text=True, timeout=60)
    assert r.returncode == 2
    for o in ("-modelLevelOutput", "-monoListFName", "-tiedListFName", "-cdSepChars", "-silMonophone", "-pauseMonophone"):
        assert o in r.stderr, o
