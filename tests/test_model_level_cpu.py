"""Model-level output without a GPU: the C ABI declares and exports it, the ctypes mirror of jd_model_hyp has the header's layout,
and its calls fail loudly on bad arguments (no kernel is launched here)."""
import ctypes as C
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["jd_dec_set_output_level", "jd_dec_get_output_level", "jd_dec_model_result"]


def test_model_level_symbols_declared_and_exported(built):
    from juicer_amd import capi
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "juicer_amd.h")).read(), flags=re.S)
    for s in NEW:
        assert re.search(r"\b%s\s*\(" % s, hdr), s
        assert s in capi.EXPORTS, s
        assert hasattr(capi.lib(), s), s
    assert re.search(r"#define JD_OUTPUT_WORDS\s+1\b", hdr) and re.search(r"#define JD_OUTPUT_MODELS\s+2\b", hdr)
    assert (capi.OUTPUT_WORDS, capi.OUTPUT_MODELS) == (1, 2)


def test_model_hyp_layout_matches_header(built, tmp_path):
    from juicer_amd import capi
    src = ['#include <stdio.h>', '#include <stddef.h>', '#include "juicer_amd.h"', "int main(void) {",
           '  printf("size %zu\\n", sizeof(jd_model_hyp));']
    for f, _ in capi.CModelHyp._fields_:
        src.append('  printf("%s %%zu\\n", offsetof(jd_model_hyp, %s));' % (f, f))
    src.append("  return 0; }")
    (tmp_path / "l.c").write_text("\n".join(src))
    exe = str(tmp_path / "l")
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), "-o", exe, str(tmp_path / "l.c")])
    got = dict(line.split() for line in subprocess.check_output([exe]).decode().split("\n") if line)
    assert int(got["size"]) == C.sizeof(capi.CModelHyp)
    for f, _ in capi.CModelHyp._fields_:
        assert int(got[f]) == getattr(capi.CModelHyp, f).offset, f


def test_model_level_calls_refuse_bad_arguments(built):
    from juicer_amd import capi
    L = capi.lib()
    v = C.c_int32(0)
    assert L.jd_dec_set_output_level(None, C.c_int32(3)) == capi.JD_EINVAL
    assert L.jd_dec_get_output_level(None, C.byref(v)) == capi.JD_EINVAL
    assert L.jd_dec_model_result(None, C.c_int32(0), C.byref(capi.CModelHyp())) == capi.JD_EINVAL
    assert b"jd_dec_model_result" in L.jd_last_error()


def _check_projection(net, am, x, what):
    import indep_viterbi_models as ivm
    import indep_viterbi_np as iv
    ll = iv.gmm_loglik(am, x)
    ref, got = iv.viterbi(net, am, ll), ivm.viterbi_models(net, am, ll)
    if ref is None:
        assert got is None, what
        return None
    proj = ivm.word_projection(got)
    assert proj[1] == ref[1], what
    assert abs(proj[0] - ref[0]) <= 1e-9 * max(1.0, abs(ref[0])), what
    # the chain itself: times never decrease, scores are those of one path (the last record's score plus the rest of the path)
    ch = got[2]
    assert all(a[2] <= b[2] for a, b in zip(ch, ch[1:])), what
    assert all(m > 0 or lab > 0 for (m, lab, _t, _s, _l) in ch), what
    return got


@pytest.mark.parametrize("case", ["flat_hub", "tree_hub", "mixed_topologies"])
def test_model_viterbi_word_projection_on_indep_cases(case):
    """tests/indep_viterbi_models.py projected to its words is tests/indep_viterbi_np.py, on the anchor's graphs"""
    import indep_cases
    am, net, feats, _ = indep_cases.CASES[case]()
    got = _check_projection(net, am, feats[0], case)
    assert got is not None and sum(1 for r in got[2] if r[0] > 0) > len([r for r in got[2] if r[1] > 0])


@pytest.mark.parametrize("seed", [3, 8, 21, 34])
def test_model_viterbi_word_projection_on_random_topologies(seed):
    import random_topology as rt
    from juicer_amd import synth
    am = synth.make_models(seed, n_gmm=40, n_hmm=12, n_mix=3, D=13, n_tm=4, with_tee=True)
    net = rt.random_net(seed, am, n_states=60, p_eps=0.2, p_label=0.35)
    for k in range(2):
        _check_projection(net, am, rt.random_walk_features(seed * 10 + k, net, am), "seed %d utt %d" % (seed, k))
