"""The end-of-utterance view (k_final_many) and the model-level traces for many streams (k_partial_many_models) of
juicer_amd/csrc/jd_gc.h on states a test chose, through jd_debug_paths' PD_FINAL_MANY and PD_TRACE_MANY_MODELS: every named case of
tests/paths_live_cases.py, every word that comes back - the streams' state, the kernels' whole reply buffers (heads and shares), the
result arrays, the model rows and the model lists, all prefilled with a sentinel - against tests/paths_live_ref.py (which
tests/test_paths_live_cpu.py holds to the cases' construction).  All of it is integer code: every comparison is exact."""
import pytest

import paths_live_cases as lc
import paths_live_ref as lr
import paths_ref as pr

pytestmark = pytest.mark.gpu


def check(names):
    from juicer_amd import capi
    assert names
    for name in names:
        D = lc.case(name)
        want, what = lr.run(D)
        got = capi.debug_paths(lr.encode(D), 0)
        assert pr.first_mismatch(got, want, what, name) is None


@pytest.mark.parametrize("part", range(2))
def test_final_view_on_described_states(built, part):
    check(lc.names("final_")[part::2])


@pytest.mark.parametrize("part", range(2))
def test_model_traces_on_described_states(built, part):
    check(lc.names("tm_")[part::2])


def test_refused_before_any_device_call(built):
    from juicer_amd import capi
    D = lc.case("final_two_of_three_streams")
    words = lr.encode(D)
    bad_stream, bad_cap = words.copy(), words.copy()
    bad_stream[-10] = 3                                   # the first entry's stream (three streams: 0 .. 2)
    bad_cap[-2] = 0                                        # res_cap
    T = lr.encode(lc.case("tm_have_equal"))
    neg = T.copy()
    neg[-2] = -1                                           # have_m
    for w in (bad_stream, bad_cap, neg, words[:-1]):
        with pytest.raises(capi.JuicerAmdError) as e:
            capi.debug_paths(w, 0)
        assert e.value.code == capi.JD_EINVAL
