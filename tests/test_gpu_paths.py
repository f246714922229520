"""The Path collection (launch_gc: k_gc_begin / mark / sum / scan / compact / remap) and the PARTIAL_DECODING trace (k_partial,
k_partial_many) of juicer_amd/csrc/jd_gc.h on states a test chose, through jd_debug_paths: every named case of tests/paths_cases.py,
every word that comes back - counters, GcState words, the compacted arena bit for bit, every token's and item's path, the traces'
output words, result arrays and model rows - against tests/paths_ref.py (which tests/test_paths_ref_cpu.py holds to a brute force,
and which says there what shape each case has).  All of it is integer code: every comparison is exact."""
import pytest

import paths_cases as pc
import paths_ref as pr

pytestmark = pytest.mark.gpu


def check(names):
    from juicer_amd import capi
    assert names
    for name in names:
        D = pc.case(name)
        want, what = pr.run(D)
        got = capi.debug_paths(pc.encode(D), 0)
        assert pr.first_mismatch(got, want, what, name) is None


@pytest.mark.parametrize("family", [f for f in pc.FAMILIES if f != "sizes"])
def test_device_paths(built, family):
    check(pc.names(family))


@pytest.mark.parametrize("part", range(4))
def test_device_paths_sizes(built, part):
    """arena sizes crossed with workgroups per stream: ranges of one, two, three and more scan trips, tails, empty ranges"""
    check(pc.names("sizes")[part::4])


def test_device_paths_refuses_before_any_device_call(built):
    from juicer_amd import capi
    D = pc.case("trace_deep_record_shared")
    words = pc.encode(D)
    bad = words.copy()
    bad[1] = 4                                             # NE
    for w in (bad, words[:-1], words[:3]):
        with pytest.raises(capi.JuicerAmdError) as e:
            capi.debug_paths(w, 0)
        assert e.value.code == capi.JD_EINVAL
