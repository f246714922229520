"""Partial traces for many streams at once - the C ABI's new entry points, as far as they can be held without a device."""
import ctypes as C

import pytest


@pytest.mark.parametrize("sym", ["jd_streams_trace", "jd_dec_get_partial_interval", "jd_broker_partial"])
def test_new_symbols_resolve(built, sym):
    from juicer_amd import capi
    assert sym in capi.EXPORTS
    assert hasattr(capi.lib(), sym)


def test_null_handles_are_refused_with_a_message(built):
    from juicer_amd import capi
    L = capi.lib()
    n, v = C.c_int32(0), C.c_int32(0)
    s = (C.c_int32 * 1)(0)
    calls = (("jd_streams_trace", lambda: L.jd_streams_trace(None, C.c_int32(1), s, None)),
             ("jd_broker_partial", lambda: L.jd_broker_partial(None, C.c_int32(0), C.c_int32(0), C.byref(n), None, None)),
             ("jd_dec_get_partial_interval", lambda: L.jd_dec_get_partial_interval(None, C.byref(v))))
    for what, call in calls:
        assert call() == capi.JD_EINVAL, what
        assert what in L.jd_last_error().decode(), what


def test_timing_keeps_its_layout(built):
    """jd_timing.pad0 became trace_launches: the same place, the same size"""
    from juicer_amd import capi
    assert C.sizeof(capi.Timing) == 88
    assert capi.Timing.trace_launches.offset == 84 and capi.Timing.trace_launches.size == 4
    assert capi.Timing.slot_launches.offset == 80
    assert [f for f, _ in capi.Timing._fields_][-1] == "trace_launches"
