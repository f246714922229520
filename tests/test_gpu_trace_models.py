"""Model-level partial traces for many live streams: jd_streams_trace_models (k_partial_many_models) is
jd_stream_partial_models(s, trace_now = 1) for a list of streams - one launch, one copy.

Three streams with a lag, a trace after every push: found and both lists of every stream are those of a twin model-level decoder
traced stream by stream at the same frames, the word lists are those of a word-level decoder traced with jd_streams_trace, and the
properties tests/test_gpu_model_partial.py states of a single stream's traces hold for each of them."""
import numpy as np
import pytest

from live_cases import CASES, MFIELDS, _bits, _decoder, _handles

pytestmark = pytest.mark.gpu


def _mlist(m):
    return tuple(_bits(getattr(m, f)) for f in MFIELDS)


def _schedule(feats, steps, n_calls):
    """per call: [(stream, frames)] - stream 2 a call behind, every third call lists stream 1 without frames"""
    T, out = [0, 0, 0], []
    for call in range(n_calls):
        entry = []
        for s in range(3):
            if s == 2 and call == 0:
                continue
            n = 0 if (s == 1 and call % 3 == 2) else min(steps[s], feats[s].shape[0] - T[s])
            entry.append((s, feats[s][T[s]:T[s] + n]))
            T[s] += n
        out.append(entry)
    return out


def _check_stream(traces, fin, what):
    """test_gpu_model_partial._check's properties for one stream: traces = [(found, words, model list)], fin = the finished Hyp"""
    m_fin = fin.models
    old = tuple(l[::-1] for l in _mlist(m_fin))
    prev = None
    for j, (found, words, m) in enumerate(traces):
        n = len(m[0])
        lab = [(l, t) for l, t in zip(m[1], m[2]) if l != 0]
        assert lab == words, (what, j)                                  # its labelled entries are the word list of the same trace
        if n:
            assert m[1][-1] != 0, (what, j)                             # it ends at the record the word list ends at
            assert all(a >= 0 and (a != 0 or l != 0) for a, l in zip(m[0], m[1])), (what, j)
        if prev is not None:                                            # a prefix of the next trace
            assert len(prev[0]) <= n and all(a[:len(prev[0])] == b for a, b in zip(m, prev)), (what, j)
        assert n <= m_fin.n, (what, j)                                  # a prefix of the final chain (whose newest entry carries the final weight)
        k = n if n < m_fin.n else n - 1
        assert all(a[:k] == b[:k] for a, b in zip(m, old)), (what, j)
        if n == m_fin.n and n:
            assert all(a[-1] == b[-1] for a, b in zip(m[:3], old[:3])), (what, j)
        prev = m


@pytest.mark.parametrize("max_paths", [0, 1 << 12], ids=["plain", "collecting"])
@pytest.mark.parametrize("name", CASES)
def test_many_equals_single(built, name, max_paths):
    _, _, feats, _, steps = _handles(name)
    many, twin = (_decoder(name, True, max_streams=3, max_paths=max_paths) for _ in range(2))
    word = _decoder(name, False, max_streams=3, max_paths=max_paths)
    for d in (many, twin, word):
        for s in range(3):
            d.stream_init(s)
    traces = {s: [] for s in range(3)}
    n_found = 0
    n_calls = max(-(-feats[s].shape[0] // steps[s]) for s in range(3)) + 2
    for call, entry in enumerate(_schedule(feats, steps, min(n_calls, 12))):
        ss, fr = [s for s, _ in entry], [x for _, x in entry]
        for d in (many, twin, word):
            d.streams_push(ss, fr)
        order = [2, 0, 1]
        t0 = many.last_timing()["trace_launches"]
        found = many.streams_trace_models(order)
        assert many.last_timing()["trace_launches"] - t0 == 1
        wfound = word.streams_trace(order)
        for i, s in enumerate(order):
            f1, m1 = twin.stream_partial_models(s, trace_now=True)
            what = (name, call, s)
            assert found[i] == f1 == wfound[i], what
            _, m = many.stream_partial_models(s)
            assert _mlist(m) == _mlist(m1), what
            words = many.stream_partial(s)[1]
            assert words == twin.stream_partial(s)[1] == word.stream_partial(s)[1], what
            traces[s].append((found[i], words, _mlist(m)))
            n_found += found[i]
    for s in range(3):
        fin, fin1 = many.stream_finish(s), twin.stream_finish(s)
        assert _mlist(fin.models) == _mlist(fin1.models)
        _check_stream(traces[s], fin, (name, s))
    if name in ("small", "mixed"):
        assert n_found >= 6, n_found
    for d in (many, twin, word):
        d.close()


def test_beyond_the_share_and_counters(built):
    """A first trace late in concatenated utterances: stream 0 has more new words and model records than its share (32 words, 112
    records) and is read from the device arrays, stream 1 beside it comes through the staging area; both equal the single-stream
    traces of a twin, and the next trace of stream 0 - a few records more - comes through its share."""
    _, _, feats, _, _ = _handles("small")
    x = np.concatenate(feats + feats[:2])
    many, twin = (_decoder("small", True, max_streams=2) for _ in range(2))
    for d in (many, twin):
        d.stream_init(0); d.stream_init(1)
        d.streams_push([0, 1], [x[:2000], x[:120]])
    t0 = many.last_timing()["trace_launches"]
    found = many.streams_trace_models([0, 1])
    assert many.last_timing()["trace_launches"] - t0 == 1
    for s in (0, 1):
        f1, m1 = twin.stream_partial_models(s, trace_now=True)
        _, m = many.stream_partial_models(s)
        assert found[s] == f1 and _mlist(m) == _mlist(m1) and many.stream_partial(s)[1] == twin.stream_partial(s)[1], s
    assert found == [True, True]
    n0, w0 = many.stream_partial_models(0)[1].n, len(many.stream_partial(0)[1])
    assert n0 > 112 and w0 > 32, (n0, w0)
    assert 0 < many.stream_partial_models(1)[1].n <= 112
    for d in (many, twin):
        d.streams_push([0], [x[2000:]])
    found = many.streams_trace_models([1, 0])
    f1, m1 = twin.stream_partial_models(0, trace_now=True)
    _, m = many.stream_partial_models(0)
    assert found[1] == f1 and _mlist(m) == _mlist(m1) and many.stream_partial(0)[1] == twin.stream_partial(0)[1]
    assert 0 <= m.n - n0 <= 112
    # a stream without a frame, an empty list
    many.stream_finish(1); many.stream_init(1)
    assert many.streams_trace_models([1]) == [False] and many.streams_trace_models([]) == []
    for d in (many, twin):
        d.close()


def test_refusals_and_capacity(built, monkeypatch):
    from juicer_amd import capi
    gnet, gam, feats, _, _ = _handles("small")
    dec = _decoder("small", True, max_streams=2)
    dec.stream_init(0)
    for bad, code in (([0, 0], capi.JD_EINVAL), ([2], capi.JD_EINVAL), ([-1], capi.JD_EINVAL), ([0, 1], capi.JD_ESTATE)):
        with pytest.raises(capi.JuicerAmdError) as e:
            dec.streams_trace_models(bad)
        assert e.value.code == code, bad
    with pytest.raises(capi.JuicerAmdError) as e:
        dec.streams_trace([0])                                         # (the word-level call stays refused at model level)
    assert e.value.code == capi.JD_ESTATE
    with pytest.raises(capi.JuicerAmdError) as e:
        dec.set_partial_interval(50)                                   # (and so does the interval)
    assert e.value.code == capi.JD_EINVAL
    dec.close()
    # a list longer than the result capacity fails that stream alone
    monkeypatch.setenv("JD_DEV", "1")
    monkeypatch.setenv("JD_RES_CAP", "16")
    dec = _decoder("small", True, max_streams=2)
    dec.stream_init(0); dec.stream_init(1)
    dec.streams_push([0, 1], [feats[0][:400], feats[1][:40]])
    with pytest.raises(capi.JuicerAmdError) as e:
        dec.streams_trace_models([0, 1])
    assert e.value.code == capi.JD_ENOMEM and "stream 0" in str(e.value), str(e.value)
    assert dec.stream_partial_models(0)[1].n == 0 and dec.stream_partial_models(1)[1].n <= 16
    dec.close()
