"""PARTIAL_DECODING for many streams at once: jd_streams_trace (k_partial_many), jd_streams_push under an interval, the broker's
lists (jd_broker_partial) and jd_batch_test -threads with PartialTraceInterval.  The yardstick is the oracle throughout
(OracleDecoder.decode_partial, collect_frames, path_counts); the single-stream path, itself held to the oracle by
test_gpu_parity, is a second one."""
import os
import threading

import numpy as np
import pytest

from helpers import assert_hyp_matches

pytestmark = pytest.mark.gpu


def _setup(cfg):
    from juicer_amd import capi
    from oracle.oracle import OracleAM, OracleNet
    am, net, feats, words = cfg
    return (capi.Network.from_synth(net), capi.Models.from_htk(am), OracleNet(net), OracleAM(am), feats, words)


@pytest.fixture(scope="module")
def small(built):
    from juicer_amd import synth
    return _setup(synth.config_small())


@pytest.fixture(scope="module")
def small_tree(built):
    from juicer_amd import synth
    return _setup(synth.config_small(hub="tree"))


@pytest.fixture(scope="module")
def mixed(built):
    from juicer_amd import synth
    return _setup(synth.config_mixed())


ROTATIONS = ((2, 3), (3, 2), (2, 1), (3, 1))


@pytest.fixture(scope="module")
def tree_inputs(small_tree):
    """Four concatenations of two of small_tree's utterances (> 450 frames each, another pair or order per stream) and, per interval, what the
    oracle makes of each: (snaps, final, collect_frames) - computed once, shared by the tests below, never changed."""
    from oracle.oracle import OracleDecoder
    gnet, gam, onet, oam, feats, _ = small_tree
    od = OracleDecoder(onet, oam, main_beam=150.0)
    xs = [np.concatenate([feats[i] for i in rot]) for rot in ROTATIONS]
    ora = {}
    for interval in (1, 150):
        ora[interval] = []
        for x in xs:
            assert x.shape[0] > 450
            snaps, final = od.decode_partial(x, interval=interval)
            assert len(snaps) >= 2
            assert od.collect_frames == list(range(100, x.shape[0], 101))   # the frame rule alone
            ora[interval].append((snaps, final, list(od.collect_frames)))
    assert len(set(tuple(o[1]) for o in ora[1])) == len(xs), "the streams' lists are meant to differ"
    return xs, ora


def _hyp_list(g):
    return list(zip(g.label.tolist()[::-1], g.time.tolist()[::-1]))


def _calls(lengths, sizes, skip=True):
    """The calls of a test: per call a list of (stream, lo, hi) - stream k advances by sizes[k] frames per call it takes part
    in, is left out of some calls (not listed) and listed without frames in others."""
    pos = [0] * len(lengths)
    calls, j = [], 0
    while any(p < T for p, T in zip(pos, lengths)):
        call = []
        for k, T in enumerate(lengths):
            if pos[k] >= T:
                continue
            if skip and (j + k) % 3 == 0:
                continue                                              # not listed
            if skip and (j + 2 * k) % 5 == 0:
                call.append((k, pos[k], pos[k]))                      # listed, n_frames = 0
                continue
            hi = min(T, pos[k] + sizes[k])
            call.append((k, pos[k], hi))
            pos[k] = hi
        j += 1
        if call:
            calls.append(call)
    return calls


@pytest.mark.parametrize("cfg_name", ["small", "small_tree", "mixed"])
def test_explicit_traces_many_streams(cfg_name, request):
    """jd_streams_trace: three streams on three utterances, one of them a call behind the others, traced together after every
    push - every stream's (found, list) is the oracle's for its utterance and frame, also with an arena so small that
    collections renumber the records between the traces.  (mixed: k_partial_many<6>.)"""
    from juicer_amd import capi
    from oracle.oracle import OracleDecoder
    gnet, gam, onet, oam, feats, _ = request.getfixturevalue(cfg_name)
    kw = dict(main_beam=150.0, max_hyps=200) if cfg_name != "mixed" else dict(main_beam=200.0)
    od = OracleDecoder(onet, oam, **kw)
    assert len(feats) >= 3
    ats = [list(range(7, feats[u].shape[0], 23)) for u in range(3)]
    snaps = [od.decode_partial(feats[u], interval=0, trace_at=ats[u])[0] for u in range(3)]
    want = [od.decode_certified(feats[u]) for u in range(3)]
    lag = (0, 0, 1)
    n_found = n_traces = 0
    for extra in (dict(), dict(max_paths=1 << 12)):
        gd = capi.Decoder(gnet, gam, max_streams=3, **kw, **extra)
        pos, last, done = [0, 0, 0], [[], [], []], [False] * 3
        for j in range(max(len(a) for a in ats) + 3):
            ss, xs, fs = [], [], []
            for u in range(3):
                i = j - lag[u]
                if i == 0:
                    gd.stream_init(u)
                if 0 <= i < len(ats[u]):
                    f = ats[u][i]
                    ss.append(u); xs.append(feats[u][pos[u]:f + 1]); fs.append(f)
                    pos[u] = f + 1
            if ss:
                gd.streams_push(ss, xs)
                found = gd.streams_trace(ss)
                for u, f, fnd in zip(ss, fs, found):
                    _, lst = gd.stream_partial(u)
                    assert (fnd, lst) == snaps[u][f], "%s utt %d frame %d: %r vs %r" % (cfg_name, u, f, (fnd, lst[-3:]), (snaps[u][f][0], snaps[u][f][1][-3:]))
                    last[u] = lst
                    n_found += fnd
                    n_traces += 1
            for u in range(3):
                if j - lag[u] == len(ats[u]) and not done[u]:
                    gd.streams_push([u], [feats[u][pos[u]:]])
                    g = gd.stream_finish(u)
                    assert_hyp_matches(g, want[u], "partial many %s utt %d" % (cfg_name, u))
                    assert _hyp_list(g)[:len(last[u])] == last[u]      # the prefix that could no longer change
                    done[u] = True
        assert all(done)
        gd.close()
    assert n_found >= 4 and n_found < n_traces, "vacuous: %d of %d traces found a record" % (n_found, n_traces)


def _check_stream(gd, s, at, snaps, collect_frames, what):
    due = [f for f in sorted(snaps) if f <= at]
    _, lst = gd.stream_partial(s)
    assert lst == (snaps[due[-1]][1] if due else []), what
    done = [f for f in collect_frames if f <= at]
    assert gd.stream_collect_info(s) == (len(done), done[-1] if done else -1), what
    return lst


@pytest.mark.parametrize("interval", [1, 150])
def test_schedule_frame_rule(small_tree, tree_inputs, interval):
    """jd_streams_push under an interval: four streams with push sizes of their own, left out of some calls - after every call
    every stream's list is the reference's after its last due trace, its collections the reference's, and finish
    completes the list."""
    from juicer_amd import capi
    gnet, gam = small_tree[:2]
    xs, ora = tree_inputs
    gd = capi.Decoder(gnet, gam, max_streams=4, main_beam=150.0)
    gd.set_partial_interval(interval)
    assert gd.get_partial_interval() == interval
    for s in range(4):
        gd.stream_init(s)
    at = [-1] * 4
    for call in _calls([x.shape[0] for x in xs], (37, 64, 5, 1000)):
        gd.streams_push([k for k, _, _ in call], [xs[k][lo:hi] for k, lo, hi in call])
        for k, lo, hi in call:
            at[k] = hi - 1
        for s in range(4):
            _check_stream(gd, s, at[s], ora[interval][s][0], ora[interval][s][2], "interval %d stream %d after frame %d" % (interval, s, at[s]))
    for s in range(4):
        g = gd.stream_finish(s)
        _, lst = gd.stream_partial(s)
        assert lst == ora[interval][s][1] == _hyp_list(g)
    gd.close()


def _count_rule_case(which):
    from juicer_amd import synth
    from oracle.oracle import OracleAM, OracleDecoder, OracleNet
    if which == "flat":
        am, net, feats, _ = synth.config_small(seed=31, n_utts=2, n_words=400, n_succ=5, n_gmm=120, n_hmm=45, hub="flat")
        allx = np.concatenate(feats)
        xa, xb = allx[:330], allx[allx.shape[0] - 330:]
    else:
        am, net, feats, _ = synth.config_mixed(seed=12, n_utts=3, n_words=300, n_succ=6)
        allx = np.concatenate(feats)
        xa, xb = allx[:260], allx[allx.shape[0] - 260:]
    assert xa.shape == xb.shape and not np.array_equal(xa, xb)
    od = OracleDecoder(OracleNet(net), OracleAM(am), main_beam=250.0)
    ora = []
    for x in (xa, xb):
        snaps, final = od.decode_partial(x, interval=1)
        assert od.collect_frames[0] < 100 and len(od.collect_frames) >= 4
        ora.append((snaps, final, list(od.collect_frames), list(od.path_counts)))
    return am, net, (xa, xb), ora


@pytest.fixture(scope="module")
def count_rule_cases(built):
    return {w: _count_rule_case(w) for w in ("flat", "mixed")}


@pytest.mark.parametrize("which, arena", [("flat", 0), ("flat", 1 << 15), ("mixed", 0)])
def test_schedule_count_rule(count_rule_cases, which, arena):
    """collectPaths' count rule under jd_streams_push: two streams of one call, one pushed a frame at a time, the other 16 -
    the counts behind every call are the reference's, the collections run after its frames (one case with an arena that asks
    for collections of its own in between), the lists grow by prefix and, frame by frame, are the oracle's."""
    from juicer_amd import capi
    am, net, xs, ora = count_rule_cases[which]
    gd = capi.Decoder(capi.Network.from_synth(net), capi.Models.from_htk(am), max_streams=2, main_beam=250.0, **(dict(max_paths=arena) if arena else {}))
    gd.set_partial_interval(1)
    gd.stream_init(0); gd.stream_init(1)
    T = xs[0].shape[0]
    pos_b, prev = 0, [[], []]
    for f in range(T):
        ss, fr = [0], [xs[0][f:f + 1]]
        if f % 8 == 3 and pos_b < T:                                  # (the second stream takes part in every eighth call)
            ss.append(1); fr.append(xs[1][pos_b:pos_b + 16])
            pos_b = min(T, pos_b + 16)
        gd.streams_push(ss, fr)
        for s, at in ((0, f), (1, pos_b - 1)):
            if at < 0:
                continue
            snaps, _, cframes, pcounts = ora[s]
            done = [c for c in cframes if c <= at]
            assert gd.stream_collect_info(s) == (len(done), done[-1] if done else -1), (which, s, at)
            npath, nnew, exact = gd.stream_path_counts(s)
            assert exact and (npath, nnew) == pcounts[at], (which, s, at, npath, nnew, pcounts[at])
            _, lst = gd.stream_partial(s)
            assert lst[:len(prev[s])] == prev[s] and all(t <= at for _, t in lst)
            if s == 0 and at in snaps:
                assert lst == snaps[at][1]
            prev[s] = lst
    while pos_b < T:
        gd.streams_push([1], [xs[1][pos_b:pos_b + 16]])
        pos_b = min(T, pos_b + 16)
    for s in range(2):
        g = gd.stream_finish(s)
        _, lst = gd.stream_partial(s)
        assert lst == ora[s][1] == _hyp_list(g) and lst[:len(prev[s])] == prev[s]
    gd.close()


def test_same_bits_as_single_stream_pushes(small_tree, tree_inputs):
    """The same frames once through jd_stream_push, stream after stream, and once through jd_streams_push: lists, collection
    info and path counts after every call and the hypotheses, bit for bit."""
    from juicer_amd import capi
    gnet, gam = small_tree[:2]
    xs, _ = tree_inputs
    calls = _calls([x.shape[0] for x in xs], (37, 64, 5, 1000))
    trail = []
    for many in (False, True):
        gd = capi.Decoder(gnet, gam, max_streams=4, main_beam=150.0)
        gd.set_partial_interval(1)
        for s in range(4):
            gd.stream_init(s)
        log = []
        for call in calls:
            if many:
                gd.streams_push([k for k, _, _ in call], [xs[k][lo:hi] for k, lo, hi in call])
            else:
                for k, lo, hi in call:
                    gd.stream_push(k, xs[k][lo:hi])
            log.append([(gd.stream_partial(s)[1], gd.stream_collect_info(s), gd.stream_path_counts(s)) for s in range(4)])
        for s in range(4):
            g = gd.stream_finish(s)
            log.append((g.n, g.label.tobytes(), g.time.tobytes(), g.score.view(np.uint32).tobytes(), gd.stream_partial(s)[1]))
        trail.append(log)
        gd.close()
    assert len(trail[0]) == len(trail[1])
    for i, (a, b) in enumerate(zip(trail[0], trail[1])):
        assert a == b, "call %d" % i


def test_one_trace_launch_per_round(small_tree, tree_inputs):
    """Four streams pushed the same 64 frames per call: the call with frame 100 in it traces all four with ONE launch, a call
    without a collect frame is one search launch and no trace."""
    from juicer_amd import capi
    gnet, gam = small_tree[:2]
    xs, ora = tree_inputs
    assert all(o[2][0] == 100 for o in ora[1])                         # (the oracle: every stream collects after frame 100 first)
    gd = capi.Decoder(gnet, gam, max_streams=4, main_beam=150.0)
    gd.set_partial_interval(1)
    for s in range(4):
        gd.stream_init(s)
    t0 = gd.last_timing()
    gd.streams_push(range(4), [x[0:64] for x in xs])
    t1 = gd.last_timing()
    assert t1["trace_launches"] - t0["trace_launches"] == 0
    assert t1["search_launches"] - t0["search_launches"] == 1
    gd.streams_push(range(4), [x[64:128] for x in xs])
    t2 = gd.last_timing()
    assert t2["trace_launches"] - t1["trace_launches"] == 1
    for s in range(4):
        assert gd.stream_collect_info(s) == (1, 100)
        assert gd.stream_partial(s)[1] == ora[1][s][0][100][1]
    gd.close()


def test_broker_partial(small_tree, tree_inputs):
    """A broker on a decoder with an interval: the tick worker, and every client's list as the oracle has it - one of its
    snapshots at any moment, growing, never ahead of what the client has pushed, complete after finish."""
    from juicer_amd import capi
    gnet, gam = small_tree[:2]
    xs, ora = tree_inputs
    dec = capi.Decoder(gnet, gam, max_streams=3, main_beam=150.0)
    dec.set_partial_interval(150)
    broker = capi.Broker(dec, 3)
    seen = [[] for _ in range(3)]
    errs = []

    def run(c):
        try:
            cl = broker.open()
            broker.init(cl)
            x = xs[c]
            seen[c].append((0, broker.partial(cl)))
            for pos in range(0, x.shape[0], 50):
                broker.push(cl, x[pos:pos + 50])
                seen[c].append((min(x.shape[0], pos + 50), broker.partial(cl)))
            g = broker.finish(cl)
            seen[c].append((None, broker.partial(cl), _hyp_list(g)))
            broker.close_client(cl)
        except Exception as e:  # noqa: BLE001
            errs.append(e)

    th = [threading.Thread(target=run, args=(c,)) for c in range(3)]
    for t in th:
        t.start()
    for t in th:
        t.join()
    assert not errs, errs
    assert broker.stats()["resident"] == 0
    for c in range(3):
        snaps, final, _ = ora[150][c]
        allowed = [[]] + [snaps[f][1] for f in sorted(snaps)]
        prev = []
        for pushed, lst in seen[c][:-1]:
            assert lst in allowed, (c, pushed)
            assert len(lst) >= len(prev) and lst[:len(prev)] == prev
            assert all(t < pushed for _, t in lst)
            prev = lst
        assert seen[c][-1][1] == final == seen[c][-1][2]
    broker.close()
    dec.close()


def test_batch_test_threads_partial_lines(small, tmp_path):
    """jd_batch_test -threads 2 with PartialTraceInterval=50: one 'Partial paths recovered at frames:' line per utterance, in list
    order, each the utterance's word-end frames, and the output of the run without the variable."""
    import subprocess
    from juicer_amd import build as jbuild, io as jio, synth
    from oracle.oracle import OracleDecoder
    gnet, gam, onet, oam, feats, _ = small
    am, net, _, _ = synth.config_small()
    jio.write_fsm(tmp_path / "g.fsm", net)
    jio.write_jdam(tmp_path / "m.jdam", am)
    with open(tmp_path / "list.txt", "w") as f:
        for u, x in enumerate(feats):
            jio.write_jdf(tmp_path / ("u%d.jdf" % u), x)
            f.write("%s\n" % (tmp_path / ("u%d.jdf" % u)))
    od = OracleDecoder(onet, oam, main_beam=150.0, max_hyps=200)
    want = [od.decode_certified(x) for x in feats]
    cmd = [jbuild.BATCH_TEST, "-fsmFName", str(tmp_path / "g.fsm"), "-modelsFName", str(tmp_path / "m.jdam"), "-inputFName", str(tmp_path / "list.txt"),
           "-mainBeam", "150", "-maxHyps", "200", "-outputFormat", "xmlf", "-threads", "2"]
    env = {k: v for k, v in os.environ.items() if k != "PartialTraceInterval"}
    plain = subprocess.run(cmd, capture_output=True, text=True, timeout=240, env=env)
    assert plain.returncode == 0, plain.stderr
    assert "Partial paths recovered" not in plain.stderr
    part = subprocess.run(cmd, capture_output=True, text=True, timeout=240, env=dict(env, PartialTraceInterval="50"))
    assert part.returncode == 0, part.stderr
    assert part.stdout == plain.stdout
    lines = [ln for ln in part.stderr.splitlines() if ln.startswith("Partial paths recovered at frames:")]
    assert len(lines) == len(feats)
    for u, ln in enumerate(lines):
        assert [int(v) for v in ln.split(":", 1)[1].split()] == want[u].time[::-1].tolist(), u


def test_first_trace_beyond_the_staging_share(small):
    """A stream's first trace late in a long input has more new records than its share of k_partial_many's staging area (32): they
    come from its result arrays instead, while the stream beside it, traced all along, goes through the staging area - both
    lists are the oracle's."""
    from juicer_amd import capi
    from oracle.oracle import OracleDecoder
    gnet, gam, onet, oam, feats, _ = small
    kw = dict(main_beam=150.0, max_hyps=200)
    od = OracleDecoder(onet, oam, **kw)
    x = np.concatenate(feats)
    late = x.shape[0] - 40
    at = list(range(150, late, 150)) + [late]
    snaps_late = od.decode_partial(x, interval=0, trace_at=[late])[0]
    snaps_all = od.decode_partial(x, interval=0, trace_at=at)[0]
    assert snaps_late[late][0] and len(snaps_late[late][1]) > 32
    assert all(len(snaps_all[b][1]) - len(snaps_all[a][1]) <= 32 for a, b in zip(at, at[1:]))
    gd = capi.Decoder(gnet, gam, max_streams=2, **kw)
    gd.stream_init(0); gd.stream_init(1)
    pos = 0
    for f in at:
        gd.streams_push([0, 1], [x[pos:f + 1], x[pos:f + 1]])
        pos = f + 1
        found = gd.streams_trace([1] if f != late else [1, 0])
        assert (found[0], gd.stream_partial(1)[1]) == snaps_all[f]
    assert (found[1], gd.stream_partial(0)[1]) == snaps_late[late]
    gd.close()


def test_refusals_kept(small):
    from juicer_amd import capi
    gnet, gam, _, _, feats, _ = small
    dec = capi.Decoder(gnet, gam, max_streams=2, main_beam=150.0)
    dec.stream_init(0); dec.stream_init(1)
    dec.streams_push([0, 1], [feats[0][:30], feats[1][:30]])
    with pytest.raises(capi.JuicerAmdError) as e:
        dec.streams_trace([0, 0])
    assert e.value.code == capi.JD_EINVAL
    assert dec.streams_trace([]) == []
    dec.stream_finish(0); dec.stream_finish(1)
    dec.set_partial_interval(50)
    with pytest.raises(capi.JuicerAmdError):
        dec.set_output_level(capi.OUTPUT_WORDS | capi.OUTPUT_MODELS)
    dec.set_partial_interval(0)
    dec.set_output_level(capi.OUTPUT_WORDS | capi.OUTPUT_MODELS)
    dec.stream_init(0)
    dec.stream_push(0, feats[0][:30])
    with pytest.raises(capi.JuicerAmdError) as e:
        dec.streams_trace([0])
    assert e.value.code == capi.JD_ESTATE
    assert dec.stream_partial(0, trace_now=True)[0] in (False, True)   # (the single-stream call remains)
    dec.stream_finish(0)
    dec.close()
