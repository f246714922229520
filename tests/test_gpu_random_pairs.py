"""Device composition on C.L and G pairs of ARBITRARY shape (tests/random_pairs.py): jd_net_compose against the Python references
bit for bit, at exactly enough and one too few states and arcs, and jd_net_create_lazy against the static search on the composed
graph, itself against the CPU oracle.  Every other composition test builds its pair with synth.make_cl_g - a lexicon prefix tree
and a back-off n-gram, whose C.L states have at most a few dozen arcs - so these are the only ones in which the expansion step
(jc_expand, csrc/jd_compose.hip; lz_expand, csrc/jd_lazy.h) goes round its 64-arc chunk loop more than once, G is a real
transducer, look-ahead entries are "every label" or empty, and so on: tests/test_random_pairs_cpu.py asserts each of these shapes
from the arrays, and that the references accept the weighted language of textbook composition on the same pairs."""
import numpy as np
import pytest

import random_pairs as rp
from compose_ref import compose_naive
from helpers import STAT_KEYS, assert_hyp_matches

pytestmark = pytest.mark.gpu

IDS = [name for name, _ in rp.PAIRS]
_memo = {}


def _pair(name):
    """(pair, C.L network, G network, {mask: reference arrays}) - computed once, shared by the tests, never changed"""
    if name not in _memo:
        p = rp.random_pair(**dict(rp.PAIRS)[name])
        ncl, ng = rp.networks(p)
        _memo[name] = (p, ncl, ng, {m: rp.reference(p, m) for m in rp.MASKS})
    return _memo[name]


def _compose(ncl, ng, mask, **kw):
    from juicer_amd import capi
    return capi.Network.compose(ncl, ng, pushing=bool(mask & 1), push_labels=bool(mask & 2), lookahead_sets=bool(mask & 4), **kw)


def _assert_arrays(net, want, what):
    got = net.csr()
    assert net.n_states == want["n_states"] and net.init_state == want["init"], what
    for k in ("row_ptr", "to", "ilab", "olab"):
        assert np.array_equal(got[k], want[k]), (what, k)
    for k in ("w", "fin_w"):
        assert np.array_equal(got[k].view(np.uint32), np.asarray(want[k], np.float32).view(np.uint32)), (what, k)
    return got


@pytest.mark.parametrize("name", IDS)
def test_composed_arrays_equal_the_references(built, name):
    """Masks 0-5 (weights, labels, sets and their combinations): the arrays of the Python reference, bit for bit; and a second
    composition, with little room, gives the same arrays (nothing depends on discovery order or table size)."""
    p, ncl, ng, refs = _pair(name)
    for m in rp.MASKS:
        got = _assert_arrays(_compose(ncl, ng, m), refs[m], (name, m))
        again = _compose(ncl, ng, m, max_states=4 * refs[m]["n_states"], max_arcs=2 * len(refs[m]["to"])).csr()
        assert all(np.array_equal(again[k].view(np.uint32), got[k].view(np.uint32)) for k in got), (name, m)


@pytest.mark.parametrize("name", IDS)
def test_exact_capacities(built, name):
    """max_states / max_arcs are inclusive bounds (jc_state_id, jc_expand): exactly the composed size succeeds with the same arrays,
    one state or one arc less is JD_ENOMEM, naming what ran out."""
    from juicer_amd import capi
    p, ncl, ng, refs = _pair(name)
    for m in (0, 5):
        N, M = refs[m]["n_states"], len(refs[m]["to"])
        _assert_arrays(_compose(ncl, ng, m, max_states=N, max_arcs=M), refs[m], (name, m, "exact"))
        with pytest.raises(capi.JuicerAmdError) as ei:
            _compose(ncl, ng, m, max_states=N - 1, max_arcs=M)
        assert ei.value.code == capi.JD_ENOMEM and "states" in str(ei.value), (name, m)
        with pytest.raises(capi.JuicerAmdError) as ei:
            _compose(ncl, ng, m, max_states=N, max_arcs=M - 1)
        assert ei.value.code == capi.JD_ENOMEM and "arcs" in str(ei.value), (name, m)


def _same_hyp(a, b, what):
    assert a.n == b.n and np.array_equal(a.label, b.label) and np.array_equal(a.time, b.time), what
    for k in ("score", "ac", "lm", "tot_score", "tot_ac", "tot_lm"):
        assert np.array_equal(np.asarray(getattr(a, k), np.float32).view(np.uint32), np.asarray(getattr(b, k), np.float32).view(np.uint32)), (what, k)


@pytest.mark.parametrize("name", [n for n, _ in rp.DECODABLE])
def test_search_driven_composition(built, name):
    """On the decodable pairs, for every mask: the static search on the device-composed graph equals the CPU oracle on the same
    arrays; the search-driven composition decodes bit-identically to it - three streams growing the shared network at once, then a
    second batch on the grown one - and never holds more than the composed graph; a last batch with nothing pruned shows that the
    network holds a row at the hub (65 / 129 / 150 C.L arcs: the later trips of lz_expand's chunk loop)."""
    from juicer_amd import capi
    from oracle.oracle import OracleAM, OracleDecoder
    p, ncl, ng, refs = _pair(name)
    am = rp.models(p["seed"])
    models, oam = capi.Models.from_htk(am), OracleAM(am)
    feats = rp.utterances(name, compose_naive(p["cl"], p["cl_init"], p["g"], p["g_init"]), am)
    kw = dict(max_streams=3, **rp.BEAMS)
    for m in rp.MASKS:
        static = _compose(ncl, ng, m)
        _assert_arrays(static, refs[m], (name, m))
        want = capi.Decoder(static, models, **kw).decode_batch(feats)
        od = OracleDecoder(rp.oracle_net(refs[m]), oam, **rp.BEAMS)
        for u, x in enumerate(feats):
            o = od.decode_certified(x)
            what = "%s mask %d utt %d" % (name, m, u)
            assert o.n > 0, what
            assert_hyp_matches(want[u], o, what, check_stats=False)
            for k in STAT_KEYS:
                assert want[u].stats[k] == o.stats[k], (what, k)
        lazy = capi.Network.lazy(ncl, ng, models, max_states=1 << 14, max_arcs=1 << 16, pushing=bool(m & 1), push_labels=bool(m & 2),
                                 lookahead_sets=bool(m & 4))
        dec = capi.Decoder(lazy, models, **kw)
        got = dec.decode_batch(feats[:3])
        s1 = lazy.lazy_size()
        got += dec.decode_batch(feats[3:])
        s2 = lazy.lazy_size()
        for u in range(len(feats)):
            _same_hyp(got[u], want[u], "%s mask %d utt %d" % (name, m, u))
        assert 0 < s1[0] <= s2[0] <= static.n_states and s1[1] <= s2[1] <= static.n_arcs, (name, m, s1, s2)
        dec.close()
        # lz_expand has been round its chunk loop at the hub: with nothing pruned the network grows to more arcs than the
        # composed graph has outside the rows of its states at the hub - so at least one of those rows is in it - and the
        # results are still the static search's, bit for bit
        wide = dict(max_streams=3, main_beam=0.0)
        want0 = capi.Decoder(static, models, **wide).decode_batch(feats[:3])
        dec0 = capi.Decoder(lazy, models, **wide)
        got0 = dec0.decode_batch(feats[:3])
        for u in range(3):
            _same_hyp(got0[u], want0[u], "%s mask %d utt %d, nothing pruned" % (name, m, u))
        s3 = lazy.lazy_size()
        rows = np.diff(refs[m]["row_ptr"])
        at_hub = int(sum(rows[i] for i, k in enumerate(refs[m]["keys"]) if k[0] == p["hub"])) if p["hub"] is not None else 0
        print("%s mask %d: lazy %s -> %s -> %s of %d states %d arcs; %d arcs in rows at the hub"
              % (name, m, s1, s2, s3, static.n_states, static.n_arcs, at_hub))
        assert s2[0] <= s3[0] <= static.n_states and s2[1] <= s3[1] <= static.n_arcs, (name, m, s2, s3)
        if p["hub"] is not None:
            assert at_hub > 0 and s3[1] > static.n_arcs - at_hub, (name, m, s3, static.n_arcs, at_hub)
        dec0.close()
