"""CPU side of the composition tests on C.L and G pairs of ARBITRARY shape (tests/random_pairs.py) - the pairs
tests/test_gpu_random_pairs.py holds jd_net_compose and jd_net_create_lazy to.  Three things are settled here, without a device:

  1. the references themselves are right on such pairs: compose_filtered (plain, pushing, on the label-pushed C.L) and compose_sets
     (plain, pushing) accept the weighted language of textbook composition (compose_naive) - the arbiter if a device test disagrees;
  2. the library's HOST code agrees with Python on them: jd_net_push_labels, jd_debug_cl_label_sets, jd_debug_cl_lookahead;
  3. the fixtures are what they claim to be: every shape the generator has a knob for is asserted from the arrays (row widths, list
     lengths, labels moved, a final composed state with f = 0, ...), and the decodable pairs' utterances decode to the same words on
     the textbook and the filtered composition, with words, and without order-dependent ties under any option mask."""
import numpy as np
import pytest

import random_pairs as rp
from compose_ref import _best, _lookahead, compose_naive, push_labels
from compose_sets_ref import dfs_numbering, label_sets
from helpers import rel_close

N_SEQ = 40
IDS = [name for name, _ in rp.PAIRS]
_memo = {}


@pytest.fixture(scope="module")
def lib_built():
    from juicer_amd import build as jbuild
    jbuild.build()
    return True


def _pair(name):
    if name not in _memo:
        p = rp.random_pair(**dict(rp.PAIRS)[name])
        rp.check_rules(p)
        _memo[name] = (p, compose_naive(p["cl"], p["cl_init"], p["g"], p["g_init"]))
    return _memo[name]


def _language(name):
    """(sequences accepted by the textbook composition, sequences) - after checking every reference against it"""
    if ("lang", name) not in _memo:
        p, naive = _pair(name)
        graphs = {m: rp.reference(p, m) for m in rp.MASKS}
        accepted = 0
        for ws in rp.sample_sequences(p["seed"], naive, N_SEQ):
            a = _best(naive, ws)
            accepted += bool(np.isfinite(a))
            for m, gr in graphs.items():
                b = _best(gr, ws)
                assert np.isfinite(a) == np.isfinite(b), (name, m, ws, a, b)   # accepted by both or by neither
                if np.isfinite(a):
                    assert abs(a - b) <= 1e-3 * max(1.0, abs(a)), (name, m, ws, a, b)
        _memo[("lang", name)] = (accepted, N_SEQ)
    return _memo[("lang", name)]


@pytest.mark.parametrize("name", IDS)
def test_references_accept_the_textbook_language(name):
    accepted, n = _language(name)
    print("%s: %d of %d sampled sequences accepted" % (name, accepted, n))
    assert accepted >= 1


def test_most_sampled_sequences_are_accepted():
    got = [_language(name) for name in IDS]
    accepted, n = sum(a for a, _ in got), sum(k for _, k in got)
    print("accepted %d of %d sampled sequences; fewest in a pair: %d of %d" % (accepted, n, min(a for a, _ in got), N_SEQ))
    assert 2 * accepted >= n


def _list_states(cl, cl_init):
    """{state: set size} of the C.L states whose label set is no interval under the library's word numbering"""
    num = dfs_numbering(cl, cl_init)
    sets, _ = label_sets(cl)
    out = {}
    for c, s in enumerate(sets):
        if s:
            x = sorted(num[l] for l in s)
            if x[-1] - x[0] + 1 != len(x): out[c] = len(x)
    return out, num


@pytest.mark.parametrize("name", IDS)
def test_pairs_have_the_shapes_they_are_there_for(name):
    kw = dict(rp.PAIRS)[name]
    p, naive = _pair(name)
    cl, g = p["cl"], p["g"]
    wid, gwid = rp.row_widths(cl), rp.row_widths(g)
    src = np.repeat(np.arange(len(wid)), wid)
    gsrc = np.repeat(np.arange(len(gwid)), gwid)
    lo, hi, mf = _lookahead(cl)
    f0 = rp.reference(p, 0)
    if kw.get("hub_width"):
        hub = p["hub"]
        assert wid[hub] == kw["hub_width"] and wid.max() == wid[hub]
        # a composed state at the hub, reached, that keeps some and drops some of the hub's arcs in every 64-arc chunk (but a short
        # last one): the survivors straddle the chunk edges
        a0 = int(cl["row_ptr"][hub])
        glabels = [set(g["ilab"][g["row_ptr"][s]:g["row_ptr"][s + 1]].tolist()) - {0} for s in range(len(gwid))]

        def survives(a, gs):
            o, t = int(cl["olab"][a]), int(cl["to"][a])
            if o: return o in glabels[gs]
            return any(lo[t] <= x <= hi[t] for x in glabels[gs]) or (mf[t] and bool(np.isfinite(g["fin_w"][gs])))
        rows = {k: int(f0["row_ptr"][i + 1] - f0["row_ptr"][i]) for i, k in enumerate(f0["keys"]) if k[0] == hub}
        straddle = 0
        for (c, gs, f), n in rows.items():
            keep = np.asarray([survives(a0 + j, gs) for j in range(wid[hub])])
            bo = f == 1 and 0 in g["ilab"][g["row_ptr"][gs]:g["row_ptr"][gs + 1]]
            assert n == keep.sum() + int(bo)
            chunks = [keep[j:j + 64] for j in range(0, len(keep), 64)]
            straddle += all(ch.any() and not ch.all() for ch in chunks if len(ch) >= 8) and keep[min(63, len(keep) - 1)::64].any()
        assert straddle > 0
        if wid[hub] >= 128:
            assert max(rows.values()) > 64 or kw.get("sparse")          # (a composed row wider than a wave: jc_place's second trip)
    if kw.get("transducer"):
        assert (g["olab"] != g["ilab"]).any() and (g["olab"][g["ilab"] != 0] == 0).any()
        assert set(f0["olab"].tolist()) - set(cl["olab"].tolist())    # composed arcs carry labels only G's output side has
    if kw.get("less_cycles"):
        assert any(lo[c] == 1 and hi[c] == 2 ** 31 - 1 for c in range(len(lo)))
    if kw.get("dead_ends"):
        assert all(wid[c] == 0 and lo[c] > hi[c] and not mf[c] for c in p["dead"])
        assert wid[p["term"]] == 0 and lo[p["term"]] > hi[p["term"]] and mf[p["term"]]
        assert all((cl["olab"][cl["to"] == c] == 0).any() for c in p["dead"] + [p["term"]])   # behind a label-less arc
    # LA_MAYFIN through a final state that has arcs, weighted
    nonterm = [c for c in range(len(wid)) if np.isfinite(cl["fin_w"][c]) and wid[c] > 0 and cl["fin_w"][c] != 0.0]
    assert nonterm and any(cl["olab"][a] == 0 and cl["to"][a] in nonterm for a in range(len(src)))
    # G: a state without arcs, one with the back-off only, a back-off chain three deep, all reached from arcs
    assert gwid[1] == 0 and gwid[2] == 1 and g["ilab"][g["row_ptr"][2]] == 0 and 1 in g["to"] and 2 in g["to"]
    for m in (0, 4):                                                    # ... and composed states stand at both (keys: (c, g, f), sets: (c, f, g))
        at = [k[2 if m else 1] for k in rp.reference(p, m)["keys"]]
        assert 1 in at and 2 in at
    bo = {int(gsrc[a]): int(g["to"][a]) for a in range(len(gsrc)) if g["ilab"][a] == 0}
    assert 4 in bo and bo[4] in bo and bo[bo[4]] in bo
    deep = [s for s in bo if bo[s] in bo and bo[bo[s]] in bo]
    assert any(k[2] == 1 and k[1] in deep and k[0] != p["cl_init"] for k in f0["keys"])   # entered at f = 1 away from C.L's initial state
    # words only one side knows; arcs into both initial states
    assert set(cl["olab"].tolist()) - set(g["ilab"].tolist()) - {0} and set(g["ilab"].tolist()) - set(cl["olab"].tolist()) - {0}
    assert p["cl_init"] in cl["to"] and p["g_init"] in g["to"]
    # a FINAL composed state with f = 0 (whose final weight weight pushing has to correct)
    assert any(k[2] == 0 and np.isfinite(f0["fin_w"][i]) for i, k in enumerate(f0["keys"]))
    moved = push_labels(cl, p["cl_init"])[1]
    if kw.get("sparse"):
        assert moved > 0
    if kw.get("wide_sets"):
        lists, num = _list_states(cl, p["cl_init"])
        B = p["list_state"]
        assert lists.get(B, 0) > 64 and (gwid[p["g_init"]] >= 200 or kw["wide_sets"] == 2)
        assert any(cl["to"][a] == B and cl["olab"][a] == 0 for a in range(cl["row_ptr"][p["cl_init"]], cl["row_ptr"][p["cl_init"] + 1]))
        # the list test at the start state is long on both sides (LA_WAVE_MIN = 32, csrc/jd_lazy.h): the wave does it
        sets, _ = label_sets(cl)
        nb = sorted(num[l] for l in sets[B])
        row = g["ilab"][g["row_ptr"][p["g_init"]]:g["row_ptr"][p["g_init"] + 1]]
        inside = sum(1 for l in row.tolist() if l in num and nb[0] <= num[l] <= nb[-1])
        assert min(len(nb), inside) > 32
        assert len(nb) <= inside if kw["wide_sets"] == 1 else len(nb) > inside     # which side la_set_wave walks: the list / G's arcs
    print("%s: C.L %d states, widest row %d; G widest row %d; composed %d states %d arcs (textbook %d / %d); %d labels moved"
          % (name, len(wid), wid.max(), gwid.max(), f0["n_states"], len(f0["to"]), naive["n_states"], len(naive["to"]), moved))
    assert 20 <= f0["n_states"] <= 1000 and len(f0["to"]) <= 10000


@pytest.mark.parametrize("name", IDS)
def test_host_code_matches_python(lib_built, name):
    """jd_net_push_labels, jd_debug_cl_label_sets and jd_debug_cl_lookahead (host code of the library, no device) on these pairs"""
    p, _ = _pair(name)
    ncl, _ng = rp.networks(p)
    cl = ncl.csr()
    for k in ("row_ptr", "to", "ilab", "olab"):
        assert np.array_equal(cl[k], p["cl"][k]), k
    assert np.array_equal(cl["w"].view(np.uint32), p["cl"]["w"].view(np.uint32))
    assert np.array_equal(cl["fin_w"].view(np.uint32), p["cl"]["fin_w"].view(np.uint32))
    # look-ahead intervals
    lo, hi, mf = ncl.lookahead()
    wl, wh, wm = _lookahead(p["cl"])
    assert lo.tolist() == wl and hi.tolist() == wh and mf.tolist() == wm
    # label pushing
    pushed, moved = ncl.push_labels()
    want, want_moved = push_labels(p["cl"], p["cl_init"])
    assert np.array_equal(pushed.csr()["olab"], want) and moved == want_moved
    # label sets
    rpt, labels, smf = ncl.label_sets()
    sets, want_mf = label_sets(p["cl"])
    assert [labels[rpt[c]:rpt[c + 1]].tolist() for c in range(ncl.n_states)] == [[-1] if s is None else sorted(s) for s in sets]
    assert smf.tolist() == want_mf == wm


@pytest.mark.parametrize("name", [n for n, _ in rp.DECODABLE])
def test_decodable_pairs_utterances(name):
    """The utterances the GPU test decodes: the CPU oracle on the textbook composition and on compose_filtered's arrays finds the
    same words at the same times, acoustic and language-model totals within helpers.rel_close (nothing is pruned; the path scores
    are normalised by every frame's best token, which a dead end may be on the textbook graph: not comparable), every utterance
    has words, and under every option mask the oracle's result on the reference arrays does not hang on the order of equal scores."""
    from oracle.oracle import OracleAM, OracleDecoder
    p, naive = _pair(name)
    am = rp.models(p["seed"])
    oam = OracleAM(am)
    assert rp.UTTS[name] == rp.find_utterances(name)                    # (the selection can be made again from the file)
    feats = rp.utterances(name, naive, am)
    assert len(feats) == 6
    wide = [OracleDecoder(rp.oracle_net(gr), oam, main_beam=0.0) for gr in (naive, rp.reference(p, 0))]
    for u, x in enumerate(feats):
        a, b = wide[0].decode(x), wide[1].decode(x)
        assert a.n > 0 and a.n == b.n, (name, u)
        assert np.array_equal(a.label, b.label) and np.array_equal(a.time, b.time), (name, u)
        assert rel_close(a.tot_ac, b.tot_ac) and rel_close(a.tot_lm, b.tot_lm) and rel_close(a.ac, b.ac), (name, u)
    for m in rp.MASKS:
        od = OracleDecoder(rp.oracle_net(rp.reference(p, m)), oam, **rp.BEAMS)
        for u, x in enumerate(feats):
            assert od.decode_certified(x).n > 0, (name, m, u)
