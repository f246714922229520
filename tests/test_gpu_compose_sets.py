"""Label-set look-ahead (JD_LOOKAHEAD_SETS, include/juicer_amd.h) on the device: jd_net_compose and jd_net_create_lazy with the
bit against tests/compose_sets_ref.py (Python sets, naive composition) and against the interval look-ahead where the two are the
same thing - the generator's own word numbering.  tests/test_compose_sets_cpu.py holds the host-side set computation to the same
reference without a device."""
import subprocess

import numpy as np
import pytest

from compose_sets_ref import add_variants, compose_sets, dfs_numbering, label_sets, permute_words, random_perm
from helpers import rel_close

pytestmark = pytest.mark.gpu

CASES = [dict(seed=5, n_words=40, n_succ=4, n_tri=30, with_sp=True, lm=1.0),
         dict(seed=6, n_words=60, n_succ=4, n_tri=0, with_sp=False, lm=7.5)]
KEYS = ("row_ptr", "to", "ilab", "olab", "w", "fin_w")
_memo = {}


def _am(c):
    from juicer_amd import synth
    k = ("am", c["seed"], c["with_sp"])
    if k not in _memo:
        _memo[k] = synth.make_models(c["seed"], n_gmm=100, n_hmm=45, n_mix=2, n_tm=8, sep=0.6, with_tee=c["with_sp"])
    return _memo[k]


def _pair(c, n_words=None):
    from juicer_amd import synth
    return synth.make_cl_g(c["seed"], _am(c), n_words=n_words or c["n_words"], n_succ=c["n_succ"], n_tri=c["n_tri"], with_sp=c["with_sp"])


def _nets(c, cl, g):
    from juicer_amd import capi
    return capi.Network.from_synth(cl, 1.0, 0.0), capi.Network.from_synth(g, c["lm"], 0.0)


def _arrays(net):
    a = net.csr()
    return dict(n_states=net.n_states, init=net.init_state, **{k: a[k] for k in KEYS})


def _same_arrays(a, b):
    """bit for bit, weights included"""
    assert a["n_states"] == b["n_states"] and a["init"] == b["init"]
    for k in ("row_ptr", "to", "ilab", "olab"):
        assert np.array_equal(a[k], b[k]), k
    for k in ("w", "fin_w"):
        assert np.array_equal(np.asarray(a[k], np.float32).view(np.uint32), np.asarray(b[k], np.float32).view(np.uint32)), k


def _compose(ncl, ng, mask):
    from juicer_amd import capi
    return capi.Network.compose(ncl, ng, pushing=bool(mask & 1), push_labels=bool(mask & 2), lookahead_sets=bool(mask & 4))


def _lists(ncl):
    """the states of C.L whose label set is NOT an interval under the library's internal word numbering (the order in which a
    depth-first walk from the initial state first meets the words): the ones that carry a label list on the device.
    {state: set size}"""
    csr = ncl.csr()
    num = dfs_numbering(csr, ncl.init_state)
    rp, labels, _ = ncl.label_sets()
    out = {}
    for c in range(ncl.n_states):
        s = labels[rp[c]:rp[c + 1]]
        if len(s) and s[0] != -1:
            x = sorted(num[int(l)] for l in s)
            if x[-1] - x[0] + 1 != len(x):
                out[c] = len(x)
    return out


def _same_hyp(a, b):
    assert a.n == b.n and np.array_equal(a.label, b.label) and np.array_equal(a.time, b.time)
    for k in ("score", "ac", "lm"):
        assert np.array_equal(np.asarray(getattr(a, k), np.float32).view(np.uint32), np.asarray(getattr(b, k), np.float32).view(np.uint32)), k


@pytest.mark.parametrize("mask", [0, 1, 2, 3])
@pytest.mark.parametrize("c", CASES, ids=lambda c: "seed%d" % c["seed"])
def test_sets_equal_intervals_on_the_generators_numbering(built, c, mask):
    """1. The generator numbers the words in the tree's depth-first order: the sets ARE the intervals, and the composed arrays
    with the bit are those without it, bit for bit."""
    cl, g = _pair(c)
    ncl, ng = _nets(c, cl, g)
    assert _lists(ncl) == {}
    _same_arrays(_arrays(_compose(ncl, ng, mask | 4)), _arrays(_compose(ncl, ng, mask)))


@pytest.mark.parametrize("mask", [0, 1], ids=["plain", "weights"])
@pytest.mark.parametrize("c", CASES, ids=lambda c: "seed%d" % c["seed"])
def test_composition_does_not_depend_on_the_word_numbering(built, c, mask):
    """2. With the bit, a renumbered vocabulary composes into the arrays the generator's numbering gives (C.L's input labels and G's
    output labels, the ones a composed graph carries, are not renumbered: nothing to map back); without it the intervals of a
    renumbered vocabulary let dead-end branches through - strictly more states."""
    cl, g = _pair(c)
    want = _arrays(_compose(*_nets(c, cl, g), mask))
    for k in range(3):
        pcl, pg = permute_words(cl, g, random_perm(cl, g, 100 * c["seed"] + k))
        ncl, ng = _nets(c, pcl, pg)
        _same_arrays(_arrays(_compose(ncl, ng, mask | 4)), want)
        loose = _compose(ncl, ng, mask)
        print("seed %d perm %d mask %d: %d states with sets, %d with intervals" % (c["seed"], k, mask, want["n_states"], loose.n_states))
        assert loose.n_states > want["n_states"]


def _variants(c, n_words=None, host=None):
    """(cl, g): a second pronunciation elsewhere in the tree for every fifth word - or, with host, for half the vocabulary below ONE
    tree node, whose list (and its ancestors') is then longer than a wave is wide"""
    cl, g = _pair(c, n_words)
    V = cl.n_words
    words = list(range(3, V, 5)) if host is None else [w for w in range(0, V, 2) if cl.prons[w][0] != cl.prons[host][0]]
    return add_variants(cl, _am(c), words, seed=7 + c["seed"], host=host), g


@pytest.mark.parametrize("mask", [0, 1], ids=["plain", "weights"])
@pytest.mark.parametrize("fix", ["seed5", "seed6", "long"])
def test_sets_that_are_no_interval(built, fix, mask):
    """3. Pronunciation variants: sets that are contiguous under no numbering go through the label lists - the arrays are those of
    the naive composition on Python sets.  "long": 200 words, half of them with a variant below the LAST first-level tree node
    (the walk that numbers the words has met them all before), so that the list tested against the unigram state's 200 arcs is
    longer than 64 labels: the wave-cooperative path."""
    c = CASES[0] if fix != "seed6" else CASES[1]
    cl, g = _variants(c, 200, host=199) if fix == "long" else _variants(c)
    ncl, ng = _nets(c, cl, g)
    lists = _lists(ncl)
    assert len(lists) > 0
    if fix == "long":
        csr = ncl.csr()
        first_level = set(int(t) for t in csr["to"][csr["row_ptr"][ncl.init_state]:csr["row_ptr"][ncl.init_state + 1]])
        assert max(lists.get(s, 0) for s in first_level) > 64
        grow = np.diff(ng.csr()["row_ptr"])
        assert grow.max() >= 200
    want = compose_sets(ncl.csr(), ncl.init_state, ng.csr(), ng.init_state, pushing=bool(mask & 1))
    _same_arrays(_arrays(_compose(ncl, ng, mask | 4)), want)


@pytest.fixture(scope="module")
def decoding(built):
    """the variants fixture, renumbered: networks, three utterances, and the hypotheses on the sets-composed graph"""
    from juicer_amd import capi, synth
    c = CASES[0]
    cl, g = _variants(c)
    pcl, pg = permute_words(cl, g, random_perm(cl, g, 31))
    ncl, ng = _nets(c, pcl, pg)
    models = capi.Models.from_htk(_am(c))
    feats = [synth.sample_utterance(c["seed"] + 1000 + u, g, _am(c), 6 + u)[0] for u in range(3)]
    hyps = {}
    for mask in (0, 1):
        dev = _compose(ncl, ng, mask | 4)
        hyps[mask] = (dev, capi.Decoder(dev, models, max_streams=3, main_beam=400.0).decode_batch(feats))
    return dict(c=c, cl=pcl, g=pg, ncl=ncl, ng=ng, models=models, feats=feats, hyps=hyps)


@pytest.mark.parametrize("mask", [0, 1], ids=["plain", "weights"])
def test_decoding_composed_and_lazy(decoding, mask):
    """4. The static search on the sets-composed graph == the CPU oracle on the same arrays; the search-driven composition with the
    bit decodes to the same hypotheses bit for bit, and expands fewer states than the interval look-ahead does on this
    (renumbered) vocabulary."""
    from juicer_amd import capi
    from oracle.oracle import OracleAM, OracleDecoder, OracleNet
    d = decoding
    dev, gs = d["hyps"][mask]
    a = dev.csr()
    fs = np.nonzero(np.isfinite(a["fin_w"]))[0].astype(np.int32)
    onet = OracleNet.from_csr(dev.n_states, dev.init_state, a["row_ptr"], a["to"], a["w"], a["ilab"], a["olab"], fs, a["fin_w"][fs])
    od = OracleDecoder(onet, OracleAM(_am(d["c"])), main_beam=400.0)
    for u, x in enumerate(d["feats"]):
        o = od.decode(x)
        assert gs[u].n == o.n and o.n > 0
        assert np.array_equal(gs[u].label, o.label) and np.array_equal(gs[u].time, o.time)
        assert rel_close(gs[u].score, o.score) and rel_close(gs[u].ac, o.ac) and rel_close(gs[u].lm, o.lm) and rel_close(gs[u].tot_score, o.tot_score)
    size = {}
    for bit in (4, 0):
        lz = capi.Network.lazy(d["ncl"], d["ng"], d["models"], max_states=1 << 16, max_arcs=1 << 18, pushing=bool(mask & 1), lookahead_sets=bool(bit))
        ls = capi.Decoder(lz, d["models"], max_streams=3, main_beam=400.0).decode_batch(d["feats"])
        size[bit] = lz.lazy_size()
        if bit:
            for u in range(3):
                _same_hyp(ls[u], gs[u])
    print("lazy size with sets", size[4], "with intervals", size[0])
    assert size[4][0] < size[0][0] and size[4][1] < size[0][1]


def test_lazy_life_cycle(decoding):
    """5. The renumbered G and the label lists belong to the network: they survive jd_net_lazy_reset and a generation the network
    starts by itself (high-water mark)."""
    from juicer_amd import capi
    d = decoding
    want = d["hyps"][1][1]
    lz = capi.Network.lazy(d["ncl"], d["ng"], d["models"], max_states=1 << 16, max_arcs=1 << 18, pushing=True, lookahead_sets=True)
    s0 = lz.lazy_size()
    dec = capi.Decoder(lz, d["models"], max_streams=3, main_beam=400.0)
    for u, h in enumerate(dec.decode_batch(d["feats"])):
        _same_hyp(h, want[u])
    s1 = lz.lazy_size()
    assert s1[0] > s0[0]
    lz.lazy_reset()
    assert lz.lazy_size() == s0 and lz.lazy_generation() == 1
    for u, h in enumerate(dec.decode_batch(d["feats"])):
        _same_hyp(h, want[u])
    assert lz.lazy_size() == s1
    lz.lazy_set_high_water(0.5 * (s0[0] + s1[0]) / float(1 << 16))        # (between the start state's closure and what a batch leaves)
    for u, h in enumerate(dec.decode_batch(d["feats"])):
        _same_hyp(h, want[u])
    assert lz.lazy_generation() == 2
    del dec, lz                                                           # jd_dec_destroy, jd_net_destroy


def test_batch_test_cli(decoding, tmp_path):
    """6. jd_batch_test -gramFsmFName ... -lookaheadSets, composed first and with -lazy: the transcripts of the hypotheses above."""
    from juicer_amd import build as jbuild, io as jio
    d = decoding
    jio.write_fsm(tmp_path / "cl.fsm", d["cl"])
    jio.write_fsm(tmp_path / "g.fsm", d["g"])
    jio.write_jdam(tmp_path / "m.jdam", _am(d["c"]))
    with open(tmp_path / "list.txt", "w") as f:
        for u, x in enumerate(d["feats"]):
            jio.write_jdf(tmp_path / ("u%d.jdf" % u), x)
            f.write("%s\n" % (tmp_path / ("u%d.jdf" % u)))
    base = [jbuild.BATCH_TEST, "-fsmFName", str(tmp_path / "cl.fsm"), "-gramFsmFName", str(tmp_path / "g.fsm"),
            "-modelsFName", str(tmp_path / "m.jdam"), "-inputFName", str(tmp_path / "list.txt"),
            "-mainBeam", "400", "-lmScaleFactor", str(d["c"]["lm"]), "-outputFormat", "ref", "-lookaheadSets"]
    want = [(h.label[::-1] - 1).tolist() for h in d["hyps"][0][1]]
    assert all(want)
    for extra in ([], ["-lazy"]):
        out = subprocess.run(base + extra, capture_output=True, text=True, timeout=240)
        assert out.returncode == 0, out.stderr
        lines = out.stdout.splitlines()
        assert len(lines) == 3
        assert [[int(w) for w in l.split()] for l in lines] == want
    # the option belongs to the composition
    out = subprocess.run([a for a in base if a not in ("-gramFsmFName", str(tmp_path / "g.fsm"))], capture_output=True, text=True, timeout=60)
    assert out.returncode != 0 and "-lookaheadSets" in out.stderr
