"""Random PAIRS of transducers of arbitrary shape for the composition tests - TEST INFRASTRUCTURE, plain numpy, no device.
jd_net_compose and jd_net_create_lazy take any C.L and any G; juicer_amd/synth.py only ever makes a lexicon prefix tree and a
back-off n-gram.  Here both sides are random graphs, with a knob for every shape the expansion step (jc_expand of
csrc/jd_compose.hip, lz_expand of csrc/jd_lazy.h) and the look-ahead decide on:

  hub_width     one C.L state with exactly that many arcs, labelled and label-less mixed, to states all over the graph: the
                64-arc chunks of the expansion step (63 / 64 / 65 / 128 / 129 / 150: one, exactly one, two, ... trips)
  transducer    G's output labels differ from its input labels (0 included): the composed arc must carry G's
  less_cycles   cycles (and a self loop) of label-less C.L arcs: "every label" look-ahead entries
  dead_ends     C.L states without arcs that are not final, behind label-less arcs: an empty interval without LA_MAYFIN;
                and one terminal FINAL state behind a label-less arc: an empty interval with it
  (always)      final C.L states with arcs and weights, so that LA_MAYFIN comes through non-terminal states; G states without
                arcs and with the back-off only; a back-off chain three deep, entered wherever a word ends; words 1, 2 that
                only C.L has and n_words + 1 .. n_words + 3 that only G has; arcs into both initial states
  wide_sets     a G row of 200 arcs or more and a C.L state whose label SET is no interval under the library's word numbering
                and has more than 64 labels (every other label of the hub, which the numbering walk meets first): the
                wave-cooperative list test (la_set_wave, csrc/jd_lazy.h), which walks the shorter side - here the list - and
                searches the other.  wide_sets=2: three of every four labels of the hub (about 105) against a G row of about
                100 arcs, 40 to 60 of them inside the list's range: the same test walking G's arcs and searching the list
  sparse        few labels, few arcs, and chains of label-less arcs that end in a label: label pushing moves those

Two profiles.  "arrays": anything goes, cycles of epsilon-INPUT arcs in C.L and back-off arcs to any G state included - for
the tests that compare composed arrays.  "decodable": C.L arcs with input 0 or the tee model lead to higher state numbers
only and G's epsilon to a lower one, so that (c, -g) grows along every epsilon arc of the composed graph and a search can
run on it.  In both, a G state has no two arcs with one input label (the library refuses that), hence at most one epsilon.

A pair is a dictionary: cl / g are csr()-style dictionaries (row_ptr, to, w, ilab, olab, fin_w; the weights are scores
<= 0 from a continuous range), cl_init / g_init the initial states, hub / list_state the special C.L states (or None)."""
import numpy as np

INF = np.float32(np.inf)


def _csr(n_states, arcs, fin_w):
    """arcs: (src, dst, ilab, olab, w) in the order they were added; the arcs of a state keep that order"""
    src = np.asarray([a[0] for a in arcs], np.int64)
    order = np.argsort(src, kind="stable")
    rp = np.zeros(n_states + 1, np.int64)
    np.add.at(rp, src + 1, 1)
    col = lambda k, dt: np.asarray([arcs[i][k] for i in order], dt)
    return dict(row_ptr=np.cumsum(rp).astype(np.int32), to=col(1, np.int32), ilab=col(2, np.int32), olab=col(3, np.int32),
                w=col(4, np.float32), fin_w=np.asarray(fin_w, np.float32))


def random_pair(seed, profile="arrays", n_cl=14, n_g=7, n_words=30, n_model=20, tee=0, hub_width=0, transducer=False,
                less_cycles=0, dead_ends=0, wide_sets=0, sparse=False, chains=0):
    """tee: the (1-based) input label of the tee model, 0 if there is none"""
    assert profile in ("arrays", "decodable")
    rng = np.random.default_rng(seed)
    dec = profile == "decodable"
    p_label, p_eps, per_state = (0.12, 0.1, 1.7) if sparse else (0.35, 0.15, 2.6)
    if sparse:
        n_words, chains = min(n_words, 8), max(chains, 6)
    if wide_sets:
        n_words, hub_width = max(n_words, 230), max(hub_width, 190)
    weight = lambda: -float(rng.uniform(0.05, 4.0))
    arcs = []

    # ---- C.L
    def add(s, d, olab=None, eps_in=None):
        if eps_in is None: eps_in = bool(rng.random() < p_eps)
        if olab is None:                                                # (label-less arcs lead upwards: their cycles are a knob, not the rule)
            olab = int(rng.integers(1, n_words + 1)) if (rng.random() < p_label or s >= d) else 0
        il = 0
        if not eps_in or (dec and s >= d):
            il = int(rng.integers(1, n_model + 1))
            if il == tee and dec and s >= d: il = 1 + tee % n_model     # (a tee model passes tokens on within the frame, like epsilon)
        arcs.append((s, d, il, olab, weight()))

    order = [int(x) for x in rng.permutation(n_cl)]
    if dec:                                                             # (a low initial state: epsilons have somewhere to go)
        first = min(order[:3])
        order.sort(key=lambda s: s != first)
    init = order[0]
    hub = order[1] if hub_width else None
    n_states = n_cl
    list_state = None
    if wide_sets:
        list_state = n_states; n_states += 1
        add(init, hub, olab=0, eps_in=False)                            # the numbering walk goes through the hub first
    sources = lambda k: [s for s in order[:k] if s != hub]
    for k in range(1, n_cl):                                            # a spine: every state can be reached
        cand = sources(k)
        s = order[k - 1] if (rng.random() < 0.5 and order[k - 1] != hub) else cand[int(rng.integers(0, len(cand)))]
        add(s, order[k])
    for _ in range(max(0, int(n_cl * per_state) - (n_cl - 1))):
        s = int(rng.integers(0, n_cl))
        if s != hub: add(s, int(rng.integers(0, n_cl)))                 # (parallel arcs, self loops, arcs into the initial state)
    add(order[-1], init)
    for _ in range(less_cycles):
        a, b = (int(x) for x in rng.choice([s for s in range(n_cl) if s != hub], size=2, replace=False))
        add(a, b, olab=0); add(b, a, olab=0)
        add(b, b, olab=0, eps_in=False)
    if not dec:                                                         # a cycle of epsilon-input arcs, one of them with a label
        a, b = (int(x) for x in rng.choice([s for s in range(n_cl) if s != hub], size=2, replace=False))
        add(a, b, olab=0, eps_in=True); add(b, a, eps_in=True)
    dead = []
    for _ in range(dead_ends):
        dead.append(n_states); n_states += 1
        s = int(rng.choice([x for x in range(n_cl) if x != hub]))
        add(s, dead[-1], olab=0)
    term = None
    if dead_ends:                                                       # a terminal final state behind a label-less arc
        term = n_states; n_states += 1
        add(int(rng.choice([x for x in range(n_cl) if x != hub])), term, olab=0)
    for _ in range(chains):                                             # label-less chains that end in a label: what label pushing moves
        s = int(rng.choice([x for x in range(n_cl) if x != hub]))
        for _ in range(int(rng.integers(2, 4))):
            add(s, n_states, olab=0, eps_in=False)
            s = n_states; n_states += 1
        add(s, int(rng.integers(0, n_cl)), olab=int(rng.integers(1, n_words + 1)), eps_in=False)
    if hub_width:
        targets = list(range(n_cl)) + dead + ([term] if term is not None else [])
        n_lab = 140 if wide_sets else int(round(0.6 * hub_width))
        labelled = np.zeros(hub_width, bool)
        labelled[rng.choice(hub_width, size=n_lab, replace=False)] = True
        hub_labels = [int(x) for x in (rng.permutation(n_words)[:n_lab] + 1)] if wide_sets else None
        k = 0
        for j in range(hub_width):
            d = int(targets[int(rng.integers(0, len(targets)))])
            if labelled[j]:
                add(hub, d, olab=hub_labels[k] if wide_sets else int(rng.integers(1, n_words + 1))); k += 1
            else:
                add(hub, d, olab=0)
        if wide_sets:                                                   # every other label of the hub (2: three of four), below a state met after it
            for x in (hub_labels[::2] if wide_sets == 1 else [x for j, x in enumerate(hub_labels) if j % 4]):
                add(list_state, int(rng.integers(0, n_cl)), olab=x, eps_in=False)
            add(init, list_state, olab=0, eps_in=False)
    cl_fin = np.full(n_states, INF, np.float32)
    for s in range(n_cl):
        if rng.random() < 0.3: cl_fin[s] = -rng.uniform(0.0, 3.0)
    if not np.isfinite(cl_fin[:n_cl]).any(): cl_fin[order[-1]] = -rng.uniform(0.0, 3.0)
    if term is not None: cl_fin[term] = -rng.uniform(0.0, 3.0)
    cl = _csr(n_states, arcs, cl_fin)

    # ---- G: words 3 .. n_words + 3 (C.L has 1 .. n_words)
    vocab = np.arange(3, n_words + 4)
    empty, bo_only = (1, 2) if n_g >= 6 else (None, None)               # a state without arcs, one with the back-off only
    g_init = n_g - 1 if dec else int(rng.choice([s for s in range(n_g) if s not in (empty, bo_only)]))
    garcs = []
    for s in range(n_g):
        row = []
        if s == empty:
            continue
        if s != bo_only:
            lo_k, hi_k = (2, 5) if sparse else (max(2, n_words // 4), max(3, (4 * n_words) // 5))
            k = int(rng.integers(lo_k, hi_k + 1))
            if wide_sets and s == g_init: k = max(k, 205) if wide_sets == 1 else 100
            for x in rng.choice(vocab, size=min(k, vocab.size), replace=False):
                o = int(x)
                if transducer:
                    r = rng.random()
                    o = int(rng.integers(1, n_words + 4)) if r < 0.7 else (0 if r < 0.8 else o)
                row.append((s, int(rng.integers(0, n_g)), int(x), o, weight()))
        # the back-off: states 3 -> 2 -> 1 -> 0 ... a chain, elsewhere at random; "decodable": to a lower state number only
        if s > 0 and (s <= 4 or s == bo_only or rng.random() < 0.6):
            t = s - 1 if (s <= 4 or dec and rng.random() < 0.5) else int(rng.integers(0, s if dec else n_g))
            o = int(rng.integers(1, n_words + 4)) if (transducer and rng.random() < 0.3) else 0
            row.append((s, t, 0, o, weight()))
        for i in rng.permutation(len(row)): garcs.append(row[int(i)])   # (any order: the library sorts a G state's arcs)
    g_fin = np.full(n_g, INF, np.float32)
    for s in range(n_g):
        if rng.random() < 0.5: g_fin[s] = -rng.uniform(0.0, 3.0)
    if not np.isfinite(g_fin).any(): g_fin[0] = -rng.uniform(0.0, 3.0)
    g = _csr(n_g, garcs, g_fin)
    return dict(cl=cl, cl_init=init, g=g, g_init=g_init, hub=hub, list_state=list_state, profile=profile, n_words=n_words,
                dead=dead, term=term, tee=tee, seed=seed)


# The pairs of tests/test_random_pairs_cpu.py and tests/test_gpu_random_pairs.py: (id, random_pair's arguments).  The seeds are
# the ones for which the REFERENCES alone (tests/compose_ref.py, tests/compose_sets_ref.py, the CPU oracle) meet what
# test_random_pairs_cpu.py asks of a fixture: shape facts, accepted sequences, utterances with a hypothesis and without ties.
N_MODEL = 20                                                            # HMMs of the decodable pairs' acoustic model; the last is the tee model
PAIRS = [
    ("hub63", dict(seed=101, hub_width=63, less_cycles=1, dead_ends=2)),
    ("hub64", dict(seed=102, hub_width=64, transducer=True, dead_ends=1)),
    ("hub65", dict(seed=103, hub_width=65, less_cycles=1)),
    ("hub128", dict(seed=114, hub_width=128, transducer=True, less_cycles=2, dead_ends=2)),
    ("hub129", dict(seed=105, hub_width=129, dead_ends=1)),
    ("hub150", dict(seed=106, hub_width=150, transducer=True, less_cycles=1, dead_ends=2)),
    ("wide_sets", dict(seed=107, wide_sets=1, dead_ends=1)),
    ("wide_sets_g", dict(seed=109, wide_sets=2, dead_ends=1)),
    ("sparse", dict(seed=158, sparse=True, hub_width=70, dead_ends=1)),
    ("dec_hub65", dict(seed=201, profile="decodable", tee=N_MODEL, hub_width=65, less_cycles=1, dead_ends=2)),
    ("dec_hub150", dict(seed=242, profile="decodable", tee=N_MODEL, hub_width=150, transducer=True, dead_ends=1)),
    ("dec_sparse", dict(seed=273, profile="decodable", tee=N_MODEL, sparse=True, hub_width=129, dead_ends=1)),
    ("dec_plain", dict(seed=204, profile="decodable", tee=N_MODEL, transducer=True, less_cycles=2, dead_ends=2)),
]
DECODABLE = [p for p in PAIRS if p[1].get("profile") == "decodable"]
# the utterances (walk numbers, see utterances()) of the decodable pairs: the first six on which the CPU oracle finds words,
# the same ones on the textbook and on the filtered composition, and has no order-dependent tie under any option mask.
# After changing a seed: find_utterances(name) gives the new tuple (tests/test_random_pairs_cpu.py holds UTTS to it).
UTTS = {"dec_hub65": (0, 1, 2, 3, 4, 5), "dec_hub150": (0, 1, 2, 3, 4, 5), "dec_sparse": (0, 1, 2, 3, 4, 5), "dec_plain": (0, 1, 2, 3, 5, 6)}


def models(seed):
    """the acoustic model of a decodable pair (its last HMM is the tee model, label N_MODEL)"""
    from juicer_amd import synth
    am = synth.make_models(seed, n_gmm=60, n_hmm=N_MODEL, n_mix=2, n_tm=6, sep=0.7, with_tee=True)
    assert am.sp_hmm + 1 == N_MODEL
    return am


def networks(pair):
    """(C.L, G) as capi.Network objects; the weights are taken as they are"""
    from juicer_amd import capi
    out = []
    for k, i in (("cl", "cl_init"), ("g", "g_init")):
        a = pair[k]
        fs = np.nonzero(np.isfinite(a["fin_w"]))[0].astype(np.int32)
        out.append(capi.Network.from_csr(len(a["row_ptr"]) - 1, pair[i], a["row_ptr"], a["to"], a["w"], a["ilab"], a["olab"], fs, a["fin_w"][fs]))
    return tuple(out)


def row_widths(a):
    return np.diff(np.asarray(a["row_ptr"], np.int64))


def check_rules(pair):
    """what every pair keeps; and, for a decodable one, that no epsilon arc of the composed graph can close a cycle"""
    g, cl = pair["g"], pair["cl"]
    for s in range(len(g["row_ptr"]) - 1):
        il = g["ilab"][g["row_ptr"][s]:g["row_ptr"][s + 1]]
        assert len(set(il.tolist())) == len(il), "G state %d has two arcs with one input label" % s
    if pair["profile"] == "decodable":
        tee = pair.get("tee", 0)
        src = np.repeat(np.arange(len(cl["row_ptr"]) - 1), row_widths(cl))
        quick = (cl["ilab"] == 0) | ((cl["ilab"] == tee) & (tee > 0))
        assert np.all(cl["to"][quick] > src[quick])
        gsrc = np.repeat(np.arange(len(g["row_ptr"]) - 1), row_widths(g))
        assert np.all(g["to"][g["ilab"] == 0] < gsrc[g["ilab"] == 0])


def sample_sequences(seed, graph, n, max_words=5):
    """n word sequences from random walks through a composed graph (compose_naive's): the output labels along the walk, which
    ends at a final state where it can - such a sequence is accepted - or after a while, wherever it is; every fourth
    sequence gets one word replaced (mostly not accepted any more)"""
    rng = np.random.default_rng(seed)
    rp, to, ol = graph["row_ptr"], graph["to"], graph["olab"]
    fin = np.isfinite(graph["fin_w"])
    out = []
    for i in range(n):
        want = int(rng.integers(0, max_words + 1))
        for _ in range(4):                                              # (a walk that got stuck away from a final state: try again)
            s, ws = int(graph["init"]), []
            for _ in range(60):
                if fin[s] and len(ws) >= want: break
                if rp[s] == rp[s + 1] or len(ws) >= max_words + 2: break
                a = int(rng.integers(rp[s], rp[s + 1]))
                if ol[a]: ws.append(int(ol[a]))
                s = int(to[a])
            if fin[s]: break
        if i % 4 == 3 and ws:
            ws[int(rng.integers(0, len(ws)))] = int(rng.integers(1, int(ol.max()) + 1))
        out.append(ws)
    return out


def walk_features(seed, graph, am, n_arcs=8, noise=1.0):
    """Frames along a random walk through the model arcs of a composed graph (as random_topology.random_walk_features does for a
    network): the walk goes on until it has passed n_arcs models and stands at a final state, or for three times as long.
    Eight walks are tried for one that has passed a word and ends at a final state."""
    rng = np.random.default_rng(seed)
    rp, to, il, ol = graph["row_ptr"], graph["to"], graph["ilab"], graph["olab"]
    fin = np.isfinite(graph["fin_w"])
    for _ in range(8):                                                  # (a walk that ends away from a final state: try again)
        s, gm, passed, words = int(graph["init"]), [], 0, 0
        for _ in range(n_arcs * 6):
            if (passed >= n_arcs and words and fin[s]) or passed >= 3 * n_arcs or rp[s] == rp[s + 1]: break
            a = int(rng.integers(rp[s], rp[s + 1]))
            hm = int(il[a]) - 1
            if hm >= 0 and hm != am.sp_hmm:
                passed += 1
                for j in range(1, int(am.hmm_nstates[hm]) - 1):
                    for _ in range(int(rng.integers(1, 4))): gm.append(int(am.hmm_gmm[hm, j]))
            words += int(ol[a] != 0)
            s = int(to[a])
        if fin[s] and gm and words: break
    if not gm: gm = [0] * 10
    gm = np.asarray(gm, np.int64)
    mu, sd = am.mean[gm, 0], np.sqrt(am.var[gm, 0])
    return (mu + noise * sd * rng.normal(size=mu.shape)).astype(np.float32)


def reference(pair, mask):
    """what jd_net_compose / jd_net_create_lazy have to make of the pair under `mask` (JD_PUSH_WEIGHTS 1, JD_PUSH_LABELS 2,
    JD_LOOKAHEAD_SETS 4): compose_filtered for intervals, compose_sets with the sets bit, push_labels applied first"""
    from compose_ref import compose_filtered, push_labels
    from compose_sets_ref import compose_sets
    cl = pair["cl"]
    if mask & 2:
        cl = dict(cl, olab=push_labels(cl, pair["cl_init"])[0])
    fn = compose_sets if mask & 4 else compose_filtered
    return fn(cl, pair["cl_init"], pair["g"], pair["g_init"], pushing=bool(mask & 1))


MASKS = (0, 1, 2, 3, 4, 5)
BEAMS = dict(main_beam=400.0)                                           # the GPU tests' pruning on the decodable pairs


def utterances(name, naive, am):
    """the utterances of a decodable pair: walks through its textbook composition (UTTS: the ones the references agree on)"""
    seed = dict(PAIRS)[name]["seed"]
    return [walk_features(1000 * seed + u, naive, am, n_arcs=3 + u % 5) for u in UTTS[name]]


def find_utterances(name, n=6, tries=30):
    """the selection behind UTTS[name]: of the walks 0 .. tries - 1, the first n that the CPU oracle, nothing pruned, decodes to
    the same words (at least one) at the same times with the same acoustic and language-model totals on the textbook and on the
    filtered composition, and - under BEAMS - to words and without an order-dependent tie on the reference arrays of every mask"""
    from compose_ref import compose_naive
    from helpers import rel_close
    from oracle.oracle import OracleAM, OracleDecoder
    kw = dict(PAIRS)[name]
    p, am = random_pair(**kw), models(kw["seed"])
    oam = OracleAM(am)
    naive = compose_naive(p["cl"], p["cl_init"], p["g"], p["g_init"])
    refs = [reference(p, m) for m in MASKS]
    wide = [OracleDecoder(oracle_net(gr), oam, main_beam=0.0) for gr in (naive, refs[0])]
    beamed = [OracleDecoder(oracle_net(gr), oam, **BEAMS) for gr in refs]
    keep = []
    for u in range(tries):
        x = walk_features(1000 * kw["seed"] + u, naive, am, n_arcs=3 + u % 5)
        a, b = wide[0].decode(x), wide[1].decode(x)
        if not (a.n > 0 and a.n == b.n and np.array_equal(a.label, b.label) and np.array_equal(a.time, b.time)
                and rel_close(a.tot_ac, b.tot_ac) and rel_close(a.tot_lm, b.tot_lm)):
            continue
        try:
            if all(od.decode_certified(x).n > 0 for od in beamed): keep.append(u)
        except AssertionError:                                          # (decode_certified: an order-dependent tie)
            pass
        if len(keep) == n: break
    return tuple(keep)


def oracle_net(graph):
    from oracle.oracle import OracleNet
    fs = np.nonzero(np.isfinite(graph["fin_w"]))[0].astype(np.int32)
    return OracleNet.from_csr(graph["n_states"], graph["init"], graph["row_ptr"], graph["to"], graph["w"], graph["ilab"], graph["olab"],
                              fs, graph["fin_w"][fs])
