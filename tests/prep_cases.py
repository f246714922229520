"""The cases of tests/test_prep_cpu.py: networks and model sets as jd_net / jd_am hold them, and which development knobs and pruning
settings each case runs the preparation (juicer_amd/csrc/jd_prep.h) with.  The synthetic configurations come through the library's own
loaders (host code only); everything else is written out by hand here, with log probabilities chosen as plain binary fractions so that
no case depends on how a logarithm rounds."""
import hashlib

import numpy as np

LZ = np.float32(-3.402823466e+38)
KNOBS = ["renumber", "xsort", "sole", "xcut", "srec_split", "no_lr"]
INF = np.float32(np.inf)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def fbits(x):
    return int(np.float32(x).view(np.uint32))


# ------------------------------------------------------------------------------------------------ networks

def net_of(rows, init=0, fin=()):
    """rows[q] = [(to, w, in, out), ...] in file order"""
    n = len(rows)
    row_ptr = np.zeros(n + 1, np.int32)
    row_ptr[1:] = np.cumsum([len(r) for r in rows])
    arcs = [a for r in rows for a in r]
    fin_w = np.full(n, INF, np.float32)
    for q, w in fin:
        fin_w[q] = w
    col = lambda i, dt: np.asarray([a[i] for a in arcs], dt) if arcs else np.zeros(0, dt)
    return dict(n_states=n, init=init, row_ptr=row_ptr, to=col(0, np.int32), w=col(1, np.float32), ilab=col(2, np.int32), olab=col(3, np.int32), fin_w=fin_w)


def lexicon(order, n_words=5, n_hmm=6):
    """A lexicon loop: the root, and a chain of 2 .. 5 phones per word back to it.  order "chain": numbered chain after chain (the layout the
    decoder's numbering makes itself); "bfs": the same graph numbered breadth first."""
    lens = [2 + (w % 4) for w in range(n_words)]
    ident = {}                                                         # (word, position) -> state; position 0 is the root

    def number(key):
        if key not in ident:
            ident[key] = len(ident) + 1
        return ident[key]
    if order == "chain":
        for w in range(n_words):
            for k in range(1, lens[w]):
                number((w, k))
    else:
        for k in range(1, max(lens)):
            for w in range(n_words):
                if k < lens[w]:
                    number((w, k))
    rows = [[] for _ in range(len(ident) + 1)]
    for w in range(n_words):
        for k in range(lens[w]):
            src = 0 if k == 0 else ident[(w, k)]
            dst = 0 if k == lens[w] - 1 else ident[(w, k + 1)]
            rows[src].append((dst, -0.5 * (w + 1) if k == 0 else 0.0, 1 + (3 * w + k) % n_hmm, w + 1 if k == lens[w] - 1 else 0))
    return net_of(rows, 0, [(0, -0.25)])


def unreachable_net():
    """init = 2; states 0, 1 and 5 are not reached from it (the second pass of the numbering takes them, in the network's order)"""
    rows = [[(1, -1.0, 1, 0), (3, -2.0, 2, 1)],                        # 0: unreachable, leads into the reachable part
            [(0, -0.5, 3, 0)],                                         # 1: unreachable one-arc state
            [(4, -0.25, 1, 0), (3, -0.75, 2, 2), (6, -1.5, 0, 0)],     # 2: init
            [(2, 0.0, 4, 0)],
            [(3, -1.0, 5, 3), (4, -0.125, 2, 0)],                      # (a self-loop on 4)
            [(5, -3.0, 1, 0), (2, -1.0, 2, 0)],                        # 5: unreachable, with a self-loop
            [(2, -0.5, 6, 4)]]
    return net_of(rows, 2, [(3, -1.0), (5, -2.0)])


def selfloop_net():
    rows = [[(0, -1.0, 1, 0), (1, -0.5, 2, 1), (2, -0.25, 0, 0)],      # 0: a model self-loop
            [(1, -2.0, 3, 0)],                                         # 1: a one-arc state whose arc is a self-loop
            [(2, -0.125, 0, 5), (0, -1.0, 4, 0)],                      # 2: an EPSILON self-loop (the label-less part has a cycle)
            ]
    return net_of(rows, 0, [(2, 0.0)])


def threshold_net(n_arcs, n_next):
    """n_next arcs along a chain 0 -> 1 -> .. (each to the next state number), the other arcs from the chain's last state back to 0"""
    rows = [[(q + 1, -0.5, 1 + q % 4, 0)] for q in range(n_next)]
    rows.append([(0, -0.25 * (i + 1), 1 + i % 5, i + 1) for i in range(n_arcs - n_next)])
    return net_of(rows, 0, [(n_next, 0.0)])


def xcut_net(n_plain, n_tee, tee_label):
    """n_plain arcs that enter an ordinary model (all in rows short enough to be sorted) and n_tee arcs of the tee model"""
    rows = [[(1, -0.125 * i, 1 + i % 4, 0) for i in range(n_plain)] + [(1, -0.5, tee_label, 0) for _ in range(n_tee)],
            [(0, 0.0, 0, 1)]]
    return net_of(rows, 0, [(1, 0.0)])


def long_rows_net(n_hmm):
    """rows of 57 arcs (the longest the decoder puts in its own order) and of 58 (which keeps the file's), weights neither ascending nor descending"""
    rows = [[(1, -0.25 * ((7 * i) % 19), 1 + i % n_hmm, i + 1) for i in range(57)],
            [(0, -0.25 * ((5 * i) % 23), 1 + (i * 3) % n_hmm, 0) for i in range(58)]]
    rows[0][10] = (1, -1.0, 0, 9)                                      # an epsilon arc inside the sorted row
    rows[1][20] = (0, -1.0, 0, 0)                                      # ... and inside the one that keeps its order
    return net_of(rows, 0, [(1, 0.0)])


XCAND = (0, 1, 2, 3, 4, 6, 8, 12, 16, 24, 32, 64)


def xcand_net(n_hmm, tee_label):
    """one state per count of entry arcs on either side of every position k[] samples that a sorted row can reach (0 .. 33 arcs), each
    row with an epsilon arc and a tee arc mixed in; then a row whose entry arcs all have the same key, for the stable order"""
    counts = sorted({c for p in XCAND if p < 57 for c in (p, p + 1)})
    rows = []
    sink = len(counts) + 1
    for n in counts:
        r = [(sink, -0.25 * ((11 * i) % 13) - 0.125 * (i % 2), 1 + (i * 5) % n_hmm, 0) for i in range(n)]
        r.insert(n // 2, (sink, -0.5, 0, 0))
        r.insert((n + 1) // 3, (sink, -0.75, tee_label, 3))
        rows.append(r)
    rows.append([(sink, -1.0, 1, i + 1) for i in range(9)])            # equal w and equal model: equal keys, told apart by their labels
    rows.append([(0, 0.0, 0, 0)])
    return net_of(rows, 0, [(sink, 0.0)]), counts


def sole_net(tee_label):
    """destinations with in-degree 1 reached by a model arc (1), by a tee arc (2) and by an epsilon arc (3); in-degree 2 from ONE source state
    (4); in-degree 2 from two states, one of them by an epsilon arc (5); a self-loop as the second way in (6)"""
    rows = [[(1, -0.5, 1, 0), (2, -0.25, tee_label, 0), (3, -1.0, 0, 0), (4, -0.5, 2, 0), (4, -0.75, 3, 0), (5, -0.125, 4, 1), (6, -2.0, 1, 0)],
            [(0, 0.0, 2, 1)],
            [(0, 0.0, 0, 2)],
            [(5, -1.0, 0, 0)],
            [(0, 0.0, 0, 0)],
            [(0, -0.5, 0, 0)],
            [(6, -0.25, 2, 0), (0, 0.0, 0, 0)]]
    return net_of(rows, 0, [(0, 0.0)])


# ------------------------------------------------------------------------------------------------ model sets

def se_index(trP, n, max_n):
    """SEIndex of a transition matrix (createTrPandSEIndex, HTKModels.cpp:2376-2386)"""
    se = np.zeros((max_n, 2), np.int16)
    for j in range(1, n):
        mn = 1 if j == n - 1 else 0
        while mn < n - 1 and not trP[mn, j] > LZ:
            mn += 1
        mx = n - 1
        while mx >= 1 and not trP[mx, j] > LZ:
            mx -= 1
        se[j] = (mn, mx + 1)
    return se


def tm_lr(n, max_n, v=0, skip=False, tee=False, entry2=False):
    """log transition matrix of an n-state left-to-right model, in binary fractions: variant v moves them"""
    t = np.full((max_n, max_n), LZ, np.float32)
    t[0, 1] = -0.125 * v
    for j in range(1, n - 1):
        t[j, j] = -0.5 - 0.25 * ((j + v) % 3)
        t[j, j + 1] = -1.0 - 0.125 * ((2 * j + v) % 5)
    if skip and n >= 4:
        t[1, 3] = -2.5
    if tee:
        t[0, n - 1] = -1.5
    if entry2 and n >= 4:
        t[0, 2] = -2.0
    return t


def am_of(max_n, tms, hmms, tm_n=None):
    """tms: [(n, matrix)], hmms: [(n, tm)]; tee = log P(entry -> exit) of the HMM's matrix"""
    n_tm, n_hmm = len(tms), len(hmms)
    trP = np.stack([m for _, m in tms]).astype(np.float32)
    tmn = np.asarray([n for n, _ in tms] if tm_n is None else tm_n, np.int32)
    se = np.stack([se_index(m, max(int(n), 0), max_n) for (_, m), n in zip(tms, tmn)])
    hmm_n = np.asarray([n for n, _ in hmms], np.int32)
    hmm_tm = np.asarray([t for _, t in hmms], np.int32)
    tee = np.asarray([trP[t, 0, tms[t][0] - 1] if tms[t][0] >= 2 else LZ for _, t in hmms], np.float32)
    hmm_gmm = np.full((n_hmm, max_n), -1, np.int32)
    for h, (n, _) in enumerate(hmms):
        for j in range(1, n - 1):
            hmm_gmm[h, j] = (7 * h + 3 * j) % 50
    return dict(n_hmm=n_hmm, max_n=max_n, n_tm=n_tm, hmm_n=hmm_n, hmm_tm=hmm_tm, hmm_tee=tee, hmm_gmm=hmm_gmm, tm_n=tmn, trP=trP, se=se)


def am_plain(max_n=5, n_hmm=6, n_tm=3, **kw):
    """n_hmm left-to-right models of max_n states and, as HMM n_hmm + 1, a 3-state tee model"""
    tms = [(max_n, tm_lr(max_n, max_n, v, **kw)) for v in range(n_tm)] + [(3, tm_lr(3, max_n, 1, tee=True))]
    return am_of(max_n, tms, [(max_n, h % n_tm) for h in range(n_hmm)] + [(3, n_tm)])


def am_many_tm(max_n, n_tm):
    tms = [(max_n, tm_lr(max_n, max_n, v % 7)) for v in range(n_tm)]
    return am_of(max_n, tms, [(max_n, (h * 37) % n_tm) for h in range(6)] + [(max_n, n_tm - 1)])


def synth_inputs():
    """the synthetic configurations of the GPU tests, as the library's loaders hand them to jd_dec_create"""
    from juicer_amd import capi, synth
    nets, ams = {}, {}
    for name, cfg in (("toy", synth.config_toy()), ("small", synth.config_small()), ("small_tree", synth.config_small(hub="tree")), ("mixed", synth.config_mixed())):
        am, net = cfg[0], cfg[1]
        gn, gm = capi.Network.from_synth(net), capi.Models.from_htk(am)
        c = gn.csr()
        nets[name] = dict(n_states=gn.n_states, init=gn.init_state, row_ptr=c["row_ptr"], to=c["to"], w=c["w"], ilab=c["ilab"], olab=c["olab"], fin_w=c["fin_w"])
        hn, hg, ht, _ = gm.topology()
        trP, se, tee = gm.trans()
        ams[name] = dict(n_hmm=gm.n_hmms, max_n=gm.max_states, n_tm=gm.n_tm, hmm_n=hn, hmm_tm=ht, hmm_tee=tee, hmm_gmm=hg,
                         tm_n=np.asarray(am.tm_nstates, np.int32), trP=trP, se=se)
    return nets, ams


def build():
    """(nets, ams, cases): cases = [dict(name, net, am, knobs, main_beam, max_hyps)], knobs by name, -1 unset"""
    nets, ams = synth_inputs()
    cases = []

    def case(name, net, am, main_beam=150.0, max_hyps=200, **knobs):
        assert set(knobs) <= set(KNOBS)
        cases.append(dict(name=name, net=net, am=am, knobs=dict({k: -1 for k in KNOBS}, **knobs), main_beam=float(main_beam), max_hyps=int(max_hyps)))

    # ---- the synthetic networks of the GPU tests under the knobs those tests force, and each of the other knobs on its own
    for s in ("toy", "small", "small_tree", "mixed"):
        case(s, s, s)
        for r in (0, 1):
            for sp in (0, 1, 2):
                case("%s_renumber%d_split%d" % (s, r, sp), s, s, renumber=r, srec_split=sp)
        case(s + "_no_sole", s, s, sole=0)
        case(s + "_no_sole_renumber1", s, s, sole=0, renumber=1)
        case(s + "_no_xsort", s, s, xsort=0)
        case(s + "_xcut0", s, s, xcut=0)
        case(s + "_xcut1", s, s, xcut=1)
        case(s + "_no_xsort_xcut1", s, s, xsort=0, xcut=1)
        case(s + "_no_lr", s, s, no_lr=1)
    # ---- hand-written model sets
    ams["plain5"] = am_plain(5)
    ams["plain6"] = am_plain(6)                                        # max_n 6: the wide instance template (AI 8)
    ams["skip5"] = am_plain(5, skip=True)                              # a skip transition: not left-to-right
    ams["entry2_6"] = am_plain(6, entry2=True)                         # entry into the second emitting state: other tmax0, not left-to-right
    t2 = np.full((5, 5), LZ, np.float32)
    t2[0, 1] = -0.5
    ams["tm_n2"] = am_of(5, [(5, tm_lr(5, 5)), (2, t2)], [(5, 0)] * 6 + [(2, 1)])          # a transition matrix with fewer than 3 states
    ams["hmm_n_ne_tm_n"] = am_of(5, [(5, tm_lr(5, 5)), (4, tm_lr(4, 5, 1))], [(5, 0)] * 5 + [(4, 0), (4, 1)])   # an HMM shorter than its matrix
    for max_n, n_tm in ((5, 512), (5, 513), (6, 256), (6, 257)):       # TRP_LDS_MAX / LRW and one above, for both record widths
        ams["tm%d_%d" % (n_tm, max_n)] = am_many_tm(max_n, n_tm)
    tee = 7                                                            # in-label of am_plain's tee model
    # ---- numbering
    nets["lex_chain"], nets["lex_bfs"] = lexicon("chain"), lexicon("bfs")
    nets["unreachable"], nets["selfloops"] = unreachable_net(), selfloop_net()
    case("lex_chain", "lex_chain", "plain5")
    case("lex_chain_renumber1", "lex_chain", "plain5", renumber=1)
    case("lex_bfs", "lex_bfs", "plain5")
    case("lex_bfs_renumber0", "lex_bfs", "plain5", renumber=0)
    case("unreachable", "unreachable", "plain5")
    case("unreachable_renumber1", "unreachable", "plain5", renumber=1)
    case("selfloops", "selfloops", "plain5")
    case("selfloops_renumber1", "selfloops", "plain5", renumber=1)
    # ---- thresholds, met exactly and missed by one arc
    for n_arcs, n_next in ((8, 2), (9, 2), (12, 3), (13, 3), (11, 3)):
        k = "thr_%d_%d" % (n_arcs, n_next)
        nets[k] = threshold_net(n_arcs, n_next)
        case(k, k, "plain5")
    for n_plain, n_tee in ((19, 1), (19, 2), (38, 2), (37, 2)):
        k = "xcut_%d_%d" % (n_plain, n_tee)
        nets[k] = xcut_net(n_plain, n_tee, tee)
        case(k, k, "plain5")
    # ---- arc order
    nets["long_rows"] = long_rows_net(6)
    nets["xcand_rows"], _ = xcand_net(6, tee)
    for a in ("plain5", "entry2_6"):
        case("long_rows_" + a, "long_rows", a)
        case("xcand_rows_" + a, "xcand_rows", a)
    case("long_rows_no_xsort", "long_rows", "plain5", xsort=0)
    case("xcand_rows_no_xsort", "xcand_rows", "plain5", xsort=0)
    # ---- SOLE
    nets["sole"] = sole_net(tee)
    case("sole", "sole", "plain5")
    case("sole_off", "sole", "plain5", sole=0)
    case("sole_renumber1", "sole", "plain5", renumber=1)
    # ---- models
    for a in ("plain6", "skip5", "tm_n2", "hmm_n_ne_tm_n", "tm512_5", "tm513_5", "tm256_6", "tm257_6"):
        case("models_" + a, "lex_chain", a)
    case("models_plain5_no_lr", "lex_chain", "plain5", no_lr=1)
    case("models_tm512_5_no_lr", "lex_chain", "tm512_5", no_lr=1)
    # ---- the histogram's range
    case("hist_off", "sole", "plain5", main_beam=150.0, max_hyps=0)
    for mb in (0.0, -5.0, 1044.0, 1045.0, 1045.5, 1046.0):
        case("hist_beam_%g" % mb, "sole", "plain5", main_beam=mb, max_hyps=100)
    return nets, ams, cases


NET_FIELDS = ["row_ptr", "to", "w", "ilab", "olab", "fin_w"]
AM_FIELDS = ["hmm_n", "hmm_tm", "hmm_tee", "hmm_gmm", "tm_n", "trP", "se"]


def _words(a):
    a = np.ascontiguousarray(a)
    if a.dtype == np.float32:
        return a.view(np.uint32).ravel()
    return a.ravel()


def digest_inputs(obj, fields):
    h = hashlib.sha256()
    for k in ("n_states", "init", "n_hmm", "max_n", "n_tm"):
        if k in obj:
            h.update(np.int32(obj[k]).tobytes())
    for f in fields:
        a = np.ascontiguousarray(obj[f])
        h.update(a.astype(a.dtype.newbyteorder("<")).tobytes())
    return h.hexdigest()


def driver_input(nets, ams, cases):
    """the text the driver reads, and the order of the networks and model sets in it"""
    net_names, am_names = sorted(nets), sorted(ams)
    out = [str(len(net_names))]
    for k in net_names:
        n = nets[k]
        out.append("%d %d %d" % (n["n_states"], n["init"], len(n["to"])))
        out.append(" ".join(map(str, n["row_ptr"].tolist())))
        arcs = np.stack([n["to"].astype(np.int64), bits(n["w"]).astype(np.int64), n["ilab"].astype(np.int64), n["olab"].astype(np.int64)], axis=1)
        out.append(" ".join(map(str, arcs.ravel().tolist())))
        out.append(" ".join(map(str, bits(n["fin_w"]).tolist())))
    out.append(str(len(am_names)))
    for k in am_names:
        a = ams[k]
        out.append("%d %d %d" % (a["n_hmm"], a["max_n"], a["n_tm"]))
        for f in AM_FIELDS:
            out.append(" ".join(map(str, _words(a[f]).tolist())))
    out.append(str(len(cases)))
    for c in cases:
        out.append(" ".join(map(str, [net_names.index(c["net"]), am_names.index(c["am"])] + [c["knobs"][k] for k in KNOBS] +
                                     [fbits(c["main_beam"]), c["max_hyps"]])))
    return "\n".join(out) + "\n"
