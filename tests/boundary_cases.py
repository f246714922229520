"""Beam settings that put a token EXACTLY on a pruning threshold (tests/test_boundary_cpu.py, tests/test_gpu_boundary.py).

Fixture scores are random floats, so no comparison of the search is ever made at equality by chance, and a `>` written as `>=`
(or a threshold built in another operation order, one ulp off) would pass every other test.  Here the oracle's probe log
(jo_dec_set_boundary) records every comparison of one site at nominal beams; of the comparisons that failed (start beam: that
kept their token) the one with the smallest margin sets the site's window to fl32(best - lhs), checked so that best - window
rounds back to lhs.  The decode then meets that token exactly on the threshold, and every earlier outcome is unchanged.  A
setting is kept only if the site's equality counter is >= 1 and the oracle with that site flipped gives another hypothesis or
other statistics - so the setting tells the right comparison from the wrong one."""
import numpy as np

SITES = ("start", "emit", "end", "word", "eps", "tee_word", "tee_end")
WINDOW = {"start": "start_beam", "emit": "main_beam", "end": "end_beam", "word": "word_beam", "eps": "end_beam",
          "tee_word": "word_beam", "tee_end": "end_beam"}
NOMINAL = dict(start_beam=60.0, main_beam=90.0, end_beam=60.0, word_beam=45.0)
SEEDS = (7004, 7011, 7020, 7024, 7035, 7065)
LZ = -1e9


def fixture(seed):
    """a random graph (tests/random_topology.py: epsilon and tee arcs anywhere, labels on any arc) with tee models"""
    from juicer_amd import synth
    import random_topology as rt
    rng = np.random.default_rng(seed)
    if seed % 2:
        am = synth.make_models(seed, n_gmm=60, n_hmm=25, n_mix=2, n_tm=6, sep=0.7, with_tee=True)
    else:
        am = synth.make_models_mixed(seed, n_gmm=120, n_hmm=25, n_mix=2, with_tee=True, sep=0.7)
    net = rt.random_net(seed + 7, am, n_states=int(rng.integers(20, 70)), p_chain=0.5)
    feats = rt.random_walk_features(seed + 9, net, am, n_arcs=int(rng.integers(8, 16)))
    return am, net, feats


def same_result(a, b):
    return (a.n == b.n and np.array_equal(a.label, b.label) and np.array_equal(a.time, b.time)
            and np.array_equal(a.score.view(np.uint32), b.score.view(np.uint32))
            and all(a.stats[k] == b.stats[k] for k in a.stats if k != "ties"))


def _candidates(site, probe):
    """(margin, window) of the comparisons whose outcome holds at equality, smallest margin first"""
    frame, lhs, th, base = (probe[:, i] for i in range(4))
    live = (lhs > LZ) & (th > LZ)
    if site == "start":
        ok = live & (lhs >= th)
        margin = lhs.astype(np.float64) - th
    else:
        ok = live & (lhs <= th)
        margin = th.astype(np.float64) - lhs
    out = []
    for i in np.flatnonzero(ok)[np.argsort(margin[ok], kind="stable")]:
        if site == "emit":
            win = np.float32(-lhs[i])
            good = np.float32(-win) == lhs[i]
        else:
            win = np.float32(np.float32(base[i]) - np.float32(lhs[i]))
            good = np.float32(np.float32(base[i]) - win) == lhs[i]
        if good and win > 0 and np.float32(float("%.9g" % win)) == win:
            out.append((float(margin[i]), win))
    return out


def find_setting(onet, oam, feats, site, tries=6):
    """beams (float32) that put a token of this fixture exactly on the site's threshold, or None"""
    from oracle.oracle import SITES as ORACLE_SITES, OracleDecoder
    s = ORACLE_SITES.index(site)
    od = OracleDecoder(onet, oam, **NOMINAL)
    od.set_boundary(0, s)
    od.decode(feats)
    seen = set()
    for _, win in _candidates(site, od.probe()):
        if win in seen:
            continue
        seen.add(win)
        if len(seen) > tries:
            break
        beams = dict(NOMINAL, **{WINDOW[site]: float(win)})
        d = OracleDecoder(onet, oam, **beams)
        try:
            o = d.decode_certified(feats)
        except AssertionError:
            continue
        if d.site_hits()[site] < 1:
            continue
        d.set_boundary(1 << s, -1)
        f = d.decode(feats)
        if same_result(o, f):
            continue
        return beams
    return None


def settings():
    """[(seed, site, beams)] over the fixtures; deterministic"""
    from oracle.oracle import OracleAM, OracleNet
    out = []
    for seed in SEEDS:
        am, net, feats = fixture(seed)
        onet, oam = OracleNet(net), OracleAM(am)
        for site in SITES:
            b = find_setting(onet, oam, feats, site)
            if b is not None:
                out.append((seed, site, b))
    return out
