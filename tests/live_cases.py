"""The fixtures the tests of the live views share (tests/test_gpu_final.py, tests/test_gpu_trace_models.py): synth.config_small
(k_search<3>), synth.config_mixed (NE = 6) and random topologies (epsilon and tee arcs, final weights anywhere) with three utterances
each, their beams, and the unequal steps three streams are pushed in.  Built once per name, never changed."""
import numpy as np

import random_topology as rt

MFIELDS = ("model", "label", "time", "score", "ac", "lm")
# (the random cases: random_3 and random_5 are the issue's, random_8 is tests/test_gpu_model_partial.py's second one)
CASES = ["small", "mixed", "random_3", "random_5", "random_8"]
# phase X's work counters differ between two identical decodes (tests/test_gpu_best.py, RUN_DEPENDENT)
RUN_DEPENDENT = ("tot_arcs_visited", "tot_paths", "tot_items_expanded", "tot_arcs_walked", "tot_closure_items")
_cache = {}


def _case(name):
    """(am, net, three utterances, beams, push steps of the three streams) - built once per name, never changed"""
    if name in _cache:
        return _cache[name]
    from juicer_amd import synth
    if name == "small":
        am, net, feats, _ = synth.config_small(n_utts=3)
        kw, steps = dict(main_beam=150.0, max_hyps=200), (13, 29, 50)
    elif name == "mixed":
        am, net, feats, _ = synth.config_mixed(n_utts=3)
        kw, steps = dict(main_beam=200.0), (13, 29, 50)
    else:
        seed = int(name.split("_")[1])
        am = synth.make_models(seed, n_gmm=40, n_hmm=12, n_mix=3, D=13, n_tm=4, with_tee=True)
        net = rt.random_net(seed, am, n_states=60, p_eps=0.2, p_label=0.35)
        feats = [rt.random_walk_features(seed * 10 + k, net, am) for k in range(3)]
        kw, steps = dict(main_beam=150.0), (3, 5, 9)
    _cache[name] = (am, net, feats, kw, steps)
    return _cache[name]


def _handles(name):
    from juicer_amd import capi
    am, net, feats, kw, steps = _case(name)
    key = name + "/gpu"
    if key not in _cache:
        _cache[key] = (capi.Network.from_synth(net), capi.Models.from_htk(am))
    return _cache[key] + (feats, kw, steps)


def _decoder(name, models, **extra):
    from juicer_amd import capi
    gnet, gam, feats, kw, steps = _handles(name)
    dec = capi.Decoder(gnet, gam, **dict(kw, **extra))
    if models:
        dec.set_output_level(capi.OUTPUT_WORDS | capi.OUTPUT_MODELS)
    return dec


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32).tolist() if a.dtype == np.float32 else a.tolist()


def _fbits(x):
    return _bits(np.asarray([x], np.float32))[0]


