"""The HIP path at the pruning comparisons' equality cases (settings: tests/boundary_cases.py; tests/test_boundary_cpu.py shows
that each one hits its site and that the oracle with that comparison flipped gives another result).  Every setting is decoded
through clusters of k_search and through the slot kernel, one fixture of each site also with JD_NO_SOLE, and held to the
certified oracle bit for bit: words, times, scores and the reference's statistics."""
import pytest

from helpers import STAT_KEYS, assert_hyp_matches

pytestmark = pytest.mark.gpu

FLAVOURS = {"k_search": {}, "slot": dict(JD_CW="1", JD_SLOT_BATCH="1"), "no_sole": dict(JD_NO_SOLE="1")}


@pytest.fixture(scope="module")
def found(built):
    from boundary_cases import settings
    return settings()


@pytest.mark.parametrize("flavour", list(FLAVOURS))
def test_hip_path_at_the_boundaries(found, flavour, monkeypatch):
    from boundary_cases import fixture
    from juicer_amd import capi
    from oracle.oracle import OracleAM, OracleDecoder, OracleNet
    monkeypatch.setenv("JD_DEV", "1")
    for k in ("JD_CW", "JD_SLOT_BATCH", "JD_NO_SOLE"):
        monkeypatch.delenv(k, raising=False)
    for k, v in FLAVOURS[flavour].items():
        monkeypatch.setenv(k, v)
    done, sites = 0, set()
    cache = {}
    for seed, site, beams in found:
        if flavour == "no_sole" and site in sites:
            continue
        if seed not in cache:
            am, net, feats = fixture(seed)
            cache[seed] = (am, net, feats, capi.Network.from_synth(net), capi.Models.from_htk(am))
        am, net, feats, gnet, gam = cache[seed]
        o = OracleDecoder(OracleNet(net), OracleAM(am), **beams).decode_certified(feats)
        gd = capi.Decoder(gnet, gam, max_streams=1, **beams)
        g = gd.decode_batch([feats])[0]
        gd.close()
        what = "%s seed %d site %s %s" % (flavour, seed, site, beams)
        assert_hyp_matches(g, o, what, check_stats=False)
        for k in STAT_KEYS:
            assert g.stats[k] == o.stats[k], "%s: stat %s %d vs oracle %d" % (what, k, g.stats[k], o.stats[k])
        done += 1
        sites.add(site)
    assert done >= 7 and len(sites) == 7
