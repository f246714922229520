"""The pruning comparisons at equality, on the oracle (tests/boundary_cases.py makes the settings).  For every setting: the
site's equality counter is >= 1 in the decode that is actually run, and the oracle with that one comparison flipped (`>` as `>=`,
the start beam's `<` as `<=`) gives another hypothesis or other statistics.  So an implementation held to the oracle at these
settings (tests/test_gpu_boundary.py) cannot have the comparison the wrong way round, nor a threshold one ulp off."""
import collections

import numpy as np
import pytest

from boundary_cases import SEEDS, SITES, fixture, same_result, settings


@pytest.fixture(scope="module")
def found(built):
    return settings()


def test_every_site_is_reached_on_two_fixtures(found):
    per_site = collections.defaultdict(set)
    for seed, site, _ in found:
        per_site[site].add(seed)
    print("boundary settings per site: %s" % {s: len(per_site[s]) for s in SITES})
    for s in SITES:
        assert len(per_site[s]) >= 2, (s, sorted(per_site[s]))


def test_settings_hit_and_discriminate(found):
    from oracle.oracle import SITES as ORACLE_SITES, OracleAM, OracleDecoder, OracleNet
    assert ORACLE_SITES == SITES
    nets = {}
    for seed, site, beams in found:
        if seed not in nets:
            am, net, feats = fixture(seed)
            nets[seed] = (OracleNet(net), OracleAM(am), feats)
        onet, oam, feats = nets[seed]
        for v in beams.values():                                       # float32 windows that survive a %.9g round trip
            assert np.float32(v) == v and np.float32(float("%.9g" % v)) == v
        d = OracleDecoder(onet, oam, **beams)
        o = d.decode_certified(feats)
        hits = d.site_hits()
        assert hits[site] >= 1, (seed, site, beams, hits)
        d.set_boundary(1 << SITES.index(site), -1)
        f = d.decode(feats)
        assert not same_result(o, f), (seed, site, beams)
        d.set_boundary(0, -1)                                          # back to the reference's comparisons: the same result again
        assert same_result(o, d.decode(feats))


def test_test_aids_are_off_by_default(built):
    """counters and probes do not change a decode; a nominal decode of these fixtures meets no threshold exactly"""
    from boundary_cases import NOMINAL
    from oracle.oracle import OracleAM, OracleDecoder, OracleNet
    for seed in SEEDS:
        am, net, feats = fixture(seed)
        d = OracleDecoder(OracleNet(net), OracleAM(am), **NOMINAL)
        a = d.decode(feats)
        assert sum(d.site_hits().values()) == 0
        d.set_boundary(0, SITES.index("end"))
        b = d.decode(feats)
        assert same_result(a, b) and d.probe().shape[0] > 0
