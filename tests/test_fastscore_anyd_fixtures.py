"""The decode fixtures of tests/test_gpu_fastscore_anyd.py, checked where no GPU is needed: the CPU oracle alone certifies every utterance
under every beam set (no result rests on the visiting order of equal scores), so the GPU tests compare all of them and drop none; and the
graphs have the few thousand arcs they are meant to have."""
import pytest

from helpers import oracle_certified_many
from test_gpu_fastscore import BEAMS
from test_gpu_fastscore_anyd import _cfg


@pytest.fixture(scope="module")
def built_oracle():
    from oracle import oracle as orc
    orc.build()
    return True


@pytest.mark.parametrize("D", [13, 80])
def test_oracle_certifies_every_utterance(built_oracle, D):
    am, net, feats = _cfg(D)
    assert am.D == D and feats[0].shape[1] == D
    assert 2000 <= net.n_arcs <= 20000, net.n_arcs
    assert feats[0].shape[0] > 1 + 7 + 64                  # (the streaming test's chunks)
    for kw in BEAMS:
        want = oracle_certified_many(net, am, feats, **kw)         # (decode_certified raises on a fixture that is order-sensitive)
        assert len(want) == len(feats) and all(o is not None and o.n > 0 for o in want), kw
