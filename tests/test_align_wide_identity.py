"""swa_align_wide_for (align.hip): the band, the saturation and the offsets a lane of the wide alignment form, as a pure
function of the scoring and d — against the arithmetic restated here, for every reduced legal command-line scoring and
every d, and at the boundaries of the default scoring and of (1, 0, 1).  No GPU."""
import pytest

from swarm_amd import capi, reduced_penalties
from swarm_amd.capi import SWA_E_ARG, SwaError

SCORINGS = sorted({reduced_penalties(m, p, g, e) for m in range(1, 8) for p in range(1, 8) for g in range(8)
                   for e in range(8) if g + e >= 1})


def _expected(mm, go, ge, d):
    W = d * max(mm, go + ge) // ge + 1
    sat = 65535 if d > min(255 // mm, 255 // (go + ge)) else 255
    K = 0
    if 2 * W + 3 > 64:
        K = next((k for k in (2, 4, 8) if 2 * W + 3 <= 64 * k), 0)
    return W, sat, K


def test_every_scoring_and_d():
    assert len(SCORINGS) == 1486
    seen = set()
    for mm, go, ge in SCORINGS:
        last = 0
        grown = False
        for d in range(2, 256):
            got = capi.align_wide_for(mm, go, ge, d)
            assert got == _expected(mm, go, ge, d), (mm, go, ge, d)
            W, _, K = got
            assert (K == 0) == (W <= 30 or W > 254)
            if K != 0:                                       # the smallest K that holds band and guards
                assert 2 * W + 3 <= 64 * K and (K == 2 or 2 * W + 3 > 32 * K)
            # K does not decrease with d until the band passes 254, and stays 0 from there
            if W > 254:
                grown = True
                assert K == 0
            else:
                assert not grown and K >= last
                last = K
            seen.add(K)
    assert seen == {0, 2, 4, 8}


@pytest.mark.parametrize("d,K,W", [(10, 0, 29), (11, 2, 32), (21, 2, None), (22, 4, 63), (44, 4, None), (45, 8, 129),
                                   (89, 8, None), (90, 0, 257)])
def test_default_scoring_boundaries(d, K, W):
    got = capi.align_wide_for(18, 24, 13, d)
    assert got[2] == K and got[1] == 65535
    if W is not None:
        assert got[0] == W


def test_unit_scoring_boundaries():
    """(1, 0, 1): W = d + 1, 8-bit arithmetic at every d.  K = 2 at d = 31, 4 from d = 62, 8 from d = 126, 0 from d = 254.
    (W = 31 at d = 30 already needs 65 lanes, one more than k_align<64> has, so by 2 W + 3 <= 64 K the first d with
    K = 2 is 30.)"""
    first = {}
    for d in range(1, 256):
        W, sat, K = capi.align_wide_for(1, 0, 1, d)
        assert (W, sat) == (d + 1, 255)
        first.setdefault(K, d)
        if d >= 254:
            assert K == 0
    assert [capi.align_wide_for(1, 0, 1, d)[2] for d in (29, 31, 61, 62, 125, 126, 253, 254)] == [0, 2, 2, 4, 4, 8, 8, 0]
    assert first[2] == 30 and first[4] == 62 and first[8] == 126


@pytest.mark.parametrize("args", [(0, 1, 1, 2), (1, 0, 0, 2), (65536, 0, 1, 2), (1, 65536, 1, 2), (1, 0, 65536, 2),
                                  (18, 24, 13, 0), (18, 24, 13, 256)])
def test_refuses_what_search_begin_refuses(args):
    with pytest.raises(SwaError) as e:
        capi.align_wide_for(*args)
    assert e.value.code == SWA_E_ARG
