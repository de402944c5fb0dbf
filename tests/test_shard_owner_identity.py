"""The shard owner of a heavy amplicon in closed form (swa_d1_shard_owner_for) against the slices swa_d1_fastidious_shard
cuts: shard s of S takes the heavy amplicons whose ordinal h among the H heavy ones lies in [H s // S, H (s + 1) // S).  No
device: the kernels that evaluate the same form on the role bytes are tested in tests/test_multi_resident_gpu.py."""
import numpy as np
import pytest

from swarm_amd import SwaError, capi

SHARDS = (1, 2, 3, 7, 8, 63, 64)


def owners_by_ranges(heavy: int, nshards: int) -> np.ndarray:
    """owner of every ordinal, from the ranges themselves; every h must fall into exactly one"""
    owner = np.full(heavy, -1, dtype=np.int64)
    for s in range(nshards):
        lo, hi = heavy * s // nshards, heavy * (s + 1) // nshards
        assert (owner[lo:hi] == -1).all()
        owner[lo:hi] = s
    assert (owner >= 0).all()
    return owner


def shard_roles(is_light: np.ndarray, shard: int, nshards: int) -> np.ndarray:
    """the host loop of swa_d1_fastidious_shard restated: 0 light, 1 heavy and in this shard's slice, 2 neither"""
    heavy = is_light == 0
    seen = np.cumsum(heavy) - heavy                                # heavy amplicons in front of each one
    total = int(heavy.sum())
    lo, hi = total * shard // nshards, total * (shard + 1) // nshards
    return np.where(~heavy, 0, np.where((seen >= lo) & (seen < hi), 1, 2)).astype(np.uint8)


def owner_bytes(is_light: np.ndarray, nshards: int) -> np.ndarray:
    """255 for light, else shard_owner_for of the ordinal: what swa_d1_shard_owners_device leaves in HBM"""
    heavy = is_light == 0
    total = int(heavy.sum())
    out = np.full(len(is_light), 255, dtype=np.uint8)
    out[heavy] = [capi.shard_owner_for(total, nshards, h) for h in range(total)]
    return out


@pytest.mark.parametrize("nshards", SHARDS)
def test_closed_form_agrees_with_the_ranges(nshards):
    for heavy in range(1, 301):
        want = owners_by_ranges(heavy, nshards)
        got = np.array([capi.shard_owner_for(heavy, nshards, h) for h in range(heavy)], dtype=np.int64)
        assert np.array_equal(got, want), (heavy, nshards)
        assert (np.diff(got) >= 0).all() and got.max() == nshards - 1    # never falls along h; the last shard ends the list
        if heavy < nshards:                                        # more shards than heavy amplicons: some are empty
            assert len(np.unique(got)) == heavy < nshards


def test_closed_form_in_64_bits():
    heavy, nshards = 2**32 - 1, 64                                 # (h + 1) * 64 passes 2^32 from h = 2^26 on
    for s in (0, 1, 31, 62, 63):
        lo, hi = heavy * s // nshards, heavy * (s + 1) // nshards
        assert capi.shard_owner_for(heavy, nshards, lo) == s and capi.shard_owner_for(heavy, nshards, hi - 1) == s
        if lo > 0:
            assert capi.shard_owner_for(heavy, nshards, lo - 1) == s - 1
    assert capi.shard_owner_for(heavy, nshards, heavy - 1) == 63


@pytest.mark.parametrize("call", [(0, 1, 0), (5, 0, 0), (5, 65, 0), (5, 2, 5), (2**32, 2, 0)])
def test_closed_form_refuses_what_has_no_owner(call):
    with pytest.raises(SwaError) as e:
        capi.shard_owner_for(*call)
    assert e.value.code == capi.SWA_E_ARG


def test_owner_plan():
    tile, turn = capi.shard_owner_plan()
    assert tile >= 4 and tile % 4 == 0 and turn >= 0              # four role bytes a load


@pytest.mark.parametrize("seed", range(6))
def test_roles_from_owner_bytes_equal_the_host_loop(seed):
    rng = np.random.default_rng(seed)
    n = int(rng.integers(1, 700))
    is_light = (rng.random(n) < (0.0, 0.3, 0.5, 0.9, 0.995, 1.0)[seed]).astype(np.uint8)
    for nshards in SHARDS:
        owner = owner_bytes(is_light, nshards)
        for shard in range(nshards):
            roles = np.where(owner == 255, 0, np.where(owner == shard, 1, 2)).astype(np.uint8)
            assert np.array_equal(roles, shard_roles(is_light, shard, nshards)), (nshards, shard)
