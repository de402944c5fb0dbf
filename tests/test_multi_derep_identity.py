"""d = 0 on several GPUs, without one: the owner function (swa_multi_derep_owner_for, a pure function that needs no device)
against its restatement, its range and its balance; and the scheme of swa_multi_derep_resident — slices, records routed by
owner, a minimum per identical sequence at the owner, the results placed — as a host model (tests/multi_derep_sets.py)
against the oracle's dereplication on every read set."""
import math

import numpy as np
import pytest

import multi_derep_sets as MD
from swarm_amd import SwaError
from swarm_amd.capi import derep_owner_for


@pytest.fixture(scope="module")
def sets(tmp_path_factory):
    return MD.make_sets(tmp_path_factory.mktemp("multi_derep_sets"))


def _hashes(count: int, seed: int) -> list:
    rng = np.random.default_rng(seed)
    return [int(h) for h in rng.integers(0, 2**64, size=count, dtype=np.uint64)]


def test_owner_is_below_world_and_zero_alone():
    hashes = _hashes(64, 1) + [0, 1, 2**32 - 1, 2**32, 2**63, 2**64 - 1]
    for world in range(1, 65):
        owners = [derep_owner_for(h, world) for h in hashes]
        assert all(0 <= o < world for o in owners), world
        if world == 1:
            assert owners == [0] * len(hashes)


def test_owner_is_deterministic_and_the_restatement():
    hashes = _hashes(512, 2) + [0, 1, 2**64 - 1]
    for world in (1, 2, 3, 5, 8, 63, 64):
        got = [derep_owner_for(h, world) for h in hashes]
        assert got == [derep_owner_for(h, world) for h in hashes]
        assert got == [MD.owner(h, world) for h in hashes], world


def test_owner_rejects_a_world_outside_1_to_64():
    for world in (0, 65):
        with pytest.raises(SwaError):
            derep_owner_for(1, world)


@pytest.mark.parametrize("world", [2, 3, 8, 64])
def test_owner_balance(world):
    """N = 2^16 random hashes: a rank's count is binomial(N, 1 / world), standard deviation below sqrt(N / world); six of
    them either way holds for every rank of every world here with probability 1 - 1e-7"""
    n = 1 << 16
    counts = np.bincount([derep_owner_for(h, world) for h in _hashes(n, 3)], minlength=world)
    assert counts.sum() == n and len(counts) == world
    bound = 6.0 * math.sqrt(n / world)
    print(world, counts.min(), counts.max(), n / world, bound)
    assert np.all(np.abs(counts - n / world) <= bound), (world, counts)


def test_owner_ignores_nothing_of_the_hash():
    """hashes that agree in their low 32 bits, or in their high 32 bits, still spread over the ranks: the owner is a
    function of the full 64 bits, not of the bits k_derep_claim takes its slot from"""
    for fixed in ([(h << 32) | 0x12345678 for h in range(4096)], [(0x12345678 << 32) | h for h in range(4096)]):
        counts = np.bincount([derep_owner_for(h, 8) for h in fixed], minlength=8)
        assert np.all(np.abs(counts - 512) <= 6.0 * math.sqrt(512)), counts


@pytest.mark.parametrize("world", MD.WORLDS)
@pytest.mark.parametrize("name", MD.NAMES)
def test_model_is_the_oracles_dereplication(sets, name, world):
    _, db, want, seqs = sets[name]
    first, received = MD.model_derep(seqs, world, derep_owner_for)
    assert first.dtype == want.dtype and np.array_equal(first, want)
    assert int(received.sum()) == db.n and len(received) == world
