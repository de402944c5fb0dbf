"""Inputs for the tests of SWA_FAST_LONG=split (swarm_amd/csrc/fastidious.hip: fast_plan; include/swarm_amd.h), built from
tests/fastidious_sets.py.  Not product code.

The pair route holds sequences of up to CAP = 1004 nt.  Under the switch, a database with longer sequences keeps the
pair route for the pairs whose two lengths lie in [112, CAP]; every other pair takes the Bloom route.

  long        edit_atlas(LONG, LONG, small): records of 1001 .. 1005 nt, so pairs on both sides of the cap and across it
  three       edit_atlas(112) (110 .. 113 nt: the short band), edit_atlas(150) and the long atlas, headers prefixed by
              s / m / l so that they stay distinct (the `_abundance` suffix stays), and a 3071-nt outlier: the short band,
              the pair route and the long band in one database, the Zobrist table read from memory
  all_long    the records of the long atlas that are longer than CAP (the centroid of LONG nt is one of them): nothing
              for the pair route
  150+X       edit_atlas(150) and an outlier of X nt ("borrowed": the 150-nt pairs under the plan of X)
  150, 1004   edit_atlas(L) alone: the switch does not apply

LONG = 1005: chosen on the oracle's result (tests/test_fastidious_split_identity.py checks it).  edit_atlas(1005, 1005,
small) has graft pairs (light, heavy) of lengths (1004, 1005), (1005, 1004), (1003, 1005) and (1005, 1003), 64 pairs with a
member of 1005 nt and about 100 with both members in 1001 .. 1004: 1006 is not needed."""
from __future__ import annotations

import functools

import numpy as np

import fastidious_sets as FS

CAP = 1004                      # the tests derive it (expected_plan) before they rely on it
MIN_LEN = 112
LONG = 1005
NAMES = ["long", "three", "all_long", "150+1005", "150+3071", "150", "1004"]


def _prefixed(atlas, tag: str):
    recs, three = atlas
    return [(tag + h, s) for h, s in recs], [tag + h for h in three]


@functools.lru_cache(maxsize=None)
def records(name: str):
    """(records, headers of the three-edit sequences) of a set"""
    if name == "long":
        return FS.edit_atlas(LONG, LONG, True)
    if name == "three":
        recs, three = [], []
        for tag, L in (("s", 112), ("m", 150), ("l", LONG)):
            r, t = _prefixed(FS.edit_atlas(L, L, FS.is_small(L)), tag)
            recs += r
            three += t
        return FS.with_outlier(recs, 3071), three
    if name == "all_long":
        recs, three = FS.edit_atlas(LONG, LONG, True)
        keep = [(h, s) for h, s in recs if len(s) > CAP]
        return keep, [h for h in three if h in {k for k, _ in keep}]
    if "+" in name:
        L, X = (int(v) for v in name.split("+"))
        recs, three = FS.edit_atlas(L, L, FS.is_small(L))
        return FS.with_outlier(recs, X), three
    L = int(name)
    return FS.edit_atlas(L, L, FS.is_small(L))


def build(name: str, path):
    """the set written to `path` and clustered on the host from the oracle's network: (db, light flags, three)"""
    import support as S
    from swarm_amd import D1Clusters, HostDb
    recs, three = records(name)
    FS.write_fasta(path, recs)
    db = S.db_from_fasta(path)
    off, nb, dup = S.oracle_d1_network(db)
    assert not dup
    flags, _ = D1Clusters(HostDb(path), off, nb).light_flags(3)
    return db, flags, three


def graft_pair_lengths(db, graft) -> list:
    """(length of the light amplicon, length of its heavy graft candidate) of every graft"""
    return [(int(db.seqlen[x]), int(db.seqlen[graft[x]])) for x in np.flatnonzero(graft != FS.NO_GRAFT)]


def route_of(a, b, cap: int = CAP, min_len: int = MIN_LEN):
    """the rule, on arrays of lengths: (pair route takes the pair, Bloom route takes the pair)"""
    lo, hi = np.minimum(a, b), np.maximum(a, b)
    return (lo >= min_len) & (hi <= cap), (lo < min_len) | (hi > cap)


def in_bands(length, cap: int = CAP, min_len: int = MIN_LEN):
    """amplicons the Bloom route lists: they can be half of a pair the pair route does not take"""
    return (length <= min_len + 1) | (length >= cap - 1)
