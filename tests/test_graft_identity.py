"""The grafting of --fastidious in closed form (tests/graft_sets.py: closed_form — the smallest packed pair per light swarm,
the winners sorted by heavy swarm and pair), which is what the reference's sequential walk over the sorted pairs decides,
against D1Clusters.graft; and the install step (swa_d1_result_install_graft), which must leave a result as graft leaves
it.  Random small clusterings, random candidates, a few hundred amplicons each; no GPU.

The result is read off what the writers print: -o (who is printed with whom, in which order: a heavy swarm's own members,
then those of the light swarms it won, in the order it won them), -s (size, mass, singletons, deepest generation of every
printed swarm) and -i (the winning children's candidates); -w, -u and -r as well where two results are compared."""
import filecmp

import numpy as np
import pytest

import graft_sets as GS
from swarm_amd import D1Clusters, HostDb, d1_write_uclust


def _clustered(case, tmp_path):
    fa = tmp_path / "in.fa"
    if not fa.exists():
        GS.write_fasta(fa, case.records)
    hdb = HostDb(fa)
    assert np.array_equal(hdb.abundance, case.abundance) and np.array_equal(hdb.seqlen, case.seqlen)   # (the reader kept the ids)
    offsets, neighbours, _ = case.csr
    cl = D1Clusters(hdb, offsets, neighbours)
    assert np.array_equal(cl.swarmid(), case.want.swarmid) and np.array_equal(cl.generation(), case.want.generation)
    return hdb, cl


def _id(token: bytes) -> int:
    return int(token.split(b"_")[0][1:])


def _written(cl, tmp_path, tag):
    paths = {k: tmp_path / f"{tag}.{k}" for k in "osiwur"}
    cl.write_swarms(paths["o"])
    cl.write_stats(paths["s"])
    cl.write_structure(paths["i"])
    cl.write_seeds(paths["w"])
    d1_write_uclust(cl, paths["u"])
    cl.write_swarms(paths["r"], mothur=True)
    return paths


@pytest.mark.parametrize("seed,n,share", GS.CASES)
def test_closed_form_is_the_sequential_walk(tmp_path, seed, n, share):
    case = GS.make_case(seed, n, share)
    want = case.want
    hdb, cl = _clustered(case, tmp_path)
    flags, stats = cl.light_flags(case.boundary)
    assert np.array_equal(flags, case.light) and stats[0] > 0 and stats[3] > 0
    g = GS.closed_form(want.swarmid, case.cand)
    assert cl.graft(case.cand) == len(g.heavy)
    paths = _written(cl, tmp_path, "walk")

    nswarms = len(want.begins) - 1
    members = [[int(v) for v in want.order[want.begins[s]:want.begins[s + 1]]] for s in range(nswarms)]
    chain = {}
    for h, l in zip(g.heavy.tolist(), g.light.tolist()):
        chain.setdefault(h, []).append(l)
    attached = set(g.light.tolist())
    assert not attached & set(chain)                              # (no light swarm is anybody's heavy swarm)
    printed = [s for s in range(nswarms) if s not in attached]
    # -o: a heavy swarm's own members, then its light swarms' in chain order
    lines = paths["o"].read_bytes().splitlines()
    assert [[_id(t) for t in line.split()] for line in lines] == [members[s] + [a for l in chain.get(s, []) for a in members[l]] for s in printed]
    # -s: the grown sums; the deepest generation stays the heavy swarm's own
    sums = GS.sums_of(want.swarmid, want.generation, case.abundance, case.seqlen, nswarms)
    (mass, _, singles, maxgen), sizes = GS.grown(sums, np.diff(want.begins), g)
    rows = [line.split(b"\t") for line in paths["s"].read_bytes().splitlines()]
    assert [(int(r[0]), int(r[1]), int(r[2][1:]), int(r[4]), int(r[5])) for r in rows] == \
           [(int(sizes[s]), int(mass[s]), members[s][0], int(singles[s]), int(maxgen[s])) for s in printed]
    assert cl.summary()["swarms"] == len(printed) and cl.summary()["largest"] == int(sizes[printed].max())
    # -i: the lines of two differences are the winning (parent, child) pairs, with the parent's generation + 1
    twos = [line.split(b"\t") for line in paths["i"].read_bytes().splitlines() if line.split(b"\t")[2] == b"2"]
    assert sorted((int(r[0][1:]), int(r[1][1:]), int(r[4])) for r in twos) == \
           sorted((int(p), int(c), int(want.generation[p]) + 1) for p, c in zip(g.parent, g.child))

    # the install step on a second result of the same clustering: every file byte for byte, the same summary
    hdb2, cl2 = _clustered(case, tmp_path)
    cl2.install_graft(g.heavy, g.light, g.parent, g.child)
    assert cl2.summary() == cl.summary()
    for k, path in _written(cl2, tmp_path, "installed").items():
        assert filecmp.cmp(path, paths[k], shallow=False), k


def test_the_cases_exercise_the_walk():
    """over the seeds: light swarms with several candidate children, several parents for one child's swarm, several light
    swarms won by one heavy swarm, candidates withdrawn, and a case without any candidate"""
    seen = {}
    for seed, n, share in GS.CASES:
        case = GS.make_case(seed, n, share)
        for k, v in GS.properties(case.want.swarmid, case.cand).items():
            seen[k] = seen.get(k, 0) + int(v)
        assert case.light.any() and not case.light.all()
        assert not set(case.want.swarmid[case.cand[case.cand != GS.NO]].tolist()) & set(case.want.swarmid[case.cand != GS.NO].tolist())
    print(seen)
    assert all(seen[k] >= 1 for k in ("several_children", "several_parents", "several_lights_one_heavy", "withdrawn", "no_candidates")), seen


def test_install_refuses_what_is_no_graft(tmp_path):
    """a swarm the result does not have, a light swarm listed twice, a heavy swarm that is itself attached: SWA_E_ARG,
    nothing installed; candidates that hang a swarm on an attached swarm: graft() makes none"""
    from swarm_amd import SwaError, capi
    case = GS.make_case(*GS.CASES[2])
    hdb, cl = _clustered(case, tmp_path)
    g = GS.closed_form(case.want.swarmid, case.cand)
    assert len(g.heavy) >= 2
    before = cl.summary()
    nswarms = len(case.want.begins) - 1
    free = next(s for s in range(nswarms) if s not in set(g.light.tolist()) | set(g.heavy.tolist()))
    one_more = lambda heavy, light: (np.append(g.heavy, heavy), np.append(g.light, light), np.append(g.parent, 0), np.append(g.child, 0))
    bad = [one_more(nswarms, free),                               # a swarm the result does not have
           one_more(g.heavy[0], g.light[0]),                      # a light swarm twice
           one_more(g.light[0], free)]                            # hung on a swarm that is attached itself
    for four in bad:
        with pytest.raises(SwaError) as e:
            cl.install_graft(*four)
        assert e.value.code == capi.SWA_E_ARG
        assert cl.summary() == before
    # the same from candidates: a member of a free swarm names a member of a light swarm that is won itself — no graft at all
    ill = case.cand.copy()
    ill[case.want.order[case.want.begins[free]]] = case.want.order[case.want.begins[g.light[0]]]
    assert cl.graft(ill) == 0 and cl.summary() == before and cl.graft_route() == 0
    cl.install_graft(g.heavy, g.light, g.parent, g.child)
    assert cl.summary()["swarms"] == before["swarms"] - len(g.heavy)
