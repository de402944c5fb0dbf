"""The filter of the --fastidious Bloom route (swarm_amd/csrc/fastidious.hip: fastidious_bloom_route, k_d1_flex<ZLDS, 0 | 1>,
flex_word) against tests/bloom_model.py, across -y (bloom_bits 2 .. 64, so k from 1 to 25), filters from one word to
9.9 M words of every parity, and --ceiling.

A Bloom filter has no false negatives and every survivor is verified, so graft candidates and counters are the same
whatever the filter holds: the tests of tests/test_bloom_forms_gpu.py cannot see a wrong word index, a wrong pattern or a
heavy pass that ignores the filter.  swa_d1_fastidious_bloom_read shows what they cannot: the words as the light pass left
them and the number of heavy microvariants that passed.  The model states both in integers from the oracle's hashes
(tests/test_bloom_model_identity.py checks it without a GPU), and everything here is integer equality.

Every database here is the Bloom route's by its lengths (longest < 112, or > 1004): SWA_FAST_BLOOM is not needed."""
import filecmp
import functools
import re
import subprocess

import numpy as np
import pytest

import bloom_model as B
import plain_sets as P
import support as S
from d1_sets import upload
from swarm_amd import D1Clusters, HostDb, SwaError
from swarm_amd import capi

pytestmark = pytest.mark.gpu
HOOK = "SWA_FAST_TASK_CAP"
BIN = S.ROOT / "swarm_amd" / "bin" / "swarm"
GRID_LENGTHS = (2, 31, 63, 64)
GRID_BITS = (2, 3, 5, 7, 16, 63, 64)


def _batch_set_short_first():
    """plain_sets.batch_set with its first two heavy amplicons cut to 2 nt (GG, TT): they have 17 microvariants each where
    the 16-nt ones had 101, so that few pass even a filter of 2 bits a nucleotide, and the loop's optimistic second batch overflows there too"""
    db, flags = P.batch_set()[:2]
    recs = [(db.headers[i], (("GG", "TT")[i] if i < 2 else db.seq_str(i)).encode()) for i in range(db.n)]
    short = S.build_db(recs)
    assert short.headers == db.headers and short.longest == db.longest
    return short, flags


CASES = {"batch": lambda: P.batch_set()[:2], "batch_short": _batch_set_short_first, "long": lambda: P.long_shell_case(3071)[:2],
         "hand2": lambda: B.hand_case(2), "hand5": lambda: B.hand_case(5)}


def _case(key):
    return CASES[key]() if key in CASES else P.shell_case(key)[:2]


@functools.lru_cache(maxsize=None)
def _model(key, bits: int) -> dict:
    """computed once per (database, bits), shared by the tests, never written to"""
    mo = B.flex_model(*_case(key), bits)
    mo["words"].setflags(write=False)
    return mo


@functools.lru_cache(maxsize=None)
def _oracle(key, bits: int):
    graft, counters = S.oracle_fastidious(*_case(key), bits)
    graft.setflags(write=False)
    return graft, [int(x) for x in counters[:5]]


def _resident(ctx, db):
    upload(ctx, db)
    assert ctx.d1_index_build() is False


def _pass(ctx, db, flags, bits, shard=None):
    """one pass on the resident database (the pass re-purposes the table: the index is made again first)"""
    assert ctx.d1_index_build() is False
    light_nt = int(db.seqlen[flags != 0].astype(np.uint64).sum())
    graft, counters = ctx.d1_fastidious(flags, light_nt, bits, *(shard or ()))
    return graft, [int(x) for x in counters[:5]]


def _check_filter(ctx, mo, bits, label, tasks=None):
    """the view of the last pass against the model: the four parameters, the words, the tasks"""
    facts, words = ctx.d1_fastidious_bloom_read()
    wrong = int((words != mo["words"]).sum()) if words is not None and len(words) == mo["fsize"] else -1
    print(f"{label}: facts {facts} model fsize {mo['fsize']} m {mo['m']} k {mo['k']} tasks {mo['tasks']} of {mo['heavy_variants']} "
          f"words that differ {wrong} batches {ctx.d1_fastidious_bloom_batches()}")
    assert facts[:4] == [mo["fsize"], mo["m"], mo["k"], bits] and facts[5:] == [0, 0, 0], label
    assert words is not None and words.dtype == np.uint64 and np.array_equal(words, mo["words"]), label
    assert facts[4] == (mo["tasks"] if tasks is None else tasks), label
    return facts, words


# ---- the parameter grid ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("bits", GRID_BITS)
@pytest.mark.parametrize("L", GRID_LENGTHS)
def test_filter_across_bits_and_sizes(gpu_ctx, L, bits):
    """L = 2: filters of 2 to 91 words; L = 31 .. 64: odd and even sizes that are no power of two, up to 300 251 words;
    63 / 64 either side of the third staged word.  bits 2 .. 64: k = 1, 1, 2, 2, 6, 25, 25."""
    db, flags = _case(L)
    mo = _model(L, bits)
    want_graft, want_counters = _oracle(L, bits)
    assert db.longest < 112 and 0 < mo["tasks"] < mo["heavy_variants"]       # the filter decides something
    _resident(gpu_ctx, db)
    assert gpu_ctx.d1_fastidious_plan()[0] == 0
    graft, counters = _pass(gpu_ctx, db, flags, bits)
    assert np.array_equal(graft, want_graft) and counters == want_counters
    facts, _ = _check_filter(gpu_ctx, mo, bits, f"shells {L} bits {bits}")
    batches = gpu_ctx.d1_fastidious_bloom_batches()
    assert batches[:2] == [1, 0] and batches[3] == facts[4]                   # one launch: its tasks are all the tasks


def test_grid_reaches_what_it_claims():
    """(no GPU needed, kept beside the grid it describes) the sizes: one word at the floor, odd and even ones, none a
    power of two above 4, k from 1 to 25"""
    fsizes = {B.sizes(int(_case(L)[0].seqlen[_case(L)[1] != 0].sum()), bits)[2] for L in GRID_LENGTHS for bits in GRID_BITS}
    assert min(fsizes) == 2 and max(fsizes) == 300251
    assert sum(f % 2 for f in fsizes) >= 8 and sum(1 - f % 2 for f in fsizes) >= 8
    assert all(f & (f - 1) for f in fsizes if f > 4)
    assert sorted({B.k_of(b) for b in GRID_BITS}) == [1, 2, 6, 25]


# ---- the floor of m ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("light_len,m", [(2, 64), (5, 70)])
def test_minimum_filter(gpu_ctx, light_len, m):
    """one heavy centre and one light amplicon two edits away at bits 2: 28 bits lifted to m = 64, and 70 bits = 9 bytes
    truncated to one word; fsize = 1, where every index is 0"""
    key = f"hand{light_len}"
    db, flags = _case(key)
    mo = _model(key, 2)
    assert [mo["fsize"], mo["m"], mo["k"]] == [1, m, 1] and mo["tasks"] > 0
    _resident(gpu_ctx, db)
    graft, counters = _pass(gpu_ctx, db, flags, 2)
    facts, words = gpu_ctx.d1_fastidious_bloom_read()
    print(f"minimum filter, light {light_len} nt: facts {facts} word {int(words[0]):#018x} model {int(mo['words'][0]):#018x}")
    assert facts == [1, m, 1, 2, mo["tasks"], 0, 0, 0]
    assert len(words) == 1 and int(words[0]) == int(mo["words"][0])
    assert graft.tolist() == [P.NO_GRAFT, 0]
    want_graft, want_counters = _oracle(key, 2)
    assert np.array_equal(graft, want_graft) and counters == want_counters


# ---- the Zobrist table in HBM ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("bits", [2, 64])
def test_filter_with_the_zobrist_table_in_hbm(gpu_ctx, bits):
    """k_d1_flex<false, .>: long_shell_case(3071) whole — 459 light and 406 heavy amplicons, 9.1 M light and 4.5 M heavy
    microvariants, filters of 308 218 and 9 862 979 words.  At bits 2 a third of the heavy microvariants pass (1.6 M tasks),
    more than the oracle can probe in a test's time on a CPU; candidates and counters do not depend on the filter (no false
    negative, every survivor verified), so both cases are held against the oracle's pass at 64 bits, m and k against the model."""
    db, flags = _case("long")
    mo = _model("long", bits)
    want_graft, want_counters = _oracle("long", 64)
    assert db.longest == 3071 and 0 < mo["tasks"] < mo["heavy_variants"]
    _resident(gpu_ctx, db)
    plan = gpu_ctx.d1_fastidious_plan()
    assert plan[0] == 0 and plan[6] == 0
    graft, counters = _pass(gpu_ctx, db, flags, bits)
    assert np.array_equal(graft, want_graft)
    assert counters == want_counters[:3] + [mo["m"], mo["k"]]
    facts, _ = _check_filter(gpu_ctx, mo, bits, f"long shells 3071 bits {bits}")
    batches = gpu_ctx.d1_fastidious_bloom_batches()
    assert batches[:2] == [1, 0] and batches[3] == facts[4]


# ---- under the batch hook ----------------------------------------------------------------------------------------------------

def _batch_loop(per_heavy, cap: int, maxv: int) -> list:
    """fastidious_bloom_route's batch loop on the model's tasks per heavy amplicon, in list order: [launches, redone, cap in
    effect, fullest batch that ran].  The first batch cannot overflow (cap / maxv amplicons); the next ones are sized for
    four times the rate just seen, and one that overflows is launched again, sized by its own rate."""
    task_cap = max(cap, maxv)
    floor = task_cap // maxv
    done, rate, launches, redone, fullest = 0, -1.0, 0, 0, 0
    while done < len(per_heavy):
        want = floor if rate < 0.0 else max(int(task_cap / (4.0 * rate + 1.0)), floor)
        want = min(want, len(per_heavy) - done)
        got = int(sum(per_heavy[done:done + want]))
        rate = got / want
        launches += 1
        if got > task_cap:
            redone += 1
            continue
        fullest = max(fullest, got)
        done += want
    return [launches, redone, task_cap, fullest]


@pytest.mark.parametrize("key,bits,redo", [("batch", 16, True), ("batch", 2, False), ("batch_short", 2, True), ("batch_short", 16, True)])
def test_tasks_of_a_redone_batch_count_once(gpu_ctx, monkeypatch, key, bits, redo):
    """plain_sets.batch_set under a cap of one heavy amplicon's worth of tasks: several launches, one of them overflows
    and is redone smaller.  The filter is the light pass's and does not change; the task sum counts the batches that ran,
    the redone one once.  These sets have at most 64 amplicons, so the heavy list is in id order and the loop can be
    followed on the model's tasks per heavy amplicon: launches, redone batches and the fullest batch are compared too.
    At 2 bits batch_set itself redoes nothing — its first heavy amplicon, though nothing lies near it, has 37 of its 101
    microvariants pass so small a filter, and a batch sized for four times that rate cannot overflow (the dense ones make
    68 at the most) — hence batch_short, whose first two heavy amplicons are 2 nt long: redone at 2 bits and at 16."""
    db, flags = _case(key)
    cap = P.batch_set()[3]
    mo = _model(key, bits)
    want_graft, want_counters = _oracle(key, bits)
    heavy = np.flatnonzero(flags == 0)
    assert db.n <= 64 and cap == 7 * db.longest + 4
    per_heavy = np.bincount(mo["task_list"]["heavy"], minlength=db.n)[heavy].tolist()
    want_batches = _batch_loop(per_heavy, cap, cap)
    assert (want_batches[1] >= 1) == redo and want_batches[0] >= 3
    _resident(gpu_ctx, db)
    graft, counters = _pass(gpu_ctx, db, flags, bits)
    assert np.array_equal(graft, want_graft) and counters == want_counters
    _, free_words = _check_filter(gpu_ctx, mo, bits, f"{key} bits {bits}, hook off")
    assert gpu_ctx.d1_fastidious_bloom_batches() == [1, 0, len(heavy) * cap, mo["tasks"]] and mo["tasks"] > cap
    monkeypatch.setenv(HOOK, str(cap))
    graft, counters = _pass(gpu_ctx, db, flags, bits)
    assert np.array_equal(graft, want_graft) and counters == want_counters
    _, words = _check_filter(gpu_ctx, mo, bits, f"{key} bits {bits}, hook on")      # facts[4]: every task once
    launches, redone, cap_used, fullest = gpu_ctx.d1_fastidious_bloom_batches()
    assert cap_used == cap and fullest <= cap and launches >= 3
    if redo:
        assert redone >= 1
    assert [launches, redone, cap_used, fullest] == want_batches
    assert np.array_equal(words, free_words)


# ---- two shards --------------------------------------------------------------------------------------------------------------

def test_each_shard_builds_the_whole_filter(gpu_ctx):
    db, flags = _case(64)
    mo = _model(64, 2)
    want_graft, _ = _oracle(64, 2)
    _resident(gpu_ctx, db)
    grafts, tasks = [], []
    for shard in range(2):
        graft, _ = _pass(gpu_ctx, db, flags, 2, (shard, 2))
        facts, _ = gpu_ctx.d1_fastidious_bloom_read(words=False)
        _check_filter(gpu_ctx, mo, 2, f"shells 64 bits 2 shard {shard}", tasks=facts[4])
        grafts.append(graft)
        tasks.append(facts[4])
    assert sum(tasks) == mo["tasks"] and all(0 < t < mo["tasks"] for t in tasks)
    assert np.array_equal(np.minimum(grafts[0], grafts[1]), want_graft)


# ---- no Bloom route, errors, what ends the view -------------------------------------------------------------------------------

def _raw_read(ctx, buf, cap):
    facts = np.full(8, 7, dtype=np.uint64)
    rc = ctx.lib.swa_d1_fastidious_bloom_read(ctx.h, capi._ptr(facts), capi._ptr(buf), cap)
    return rc, [int(v) for v in facts]


def test_no_bloom_route_nothing_to_read(gpu_ctx, tmp_path):
    """a database of 150-nt amplicons (the set of test_bloom_forms_gpu.py's test_no_bloom_route_no_report): every pair is
    the pair route's; the facts are zero and a buffer of any capacity is left as it was.  A pass on the Bloom route comes
    first, so that there is a filter in HBM that must not be shown."""
    db, flags = _case(2)
    _resident(gpu_ctx, db)
    _pass(gpu_ctx, db, flags, 16)
    assert gpu_ctx.d1_fastidious_bloom_read()[0][0] == _model(2, 16)["fsize"]
    fa = tmp_path / "in.fa"
    S.gen_fasta(fa, 3000, 150, 62, 1, 0.3)
    db = S.db_from_fasta(fa)
    off, nb, _ = S.oracle_d1_network(db)
    flags = np.asarray(D1Clusters(HostDb(fa), off, nb).light_flags(3)[0], dtype=np.uint8)
    assert int(db.seqlen.min()) > 113
    _resident(gpu_ctx, db)
    graft, counters = _pass(gpu_ctx, db, flags, 16)
    want_graft, want_counters = S.oracle_fastidious(db, flags, 16)
    assert np.array_equal(graft, want_graft) and counters == [int(x) for x in want_counters[:5]]
    assert gpu_ctx.d1_fastidious_plan()[0] == 1 and gpu_ctx.d1_fastidious_bloom_batches() == [0, 0, 0, 0]
    assert gpu_ctx.d1_fastidious_bloom_read() == ([0] * 8, None)
    for cap in (0, 1, 1000):
        buf = np.full(1000, 0x5A5A5A5A5A5A5A5A, dtype=np.uint64)
        assert _raw_read(gpu_ctx, buf, cap) == (capi.SWA_OK, [0] * 8)
        assert (buf == 0x5A5A5A5A5A5A5A5A).all()


def test_capacity_error_then_success_and_an_upload_ends_the_view(gpu_ctx):
    db, flags = _case(31)
    mo = _model(31, 5)
    _resident(gpu_ctx, db)
    _pass(gpu_ctx, db, flags, 5)
    before = (gpu_ctx.d1_fastidious_bloom_batches(), gpu_ctx.d1_fastidious_totals())
    want_facts = [mo["fsize"], mo["m"], mo["k"], 5, mo["tasks"], 0, 0, 0]
    with pytest.raises(SwaError) as err:
        gpu_ctx.d1_fastidious_bloom_read(cap_words=mo["fsize"] - 1)
    assert err.value.code == capi.SWA_E_CAPACITY
    buf = np.full(mo["fsize"], 0x5A5A5A5A5A5A5A5A, dtype=np.uint64)          # the raw call: facts valid, buffer untouched
    assert _raw_read(gpu_ctx, buf, mo["fsize"] - 1) == (capi.SWA_E_CAPACITY, want_facts)
    assert (buf == 0x5A5A5A5A5A5A5A5A).all()
    _check_filter(gpu_ctx, mo, 5, "after the capacity error")
    _check_filter(gpu_ctx, mo, 5, "read again")                                # reading changes nothing
    assert gpu_ctx.d1_fastidious_bloom_read(words=False) == (want_facts, None)
    assert (gpu_ctx.d1_fastidious_bloom_batches(), gpu_ctx.d1_fastidious_totals()) == before
    upload(gpu_ctx, db)                                                        # the filter was the previous upload's
    assert gpu_ctx.d1_fastidious_bloom_read() == ([0] * 8, None)
    assert _raw_read(gpu_ctx, buf, len(buf)) == (capi.SWA_OK, [0] * 8) and (buf == 0x5A5A5A5A5A5A5A5A).all()
    _resident(gpu_ctx, db)
    _pass(gpu_ctx, db, flags, 5)
    _check_filter(gpu_ctx, mo, 5, "a pass after the upload")


# ---- the command line: -y and -c ----------------------------------------------------------------------------------------------

CLI_N, CLI_SEED, CEILING = 36000, 71, 40
OUTS = "osiwj"
FLAG = {"o": "-o", "s": "-s", "i": "-i", "w": "-w", "j": "-j"}
RUNS = {"default": [], "y2": ["-y", "2"], "y64": ["-y", "64"], "y64_c40": ["-y", "64", "-c", str(CEILING)]}
SHRINK_LINE = "Reducing memory used for Bloom filter due to --ceiling option."


def cli_bits(asked: int, ceiling: int, x: int) -> int:
    """the bits in effect (swarm_amd/csrc/host/main.cpp, as src/algod1.cc:1337-1396): the ceiling in MB buys 8 budget /
    (7 X) bits a nucleotide, and shrinks the bits when that is fewer than asked for"""
    if ceiling:
        return min(asked, 8 * ceiling * 1024 * 1024 // (7 * x))
    return asked


@pytest.fixture(scope="module")
def cli_runs(tmp_path_factory):
    """36 000 amplicons of about 80 nt (longest < 112: the Bloom route by default), `swarm -d 1 -f` four times, and once
    the reference where it is built.  X, the nucleotides in light swarms, is known before any run."""
    d = tmp_path_factory.mktemp("bloom_cli")
    fa = d / "in.fa"
    S.gen_fasta(fa, CLI_N, 80, CLI_SEED, 1, 0.3)
    db = S.db_from_fasta(fa)
    off, nb, dup = S.oracle_d1_network(db)
    assert not dup and db.longest < 112
    x = int(D1Clusters(HostDb(fa), off, nb).light_flags(3)[1][2])
    # -y 64 -c 40 must shrink the bits (8 * 40 * 2^20 / (7 * 64) = 748 982.9) and leave at least two
    assert x > 748983 and 8 * CEILING * 2 ** 20 // (7 * x) >= 2
    logs = {}
    for name, extra in RUNS.items():
        cmd = [str(BIN), "-d", "1", "-f"] + extra
        for k in OUTS:
            cmd += [FLAG[k], str(d / f"{name}.{k}")]
        r = subprocess.run(cmd + ["-l", str(d / f"{name}.log"), str(fa)], capture_output=True, text=True)
        assert r.returncode == 0, (name, r.stderr)
        logs[name] = (d / f"{name}.log").read_text()
    have_ref = S.have_reference()
    if have_ref:                                                 # no -y, no -c: its shrink is computed from its own resident memory
        cmd = ["-d", "1", "-f"]
        for k in OUTS:
            cmd += [FLAG[k], str(d / f"ref.{k}")]
        r = S.run_ref_swarm(cmd + ["-l", str(d / "ref.log"), str(fa)])
        assert r.returncode == 0, r.stderr
    return {"dir": d, "x": x, "logs": logs, "have_ref": have_ref}


def test_cli_outputs_do_not_depend_on_the_filter(cli_runs):
    d = cli_runs["dir"]
    for name in list(RUNS)[1:]:
        for k in OUTS:
            assert filecmp.cmp(d / f"default.{k}", d / f"{name}.{k}", shallow=False), (name, k)
    assert (d / "default.o").stat().st_size > 0 and "Got " in cli_runs["logs"]["default"]
    if cli_runs["have_ref"]:
        for k in OUTS:
            assert filecmp.cmp(d / f"default.{k}", d / f"ref.{k}", shallow=False), k


def test_cli_log_states_the_filter_in_effect(cli_runs):
    x = cli_runs["x"]
    shrunk = cli_bits(64, CEILING, x)
    assert 2 <= shrunk < 64
    for name, asked, ceiling in (("default", 16, 0), ("y2", 2, 0), ("y64", 64, 0), ("y64_c40", 64, CEILING)):
        log = cli_runs["logs"][name]
        assert f"Total length of amplicons in light swarms: {x}\n" in log, name
        bits = cli_bits(asked, ceiling, x)
        m, _, _ = B.sizes(x, bits)
        got = re.findall(r"^Bloom filter: bits=(\d+), m=(\d+), k=(\d+), size=[0-9.]+MB$", log, re.M)
        print(f"{name}: X {x} bits {bits} m {m} k {B.k_of(bits)} log {got}")
        assert got == [(str(bits), str(m), str(B.k_of(bits)))], name
        assert (SHRINK_LINE in log) == (name == "y64_c40"), name
