"""Every compiled variant of the exact path's kernels, at its own tile edges, bit for bit against the oracle.

k_fill has ten instances (4 / 8 / 12 / 16 slots per thread, temporal or non-temporal stores, 64-bit records), k_lookup three
(<4,false>, <8,false>, <4,true>), cells three sizes or none; tile_q has two producers and the fill may run speculatively.  The
defaults exercise one combination.  Here every instance is selected (by its tuning variable, or by the history of a result handle),
asserted to be in effect through kmx_index_paths / kmx_result_paths — a variable the engine does not recognise leaves the default
in place, and the assertion then fails — and run on batches whose hit lists put the boundary cases on the boundaries of THAT
instance's tile (tests/variant_layouts.py; tests/test_variant_layouts_cpu.py checks the batches themselves).

All searches use the device-buffer form: the host-buffer form answers batches up to 8192 queries on its latency path (k_small),
which runs none of these kernels.  Comparisons are np.array_equal on status, hit_off and positions against the oracle in
MODE_INTENDED; planted queries also against the naive scan of the text."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import variant_layouts as vl
from tests.variant_runs import K, cells_case, dev_search, lookup_text_and_batch, same_answers, small_batches

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FILL_VARIANTS = [("4", False), ("4n", False), ("8", False), ("8n", False), ("12", False), ("12n", False), ("16", False), ("16n", False),
                 ("8", True), ("8n", True)]


class Case:
    """A batch and its expected answer (computed once per tile size, never modified)."""

    def __init__(self, orc, oidx, text, batch):
        self.batch, self.q, self.off = batch, batch.qranks, batch.qoff
        o_off, o_pos, o_st, _ = oidx.search_batch(self.q, self.off, mode=orc.MODE_INTENDED, n_threads=4)
        for a in (o_off, o_pos, o_st):
            a.setflags(write=False)
        self.want = (o_off, o_pos, o_st)
        assert (o_st == 0).all()
        vl.check_events(batch, o_off)
        self.planted = {ev["q"]: orc.naive_scan(text, batch.qs[ev["q"]]) for ev in batch.events if "q" in ev}

    def check(self, got, what):
        same_answers(got, self.want, what)
        ho, pos = got[0], got[1]
        for q, naive in self.planted.items():
            assert np.array_equal(pos[int(ho[q]):int(ho[q + 1])], naive), ("naive scan", what, q)


@pytest.fixture(scope="module")
def world(orc):
    text = vl.make_text()
    lb = vl.LayoutBuilder(text, K)
    oidx = orc.Index(text, vl.SIGMA, [K])
    cache = {}

    def cases(T):
        if T not in cache:
            main = vl.main_batch(lb, T)
            c = {"main": Case(orc, oidx, text, main),
                 "bigger": Case(orc, oidx, text, lb.build(T, vl.EVENT_LAYOUTS + [("total", 2 * main.total + 1)])),
                 "stitch": Case(orc, oidx, text, lb.build(T, ["stitch_straddles", ("total", None)]))}
            for total in (T - 1, T, T + 1, 3 * T, 3 * T + 1):
                c[total] = Case(orc, oidx, text, lb.build(T, [("total", total)]))
            cache[T] = c
        return cache[T]
    return text, cases


def fill_index(engine, monkeypatch, text, variant, rec64, prefix_levels=-1):
    """prefix_levels = -1: no pre-merged levels, so a sub-k query is what the layouts mean — the slice of every k-mer with that prefix
    (several runs, ordered by the prefix kernels) and its tail positions, k_fill's `mid` between them.  With the default levels the same
    queries copy one merged list (one run, the tail merged in)."""
    monkeypatch.delenv("KMX_PREFIX_LEVELS", raising=False)
    monkeypatch.setenv("KMX_FILL_VARIANT", variant)
    if rec64:
        monkeypatch.setenv("KMX_FORCE_REC64", "1")
    else:
        monkeypatch.delenv("KMX_FORCE_REC64", raising=False)
    idx = engine.Index(text, vl.SIGMA, [K], prefix_levels=prefix_levels)          # the variables are read when the index is installed
    assert (idx.levels() == [0]) if prefix_levels < 0 else (idx.levels()[0] >= 1), idx.levels()
    p = idx.paths()
    assert (str(p["fill_slots"]) + ("n" if p["fill_nontemporal"] else ""), p["rec64"]) == (variant, rec64), (variant, rec64, p)
    return idx, 256 * p["fill_slots"]


def check_prefix_events(engine, case, got, n):
    """The sub-k layouts ran as PREFIX queries whose last `tails` hits are tail positions (inside the last k - 1 letters): the
    builder's `mid` is k_fill's."""
    ho, pos, _, kinds = got
    n_seen = 0
    for ev in case.batch.events:
        if "mid" in ev:
            q = ev["q"]
            assert kinds[q] == engine.KIND_PREFIX, (ev["layout"], int(kinds[q]))
            mid = ev["mid"]
            assert (pos[mid:int(ho[q + 1])] > n - K).all() and (pos[int(ho[q]):mid] <= n - K).all() and int(ho[q + 1]) - mid == ev["tails"], ev["layout"]
            n_seen += 1
    assert n_seen == 5


@pytest.mark.gpu
@pytest.mark.parametrize("variant,rec64", FILL_VARIANTS)
def test_fill_variant_at_its_tile_edges(engine, world, monkeypatch, variant, rec64):
    text, cases = world
    idx, T = fill_index(engine, monkeypatch, text, variant, rec64)
    assert T == 256 * int(variant.rstrip("n"))
    c = cases(T)
    main = c["main"]
    idx.stats_enable(True)
    res = engine.Result()
    # a. a fresh handle: no tile table yet, k_partition writes it, nothing is speculative
    got, p = dev_search(idx, main.q, main.off, res)
    main.check(got, "a")
    check_prefix_events(engine, main, got, text.size)
    assert not p["small"] and p["tile_q_source"] == engine.TILE_Q_PARTITION and not p["spec_fill"] and p["fill_tiles"] == main.batch.total // T, p
    # b. the same batch again: the scan writes tile_q, the fill goes out behind it and is kept
    got, p = dev_search(idx, main.q, main.off, res)
    main.check(got, "b")
    assert p["tile_q_source"] == engine.TILE_Q_SCAN and p["spec_fill"] and p["spec_ok"] and p["fill_blocks"] >= p["fill_tiles"], p
    # c. more hits than the handle's buffers hold: the speculative fill ran on a grid that was too small and is redone
    got, p = dev_search(idx, c["bigger"].q, c["bigger"].off, res)
    c["bigger"].check(got, "c")
    assert p["spec_fill"] and not p["spec_ok"] and p["fill_blocks"] == p["fill_tiles"] == (2 * main.batch.total + 1 + T - 1) // T, p
    # d. the small batch again, on the grown buffers: half of the speculative grid is surplus blocks that leave at once
    got, p = dev_search(idx, main.q, main.off, res)
    main.check(got, "d")
    assert p["spec_fill"] and p["spec_ok"] and p["fill_tiles"] == main.batch.total // T and p["fill_blocks"] >= 2 * p["fill_tiles"], p
    # ... and a batch of two tiles: nearly all of it
    got, p = dev_search(idx, c[T + 1].q, c[T + 1].off, res)
    c[T + 1].check(got, "d, two tiles")
    assert p["spec_fill"] and p["spec_ok"] and p["fill_tiles"] == 2 and p["fill_blocks"] > 2 * p["fill_tiles"], p
    # e. counts only, then a filling search
    got, p = dev_search(idx, main.q, main.off, res, flags=engine.SEARCH_COUNT_ONLY)
    assert np.array_equal(got[0], main.want[0]) and np.array_equal(got[2], main.want[2].astype(np.uint8)) and p["tile_q_source"] == engine.TILE_Q_NONE
    got, p = dev_search(idx, main.q, main.off, res)
    main.check(got, "e")
    # ... and a batch with a STITCH query across a boundary (its slots are k_fill's slow path), and the main batch behind it
    got, p = dev_search(idx, c["stitch"].q, c["stitch"].off, res)
    c["stitch"].check(got, "stitch")
    assert got[3][c["stitch"].batch.events[0]["q"]] == engine.KIND_STITCH
    got, p = dev_search(idx, main.q, main.off, res)
    main.check(got, "after stitch")
    # the slices of several runs were put in order by the prefix kernels (k_fill leaves their slots alone)
    st = idx.stats()
    assert sum(v["launches"] for n, v in st.items() if n.startswith("k_prefix")) > 0, st

    # totals around one and three tiles on a second handle; 3T is then exactly what its buffers hold, 3T + 1 one slot more
    # (the first handle stays open: a released one would be handed to the next search, buffers and all)
    res2 = engine.Result()
    seen = []
    for total in (T - 1, T, T + 1, 3 * T, 3 * T, 3 * T + 1):
        got, p = dev_search(idx, c[total].q, c[total].off, res2)
        c[total].check(got, total)
        assert p["fill_tiles"] == (total + T - 1) // T, (total, p)
        seen.append(p)
    assert seen[0]["tile_q_source"] == engine.TILE_Q_PARTITION
    # The first 3T grew the output buffer, the second runs on a speculative grid sized from what that buffer holds.  The edge wanted
    # here is total == spec_tiles * tile: the grid the handle reports must be exactly the tiles in use (the buffer's growth slack, a
    # sixteenth and 256 bytes today, is below one tile; should the allocation policy change, this fails and the totals must follow it).
    assert seen[4]["spec_fill"] and seen[4]["spec_ok"] and seen[4]["fill_blocks"] == seen[4]["fill_tiles"], seen[4]
    # ... and one hit more is one tile more than that grid: launched, not kept, filled again
    assert seen[5]["spec_fill"] and not seen[5]["spec_ok"] and seen[5]["fill_tiles"] == seen[4]["fill_blocks"] + 1, seen[5]
    res2.close()
    res.close()
    idx.close()

    # the same batch on an index WITH prefix levels: its sub-k queries are one-run copies out of a merged list (k_fill's plain PREFIX copy)
    idx, _ = fill_index(engine, monkeypatch, text, variant, rec64, prefix_levels=0)
    res = engine.Result()
    for rep in range(2):
        got, p = dev_search(idx, main.q, main.off, res)
        main.check(got, ("levels", rep))
    assert p["spec_ok"]
    res.close()
    idx.close()


@pytest.mark.gpu
def test_fill_variants_agree_with_one_another(engine, world, monkeypatch):
    """One batch (every layout at T = 3072, so in the middle of the other variants' tiles) through all ten instances, twice each."""
    text, cases = world
    c = cases(3072)["main"]
    outs = []
    for variant, rec64 in FILL_VARIANTS:
        idx, _ = fill_index(engine, monkeypatch, text, variant, rec64, prefix_levels=(-1, 0)[len(outs) % 2])
        res = engine.Result()
        for rep in range(2):
            got, _ = dev_search(idx, c.q, c.off, res)
        c.check(got, (variant, rec64))
        outs.append(got)
        res.close()
        idx.close()
    for got in outs[1:]:
        for a, b in zip(outs[0], got):
            assert np.array_equal(a, b)


# ---------------------------------------------------------------------------------------------------------------------------
# k_lookup variants

LOOKUP_CHILD = r"""
import json, sys
sys.path.insert(0, %(root)r)
import numpy as np
from kmer_index_amd import engine
from oracle import orc
from tests.variant_runs import dev_search, same_answers, lookup_text_and_batch

text = q = None
for table in (engine.TABLE_DENSE, engine.TABLE_OPEN):
    idx = engine.Index(lookup_text_and_batch(1)[0], 4, [7], table=table)
    ip = idx.paths()
    S = ip["scan_tile"]
    if q is None:
        text, q, off = lookup_text_and_batch(3 * S + 5)
        o_off, o_pos, o_st, _ = orc.Index(text, 4, [7]).search_batch(q, off, mode=orc.MODE_INTENDED, n_threads=4)
    res = engine.Result()
    for nq in (1, 255, 256, 1023, 1024, 1025, 2047, 2048, 2049, S - 1, S, S + 1, 3 * S + 5):
        assert nq <= off.size - 1
        nl, nh = int(off[nq]), int(o_off[nq])
        for rep in range(2):
            got, p = dev_search(idx, q[:nl], off[:nq + 1], res)
            same_answers(got, (o_off[:nq + 1], o_pos[:nh], o_st[:nq]), (table, nq, rep))
            print("paths", json.dumps({"table": table, "nq": nq, "cell_shift": ip["cell_shift"], "tiny": ip["tiny_cells"], "items": p["lookup_items"],
                                       "pairs": p["lookup_pairs"], "small": p["small"]}))
    kinds = np.bincount(got[3], minlength=4)
    assert (kinds[1:] > 0).all(), kinds
    res.close()
    idx.close()
print("lookup child ok")
"""


@pytest.mark.gpu
@pytest.mark.parametrize("knob,items,pairs", [("4", 4, False), ("8", 8, False), ("-4", 4, True)])
def test_lookup_variant_by_knob(knob, items, pairs):
    """KMX_LOOKUP_ITEMS is read once per process: a child per value.  nq around the lookup blocks (1024 / 2048 queries) and the scan
    tile: the fused scan consumes scan_tile / (256 * items) block sums per scan block, a wrong sum shifts every later hit_off."""
    e = dict(os.environ)
    e["KMX_LOOKUP_ITEMS"] = knob
    res = subprocess.run([sys.executable, "-c", LOOKUP_CHILD % {"root": ROOT}], capture_output=True, text=True, timeout=600, env=e)
    assert res.returncode == 0 and "lookup child ok" in res.stdout, res.stdout[-2000:] + res.stderr[-4000:]
    rows = [json.loads(line[6:]) for line in res.stdout.splitlines() if line.startswith("paths ")]
    assert len(rows) == 2 * 13 * 2
    for r in rows:
        assert (r["items"], r["pairs"], r["small"]) == (items, pairs, False), (knob, r)
    dense = [r for r in rows if r["table"] == 2]
    assert dense and all(r["cell_shift"] == [3] and r["tiny"] for r in dense), dense[:1]
    assert all(r["cell_shift"] == [0] and not r["tiny"] for r in rows if r["table"] == 1)


@pytest.mark.gpu
def test_lookup_variants_by_history(engine, orc):
    """Without the knob the variant follows the previous batch on the handle: <4,true> behind a batch with cross-referenced queries,
    <8,false> on an index of tiny cells otherwise, <4,false> elsewhere; reads of very many parts are deferred behind a batch that held some."""
    assert "KMX_LOOKUP_ITEMS" not in os.environ
    text, q, off = lookup_text_and_batch(12_000)
    oidx = orc.Index(text, 4, [7])
    lens = np.diff(off.astype(np.int64))

    def batch(keep, n, extra=()):
        ids = np.nonzero(keep)[0][:n]
        qs = [q[int(off[i]):int(off[i + 1])] for i in ids] + list(extra)
        o = np.zeros(len(qs) + 1, np.uint64)
        o[1:] = np.cumsum([len(x) for x in qs])
        qq = np.concatenate(qs).astype(np.uint8)
        return qq, o, oidx.search_batch(qq, o, mode=orc.MODE_INTENDED, n_threads=4)[:3]

    reads = [text[s:s + 5000].copy() for s in (0, 1234, 40_000, 45_000)]
    with_pairs = batch(lens > 0, 3000)
    without = batch(lens <= 7, 3000)
    with_long = batch(lens <= 7, 2000, reads)
    assert (with_long[2][2] == 0).all() and (np.diff(with_long[2][0].astype(np.int64))[-4:] >= 1).all()
    reached = {}
    for table in (engine.TABLE_OPEN, engine.TABLE_DENSE):
        idx = engine.Index(text, 4, [7], table=table)
        tiny = idx.paths()["tiny_cells"]
        assert tiny == (table == engine.TABLE_DENSE)
        res = engine.Result()
        seq = [("pairs", with_pairs), ("after pairs", without), ("plain", without), ("long", with_long), ("after long", without), ("plain again", without)]
        for name, (qq, o, want) in seq:
            got, p = dev_search(idx, qq, o, res)
            same_answers(got, want, (table, name))
            reached[(tiny, name)] = (p["lookup_items"], p["lookup_pairs"], p["deferred_long"])
        res.close()
        idx.close()
    for tiny in (False, True):
        lean = 8 if tiny else 4
        assert reached[(tiny, "pairs")] == (lean, False, False)                    # (a fresh handle has no history)
        assert reached[(tiny, "after pairs")] == (4, True, False)
        assert reached[(tiny, "plain")] == (lean, False, False)
        assert reached[(tiny, "plain again")] == (lean, False, False)
        assert reached[(tiny, "long")] == (lean, False, False)
        assert reached[(tiny, "after long")][2], reached                            # (a read of many parts is a cross-referenced query too)
    assert {v[:2] for v in reached.values()} == {(4, True), (4, False), (8, False)}


# ---------------------------------------------------------------------------------------------------------------------------
# cells

# c = npos / n_keys just ABOVE the thresholds of the default choice — 3.5 (cells of 8 up to there), 10.5 (of 16), 24 (of 32, none
# beyond) — so that the default is the next answer and only a knob that took effect gives the shift asked for:
# (variable, value, shift wanted, n, shift without the variable)
CELLS = [("KMX_CELL_SHIFT", "3", 3, 14_500, 4), ("KMX_CELL_SHIFT", "4", 4, 43_200, 5), ("KMX_CELL_SHIFT", "5", 5, 98_500, 0),
         ("KMX_CELLS", "0", 0, 42_900, 4)]


@pytest.mark.gpu
@pytest.mark.parametrize("var,value,shift,n,default", CELLS)
def test_cell_sizes(engine, orc, monkeypatch, var, value, shift, n, default):
    text, hist, q, off = cells_case(n)
    monkeypatch.delenv("KMX_CELLS", raising=False)
    monkeypatch.delenv("KMX_CELL_SHIFT", raising=False)
    plain = engine.Index(text, 4, [K], table=engine.TABLE_DENSE)
    assert plain.paths()["cell_shift"] == [default] != [shift], plain.paths()       # the variable has something to change
    plain.close()
    monkeypatch.setenv(var, value)
    idx = engine.Index(text, 4, [K], table=engine.TABLE_DENSE)
    assert idx.paths()["cell_shift"] == [shift], idx.paths()
    assert idx.memory()["cells"] == (((4 ** K) << shift) * 4 + 4 ** K if shift else 0)
    edge = 1 << (shift or 4)
    for size in (edge - 1, edge, edge + 1):                        # the last of them does not fit its cell: one more table read
        assert (hist == size).sum() >= 3, (size, int((hist == size).sum()))
    want = orc.Index(text, 4, [K]).search_batch(q, off, mode=orc.MODE_INTENDED, n_threads=4)[:3]
    assert np.array_equal(np.diff(want[0].astype(np.int64))[:4 ** K], hist)
    res = engine.Result()
    for rep in range(2):
        got, p = dev_search(idx, q, off, res)
        same_answers(got, want, (var, value, rep))
        assert not p["small"]
    for c in np.nonzero((hist >= edge - 1) & (hist <= edge + 1))[0][:12]:
        assert np.array_equal(got[1][int(got[0][c]):int(got[0][c + 1])], orc.naive_scan(text, vl.decode(int(c), K)))
    res.close()
    idx.close()


SMALL_CHILD = r"""
import sys
sys.path.insert(0, %(root)r)
from tests.variant_runs import small_batches
print("small child ok", *small_batches())
"""


@pytest.mark.gpu
def test_no_small_knob_gives_the_same_answers():
    """KMX_NO_SMALL (read once per process: a child) sends batches of 1 to 40 queries down the general path on an index with
    cells; here, without it, they take the latency path.  Same answers either way, and the oracle's."""
    assert "KMX_NO_SMALL" not in os.environ
    e = dict(os.environ)
    e["KMX_NO_SMALL"] = "1"
    res = subprocess.run([sys.executable, "-c", SMALL_CHILD % {"root": ROOT}], capture_output=True, text=True, timeout=600, env=e)
    assert res.returncode == 0 and "small child ok" in res.stdout, res.stdout[-2000:] + res.stderr[-4000:]
    path, dg = res.stdout.strip().splitlines()[-1].split()[3:]
    assert path == "general"
    here = small_batches()
    assert here[0] == "small" and here[1] == dg, (here, dg)
