"""SAM tags on the GPU: kmx_scripts_md, kmx_rescues_md, kmx_placements_mapq, the tags of Index.map_pairs / map_reads_strands and
engine.sam_lines on their results.  The oracle is always tests/md_naive.py or tests/mapq_naive.py applied to the engine's own host
views; every array and every counter must be bit-identical.  The texts, the reads, the chain settings and the helpers are those of
tests/chain_data.py and tests/chain_checks.py; nothing larger runs on the device."""
import ctypes as C
import re

import numpy as np
import pytest

from tests import fold_naive as fn
from tests import mapq_naive as qn
from tests import md_naive as mn
from tests import pair_naive as pn
from tests.chain_checks import check_md, check_rebuild, close_all, dev_array, read_of_entries, same, spell
from tests.chain_data import (ALIGN, CHAIN, COMPLEMENT, INSERT, JOBS, LETTERS, N_PAIRS, PAIRS, PAIR_WORKLOADS as WORKLOADS, PLACEMENTS, REPEAT_CHAIN,
                              RESCUE_FLOORS, SCRIPTS, pairs_of, repeat_pair, repeat_text, rescue_pairs_of, text_of)
from tests.helpers import pack

pytestmark = pytest.mark.gpu

E = CHAIN["max_edits"]


def check_mapq(mq, pl, max_edits, pairs=None, **opts):
    _, strand, dist, _, _, second = pl.host(best2=False)
    pr = {} if pairs is None else dict(zip(("cls", "score", "second_score"), [pairs.host()[k] for k in (0, 2, 3)]))
    want, counts = qn.mapq(strand, dist, second, max_edits, **opts, **pr)
    got = mq.host()
    assert got.dtype == np.uint8 and np.array_equal(got, want) and mq.counts() == counts
    assert np.array_equal(dev_array(mq.device_ptrs()[0], want.size, np.uint8), want)
    return want


class Work:
    """the indexes and, per workload, map_pairs(scripts=True) of tests/chain_data.pairs_of"""

    def __init__(self, engine):
        self.engine = engine
        self.indexes, self.mapped = {}, {}

    def index(self, name):
        if name not in self.indexes:
            sigma, k, n = WORKLOADS[name]
            self.indexes[name] = self.engine.Index(text_of(sigma, n), sigma, [k], table=2)
        return self.indexes[name]

    def workload(self, name):
        if name not in self.mapped:
            sigma, k, _ = WORKLOADS[name]
            self.mapped[name] = self.index(name).map_pairs(*pairs_of(name), k, np.asarray(COMPLEMENT[sigma], np.uint8), **CHAIN, **INSERT, scripts=True)
        return self.mapped[name]

    def close(self):
        for out in self.mapped.values():
            for h in reversed(out):
                h.close()
        for idx in self.indexes.values():
            idx.close()


@pytest.fixture(scope="module")
def work(engine):
    w = Work(engine)
    yield w
    w.close()


# ---- 1. MD of the placements' scripts -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(WORKLOADS))
def test_md_of_the_workload_equals_the_oracle_and_rebuilds_the_text(work, name):
    sigma, _, n = WORKLOADS[name]
    text = text_of(sigma, n)
    reads, loci, al, pl, pairs, sc = work.workload(name)
    before = (sc.host(), al.host(), sc.device_ptrs(), al.device_ptrs(), sc.counts(), al.counts())
    md = sc.md(work.index(name), al, LETTERS[sigma])
    try:
        _, start, end = al.host()[:3]
        strings = check_md(md, sc, start, end, text, sigma)
        assert md.counts()["n_mismatched"] == 0 and md.counts()["n_sel"] == pl.counts()["n_placed"] >= 400
        ranks2, roff2 = fn.double_reads(*pairs_of(name), COMPLEMENT[sigma], sigma)
        check_rebuild(strings, sc, ranks2, roff2, start, end, text, sigma)
        # what the batch must contain, counted on the oracle's strings (check_md has compared them)
        reverse = read_of_entries(sc.host()[0]) % 2 == 1
        letter = np.asarray([bool(re.search(r"[0-9][A-Z]", s)) for s in strings])
        caret = np.asarray(["^" in s for s in strings])
        assert letter.sum() >= 20 and caret.sum() >= 20 and (reverse & (letter | caret)).sum() >= 20
        assert (~letter & ~caret).sum() >= 100                 # and plain matches
        # the scripts and the alignments are untouched
        after = (sc.host(), al.host(), sc.device_ptrs(), al.device_ptrs(), sc.counts(), al.counts())
        assert before[2:] == after[2:]
        same(SCRIPTS, after[0], before[0])
        same(ALIGN, after[1], before[1])
        # one string per public read, where the CIGARs are
        per_read, cigars = pl.mds(md, sc), pl.cigars(sc)
        assert len(per_read) == 2 * N_PAIRS and [bool(s) for s in per_read] == [bool(s) for s in cigars]
        assert sorted(s for s in per_read if s) == sorted(strings)
    finally:
        md.close()


# ---- 2. MD of the rescued mates --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(RESCUE_FLOORS))
def test_md_of_the_rescued_mates(work, name):
    sigma, k, n = WORKLOADS[name]
    text, idx = text_of(sigma, n), work.index(name)
    ranks, roff = rescue_pairs_of(name)
    held = list(idx.map_pairs(ranks, roff, k, np.asarray(COMPLEMENT[sigma], np.uint8), **CHAIN, **INSERT, rescue=True))
    try:
        reads, res = held[0], held[5]
        rsc = res.scripts(idx, reads)
        held.append(rsc)
        rmd = rsc.md(idx, res, LETTERS[sigma])
        held.append(rmd)
        jobs = res.host()
        start, end, status = jobs[5], jobs[6], jobs[7]
        strings = check_md(rmd, rsc, start, end, text, sigma)
        assert rmd.counts()["n_mismatched"] == 0 and len(strings) == RESCUE_FLOORS[name] == 75 == int((status == 3).sum())
        assert np.array_equal(rsc.host()[1], np.flatnonzero(status == 3))
        # The 8 planted substitutions of every rescued mate: 8 mismatch letters, except where the substitution next to an end of the
        # read meets a neighbour of the text that equals the letter beside it.  Then the alignment's own rule (the largest start, the
        # smallest end) turns that one substitution into an insertion at the same distance, and the MD has 7 letters beside a 1I in
        # the CIGAR: 26 of the 75 mates on the dna4 text and 6 of 75 on the 20-letter text (counted with script_naive on the CPU).
        cigars = rsc.strings()
        letters = np.asarray([len(re.findall(r"[A-Z]", s)) for s in strings])
        n_x = np.asarray([sum(int(a) for a in re.findall(r"([0-9]+)X", c)) for c in cigars])
        n_i = np.asarray([sum(int(a) for a in re.findall(r"([0-9]+)I", c)) for c in cigars])
        assert not any("^" in s for s in strings) and not any("D" in c for c in cigars)
        assert np.array_equal(letters, n_x) and np.array_equal(n_x + n_i, np.full(75, 8)) and (n_i <= 1).all()
        assert int((letters == 8).sum()) == {"dna4_k10": 49, "aa20_k5": 69}[name]
        ranks2, roff2 = fn.double_reads(ranks, roff, COMPLEMENT[sigma], sigma)
        check_rebuild(strings, rsc, ranks2, roff2, start, end, text, sigma)
        per_read, cigars = res.mds(rmd, rsc), res.cigars(rsc)
        assert len(per_read) == 2 * N_PAIRS and [bool(s) for s in per_read] == [bool(s) for s in cigars] and sum(bool(s) for s in per_read) == 75
    finally:
        close_all(held)


# ---- 3. every aligned locus of single-strand reads; '=' and 'X' joined are refused ------------------------------------------------------
def test_md_of_all_scripts_of_map_reads_and_the_refusal_of_m_scripts(work):
    name = "dna4_k10"
    sigma, k, n = WORKLOADS[name]
    engine, idx, text = work.engine, work.index(name), text_of(sigma, n)
    ranks, roff = pairs_of(name)
    ranks, roff = ranks[:int(roff[200])], roff[:201]
    held = list(idx.map_reads(ranks, roff, k, **CHAIN))
    try:
        loci, al = held
        sc = al.scripts(idx, loci, ranks, roff, all=True)
        held.append(sc)
        md = sc.md(idx, al, LETTERS[sigma])
        held.append(md)
        _, start, end = al.host()[:3]
        strings = check_md(md, sc, start, end, text, sigma)
        assert md.counts()["n_mismatched"] == 0 and len(strings) == al.counts()["n_aligned"] >= 60
        check_rebuild(strings, sc, ranks, roff, start, end, text, sigma)
        full = md.counts()
        sc_m = al.scripts(idx, loci, ranks, roff, m=True)
        held.append(sc_m)
        o = engine.MdOptions(8, 0)
        table = np.frombuffer(LETTERS[sigma].encode(), np.uint8).copy()
        L = engine.lib()
        assert full["n_sel"] > 0 and md.device_ptrs()[0]
        assert L.kmx_scripts_md(idx._h, sc_m._h, al._h, table.ctypes.data, C.byref(o), None, C.byref(md._h)) == 1
        assert b"KMX_SCRIPT_M" in L.kmx_last_error()
        assert md.counts() == dict(n_sel=0, n_bytes=0, n_mismatched=0) and md.device_ptrs() == (None, None)
        assert md.host()[0].tolist() == [0] and md.host()[1].size == 0 and md.strings() == []
        with pytest.raises(engine.KmxError):
            sc_m.md(idx, al, LETTERS[sigma])
        with pytest.raises(TypeError):
            sc.md(idx, loci, LETTERS[sigma])
        # the handle serves again
        sc.md(idx, al, LETTERS[sigma], md=md)
        assert md.counts() == full and md.strings() == strings
    finally:
        close_all(held)


# ---- 4. the literal cases through the chain --------------------------------------------------------------------------------------------
def test_planted_edits_and_exact_reads_of_many_lengths(work):
    name = "dna4_k10"
    sigma, k, n = WORKLOADS[name]
    idx, t = work.index(name), text_of(sigma, n)
    bump = lambda q, at, by=1: q.__setitem__(at, (q[at] + by) % sigma)
    xx = t[1000:1060].copy()
    bump(xx, 30), bump(xx, 31, 2)                              # two adjacent substitutions
    dx = np.delete(t[2000:2062], [30, 31])
    bump(dx, 30)                                               # a deletion that a substitution follows
    ins = np.insert(t[3000:3060], 30, [(t[3030] + 1) % sigma, (t[3029] + 2) % sigma])
    x0, x59 = t[4000:4060].copy(), t[5000:5060].copy()
    bump(x0, 0), bump(x59, 59)                                 # a substitution at the first letter, at the last
    exact = [t[10_000 + 2000 * i:10_000 + 2000 * i + m].copy() for i, m in enumerate((10, 100, 1000, 1024, 9, 99, 999))]
    reads = [xx, dx, ins, x0, x59] + exact
    ranks, roff = pack(reads)
    held = list(idx.map_reads(ranks, roff, k, band=8, min_votes=1, max_edits=8, scripts=True))
    try:
        loci, al, sc = held
        md = sc.md(idx, al, LETTERS[sigma])
        held.append(md)
        _, start, end, best, _ = al.host()
        strings = check_md(md, sc, start, end, t, sigma)
        check_rebuild(strings, sc, ranks, roff, start, end, t, sigma)
        read_sel_off = sc.host()[0]
        of = lambda r: strings[int(read_sel_off[r])] if read_sel_off[r + 1] > read_sel_off[r] else None
        assert of(0) == "30" + LETTERS[4][t[1030]] + "0" + LETTERS[4][t[1031]] + "28"
        assert re.search(r"\^[A-Z]+0[A-Z]", of(1)) and of(2) == "60"
        assert of(3) in ("0" + LETTERS[4][t[4000]] + "59", "59") and of(4) in ("59" + LETTERS[4][t[5059]] + "0", "59")
        assert [of(5 + i) for i in range(4)] == ["10", "100", "1000", "1024"] and [of(10), of(11)] == ["99", "999"]
        assert of(9) is None                                   # 9 letters: no window of 10
        assert md.counts()["n_mismatched"] == 0
    finally:
        close_all(held)


# ---- 5. foreign handles ----------------------------------------------------------------------------------------------------------------
def test_scripts_with_the_alignments_of_another_batch(work):
    name = "dna4_k10"
    sigma, k, n = WORKLOADS[name]
    idx, text = work.index(name), text_of(sigma, n)
    reads, loci, al, pl, pairs, sc = work.workload(name)
    ranks, roff = pairs_of(name)
    other = list(idx.map_pairs(ranks[int(roff[300]):int(roff[500])], roff[300:501] - roff[300], k, np.asarray(COMPLEMENT[sigma], np.uint8), **CHAIN, **INSERT))
    md = None
    try:
        al2 = other[2]
        assert 0 < al2.counts()["n_loci"] < al.counts()["n_loci"]
        md = sc.md(idx, al2, LETTERS[sigma])
        _, start, end = al2.host()[:3]
        check_md(md, sc, start, end, text, sigma)
        c = md.counts()
        assert c["n_sel"] == sc.counts()["n_sel"] and c["n_mismatched"] >= 100          # sel past n_loci, or lengths that do not fit
        # ... and the job arrays of a rescue in the place of the alignments
        res = pairs.rescue(idx, reads, loci, al, pl, **INSERT, max_edits=E)
        other.append(res)
        jobs = res.host()
        sc.md(idx, res, LETTERS[sigma], md=md)
        check_md(md, sc, jobs[5], jobs[6], text, sigma)
    finally:
        if md is not None:
            md.close()
        close_all(other)
        work.mapped.pop(name)                                  # the rescue has rewritten the placements: the next test maps anew
        close_all(list((reads, loci, al, pl, pairs, sc)))


# ---- 6. shapes and the letters table ---------------------------------------------------------------------------------------------------
def test_batches_of_every_size_through_one_md_handle_and_the_letters_refusals(work):
    name = "aa20_k5"
    sigma, k, n = WORKLOADS[name]
    engine, idx, text = work.engine, work.index(name), text_of(sigma, n)
    md = engine.Md()
    held = [md]
    try:
        for n_reads in (257, 0, 1, 3, 257):
            reads = [text[150 * i:150 * i + 40 + i % 7].copy() for i in range(n_reads)]
            for q in reads[::3]:
                q[20] = (q[20] + 1) % sigma
            ranks, roff = pack(reads) if reads else (np.zeros(0, np.uint8), np.zeros(1, np.uint64))
            loci, al, sc = idx.map_reads(ranks, roff, k, **CHAIN, scripts=True)
            held += [loci, al, sc]
            sc.md(idx, al, LETTERS[sigma], md=md)
            _, start, end = al.host()[:3]
            strings = check_md(md, sc, start, end, text, sigma)
            assert len(strings) == n_reads and md.counts()["n_mismatched"] == 0
            if n_reads == 0:
                assert md.host()[0].tolist() == [0] and md.device_ptrs()[1] is None and md.device_ptrs()[0]
            else:
                assert strings[0] == "20" + LETTERS[sigma][text[20]] + "19" and (n_reads < 2 or strings[1] == "41")
        # the letters table: refused before any handle is looked at, the md handle stays as it is
        full, L = (md.counts(), md.strings()), engine.lib()
        o = engine.MdOptions(8, 0)
        for at, byte in ((0, ord("7")), (sigma - 1, ord("^")), (5, 0), (3, ord("0")), (sigma - 1, ord("9"))):
            table = np.frombuffer(LETTERS[sigma].encode(), np.uint8).copy()
            table[at] = byte
            assert L.kmx_scripts_md(idx._h, sc._h, al._h, table.ctypes.data, C.byref(o), None, C.byref(md._h)) == 1
            assert b"letters" in L.kmx_last_error()
            with pytest.raises(engine.KmxError):
                sc.md(idx, al, table)
        assert L.kmx_scripts_md(idx._h, sc._h, al._h, None, C.byref(o), None, C.byref(md._h)) == 1 and b"letters" in L.kmx_last_error()
        assert (md.counts(), md.strings()) == full
        # entries past sigma are not looked at, duplicates are allowed
        table = np.frombuffer((LETTERS[sigma] + "^0").encode(), np.uint8).copy()
        table[1] = table[0]
        sc.md(idx, al, table, md=md)
        assert md.counts() == full[0]
    finally:
        close_all(held)


# ---- 7. MAPQ ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(WORKLOADS))
def test_mapq_of_single_reads_pairs_and_rescued_pairs(work, name):
    sigma, k, _ = WORKLOADS[name]
    idx, comp = work.index(name), np.asarray(COMPLEMENT[sigma], np.uint8)
    ranks, roff = rescue_pairs_of(name)
    held = list(idx.map_pairs(ranks, roff, k, comp, **CHAIN, **INSERT))
    try:
        reads, loci, al, pl, pairs = held
        mq = pl.mapq(E, pairs)
        held.append(mq)
        before = check_mapq(mq, pl, E, pairs)
        assert mq.counts()["n_cap"] >= 250 and mq.counts()["nr"] == 2 * N_PAIRS
        check_mapq(pl.mapq(E, mapq=mq), pl, E)                                   # the same placements as single reads
        res = pairs.rescue(idx, reads, loci, al, pl, **INSERT, max_edits=E)
        held.append(res)
        after = check_mapq(pl.mapq(E, pairs, mapq=mq), pl, E, pairs)
        taken = res.host()[1][res.host()[7] == 3] // 2                           # the rescued public reads
        assert taken.size == 75 and (before[taken] == 0).all() and (after[taken] > 0).all()
        # the strand fold of the same alignments
        pl2 = al.fold_strands(loci)
        held.append(pl2)
        check_mapq(pl2.mapq(E, mapq=mq), pl2, E)
        # the corners of the options
        for opts in (dict(cap=0), dict(cap=254, per_edit=100, pair_bonus=1000), dict(per_edit=0), dict(pair_bonus=0), dict(pair_bonus=0xFFFFFFFF),
                     dict(cap=254, per_edit=0xFFFFFFFF, pair_bonus=0xFFFFFFFF), dict(cap=30)):
            check_mapq(pl.mapq(E, pairs, mapq=mq, **opts), pl, E, pairs, **opts)
        for budget in (0, 3, 250):
            check_mapq(pl.mapq(budget, pairs, mapq=mq), pl, budget, pairs)
    finally:
        close_all(held)


def test_mapq_of_the_repeat_mate_and_of_the_reverse_palindrome(engine):
    text, _ = repeat_text()
    idx = engine.Index(text, 4, [10], table=2)
    held = []
    try:
        held += list(idx.map_pairs(*repeat_pair(), 10, np.asarray(COMPLEMENT[4], np.uint8), **REPEAT_CHAIN, min_insert=450, max_insert=520))
        pl, pairs = held[3], held[4]
        assert pl.host()[5].tolist() == [0, 255] and pairs.host()[0].tolist() == [pn.CONCORDANT]
        mq = pl.mapq(E, pairs)
        held.append(mq)
        assert check_mapq(mq, pl, E, pairs).tolist() == [40, 60] and mq.counts() == dict(nr=2, n_zero=0, n_cap=1)
        assert check_mapq(pl.mapq(E, pairs, cap=30, mapq=mq), pl, E, pairs, cap=30).tolist() == [30, 30]
        assert check_mapq(pl.mapq(E, pairs, pair_bonus=7, mapq=mq), pl, E, pairs, pair_bonus=7).tolist() == [7, 60]
        assert check_mapq(pl.mapq(E, mapq=mq), pl, E).tolist() == [0, 60]                  # alone it stays a repeat read
        # x + rc(x) equals its reverse complement: the other strand is a copy elsewhere
        n = text.size
        out = idx.map_reads_strands(*pack([text[n - 40:].copy(), text[500:560].copy()]), 10, np.asarray(COMPLEMENT[4], np.uint8), **REPEAT_CHAIN)
        held += list(out)
        assert out[3].host()[2].tolist() == [0, 0] and out[3].host()[5].tolist() == [0, 255]
        assert check_mapq(out[3].mapq(E, mapq=mq), out[3], E).tolist() == [0, 60] and mq.counts() == dict(nr=2, n_zero=1, n_cap=1)
    finally:
        close_all(held)
        idx.close()


def test_mapq_batches_of_every_size_and_every_refusal(work):
    name = "dna4_k10"
    sigma, k, _ = WORKLOADS[name]
    engine, idx, comp = work.engine, work.index(name), np.asarray(COMPLEMENT[sigma], np.uint8)
    ranks, roff = pairs_of(name)
    L = engine.lib()
    mq = engine.Mapq()
    held = [mq]
    try:
        for n_reads in (257, 0, 1, 3):
            sub = roff[:n_reads + 1]
            out = idx.map_reads_strands(ranks[:int(sub[-1])], sub, k, comp, **CHAIN)
            held += list(out)
            check_mapq(out[3].mapq(E, mapq=mq), out[3], E)
            assert mq.counts()["nr"] == n_reads
            if n_reads == 0:
                assert mq.device_ptrs() == (None,) and mq.host().size == 0
                p = C.c_void_p(1)
                assert L.kmx_mapq_view(mq._h, C.byref(p)) == 0 and not p.value
        reads, loci, al, pl, pairs, _ = work.workload(name)
        check_mapq(pl.mapq(E, pairs, mapq=mq), pl, E, pairs)
        full = (mq.counts(), mq.host().tobytes(), mq.device_ptrs())
        size = C.sizeof(engine.MapqOptions)
        opt = lambda **kw: engine.MapqOptions(**dict(dict(struct_size=size, max_edits=E, cap=60, per_edit=10, pair_bonus=40, flags=0), **kw))
        call = lambda o, pl_=pl, pr=pairs, out_=mq: L.kmx_placements_mapq(pl_ and pl_._h, pr and pr._h, o and C.byref(o), None, out_ and C.byref(out_._h))
        # before any handle is looked at: the handle stays as it is
        for o, word in ((opt(struct_size=size - 1), "struct_size"), (opt(flags=1), "flags"), (opt(max_edits=251), "max_edits"), (opt(cap=255), "cap")):
            assert call(o) == 1 and word.encode() in L.kmx_last_error(), word
        assert call(opt(), pl_=None) == 1 and call(None) == 1 and call(opt(), out_=None) == 1
        assert (mq.counts(), mq.host().tobytes(), mq.device_ptrs()) == full
        # after looking: pairs that are not those of the placements; the handle then holds an empty result
        assert call(opt(), pl_=held[4]) == 1 and b"np" in L.kmx_last_error()        # the placements of 257 single reads
        assert mq.counts() == dict(nr=0, n_zero=0, n_cap=0) and mq.device_ptrs() == (None,) and mq.host().size == 0
        with pytest.raises(engine.KmxError):
            held[4].mapq(E, pairs, mapq=mq)
        # ... and it serves again; a handle allocated by the call
        check_mapq(pl.mapq(E, pairs, mapq=mq), pl, E, pairs)
        assert (mq.counts(), mq.host().tobytes()) == full[:2]
        mq2 = pl.mapq(E, pairs, cap=254)
        held.append(mq2)
        check_mapq(mq2, pl, E, pairs, cap=254)
    finally:
        close_all(held)


# ---- 8. the tags of the chains ---------------------------------------------------------------------------------------------------------
def test_map_pairs_and_map_reads_strands_with_tags_are_the_calls_they_are_made_of(work):
    name = "dna4_k10"
    sigma, k, n = WORKLOADS[name]
    engine, idx, comp, text = work.engine, work.index(name), np.asarray(COMPLEMENT[sigma], np.uint8), text_of(sigma, n)
    ranks, roff = rescue_pairs_of(name)
    held = []
    try:
        out = idx.map_pairs(ranks, roff, k, comp, **CHAIN, **INSERT, rescue=True, tags=True, letters=LETTERS[sigma])
        held += list(out)
        assert len(out) == 8 and isinstance(out[5], engine.Scripts) and isinstance(out[6], engine.Rescues) and isinstance(out[7], engine.SamTags)
        reads, loci, al, pl, pairs, sc, res, tags = out
        assert isinstance(tags.mapq, engine.Mapq) and isinstance(tags.md, engine.Md) and isinstance(tags.rescue_scripts, engine.Scripts)
        assert isinstance(tags.rescue_md, engine.Md)
        check_mapq(tags.mapq, pl, E, pairs)
        _, start, end = al.host()[:3]
        check_md(tags.md, sc, start, end, text, sigma)
        jobs = res.host()
        check_md(tags.rescue_md, tags.rescue_scripts, jobs[5], jobs[6], text, sigma)
        assert tags.rescue_md.counts()["n_sel"] == res.counts()["n_taken"] == 75
        # without tags: what it returns today
        plain = idx.map_pairs(ranks, roff, k, comp, **CHAIN, **INSERT, rescue=True, scripts=True)
        held += list(plain)
        assert len(plain) == 7
        same(PLACEMENTS, plain[3].host(), pl.host())
        same(PAIRS, plain[4].host(), pairs.host())
        same(SCRIPTS, plain[5].host(), sc.host())
        same(JOBS, plain[6].host(), res.host())
        bare = idx.map_pairs(ranks, roff, k, comp, **CHAIN, **INSERT)
        held += list(bare)
        assert len(bare) == 5
        no_rescue = idx.map_pairs(ranks, roff, k, comp, **CHAIN, **INSERT, tags=True, letters=LETTERS[sigma])
        held += list(no_rescue)
        assert len(no_rescue) == 7 and no_rescue[6].rescue_scripts is None and no_rescue[6].rescue_md is None
        check_mapq(no_rescue[6].mapq, no_rescue[3], E, no_rescue[4])
        same(PLACEMENTS, bare[3].host(), no_rescue[3].host())
        # both strands of single reads
        single = idx.map_reads_strands(ranks, roff, k, comp, **CHAIN, tags=True, letters=LETTERS[sigma])
        held += list(single)
        assert len(single) == 6 and single[5].rescue_scripts is None and single[5].rescue_md is None
        check_mapq(single[5].mapq, single[3], E)
        check_md(single[5].md, single[4], *single[2].host()[1:3], text, sigma)
        old = idx.map_reads_strands(ranks, roff, k, comp, **CHAIN, scripts=True)
        held += list(old)
        assert len(old) == 5
        same(PLACEMENTS, old[3].host(), single[3].host())
        same(SCRIPTS, old[4].host(), single[4].host())
        older = idx.map_reads_strands(ranks, roff, k, comp, **CHAIN)
        held += list(older)
        assert len(older) == 4
        with pytest.raises(ValueError):
            idx.map_pairs(ranks, roff, k, comp, **CHAIN, **INSERT, tags=True)
        with pytest.raises(ValueError):
            idx.map_reads_strands(ranks, roff, k, comp, **CHAIN, tags=True)
    finally:
        close_all(held)


# ---- 9. SAM lines ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("paired", (True, False))
def test_sam_lines_of_the_device_results_rebuild_the_text(work, paired):
    name = "dna4_k10"
    sigma, k, n = WORKLOADS[name]
    engine, idx, comp, text = work.engine, work.index(name), np.asarray(COMPLEMENT[sigma], np.uint8), text_of(sigma, n)
    ranks, roff = rescue_pairs_of(name)
    if paired:
        out = idx.map_pairs(ranks, roff, k, comp, **CHAIN, **INSERT, rescue=True, tags=True, letters=LETTERS[sigma])
        reads, loci, al, pl, pairs, sc, res, tags = out
        cigars, mds = (pl.cigars(sc), res.cigars(tags.rescue_scripts)), (pl.mds(tags.md, sc), res.mds(tags.rescue_md, tags.rescue_scripts))
        assert sum(bool(a) and bool(b) for a, b in zip(*cigars)) == 0 and sum(bool(b) for b in cigars[1]) == 75
    else:
        out = idx.map_reads_strands(ranks, roff, k, comp, **CHAIN, tags=True, letters=LETTERS[sigma])
        reads, loci, al, pl, sc, tags = out
        pairs, cigars, mds = None, pl.cigars(sc), pl.mds(tags.md, sc)
    try:
        names = [f"q{i}" for i in range(roff.size - 1)]
        placements = pl.host(best2=False)
        lines = engine.sam_lines(names, ranks, roff, LETTERS[sigma], comp, sigma, "ref", placements, cigars, mds, tags.mapq.host(),
                                 pairs.host() if paired else None)
        assert len(lines) == roff.size - 1
        strand, dist, start, end = placements[1], placements[2], placements[3], placements[4]
        raw = spell(text, sigma)
        n_placed = n_reverse = 0
        for i, line in enumerate(lines):
            f = line.split("\t")
            if strand[i] == 255:
                assert len(f) == 11 and f[5] == "*" and int(f[1]) & 0x4 and f[4] == "0"
                continue
            n_placed += 1
            n_reverse += int(strand[i])
            assert len(f) == 13 and f[0] == names[i] and f[2] == "ref" and f[10] == "*" and f[11] == f"NM:i:{dist[i]}" and f[12].startswith("MD:Z:")
            assert bool(int(f[1]) & 0x10) == bool(strand[i]) and not int(f[1]) & 0x4 and bool(int(f[1]) & 0x1) == paired
            runs = [(int(a) << 4) | engine.CIGAR_OPS.index(b) for a, b in re.findall(r"([0-9]+)([MIDNSHP=X])", f[5])]
            ref = mn.rebuild(f[9], runs, f[12][5:])            # from the line alone
            pos = int(f[3])
            assert pos == int(start[i]) + 1 and ref == raw[pos - 1:pos - 1 + len(ref)] and len(ref) == int(end[i]) - int(start[i])
            assert sum(int(v) >> 4 for v in runs if (v & 15) != mn.OP_EQ) == int(dist[i])
        assert n_placed == pl.counts()["n_placed"] >= 350 and n_reverse >= 100
    finally:
        close_all(list(out))
