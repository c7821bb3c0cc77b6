"""Secondary placements on the GPU: kmx_placements_secondaries, kmx_secondaries_scripts, kmx_secondaries_md, Secondaries.xa and the
`secondaries=` keyword of the chain calls.  The oracle is always tests/secondary_naive.py on the host views of the engine's own loci,
alignments and placements; the scripts and MD strings of the entries go against tests/script_naive.py and tests/md_naive.py.  No
shape is larger than those of tests/test_strands_map_gpu.py and tests/test_pairs_gpu.py, whose workloads (tests/chain_data.py) are reused."""
import ctypes as C
import re

import numpy as np
import pytest

from kmer_index_amd import synth
from tests import align_naive as an
from tests import fold_naive as fn
from tests import script_naive as scn
from tests import secondary_naive as sn
from tests import vote_naive as vn
from tests import windows_naive as wn
from tests.chain_checks import MappedStrands, StrandWork, check_md, check_rebuild, close_all, dev_array, read_of_entries, refused, same
from tests.chain_data import (ALIGN, CHAIN, COMP4, COMPLEMENT, FOLD, INSERT, LOCI, N_READS, PAIR_SIZES, PAIR_WORKLOADS, PLANT_AT, REPEAT_CHAIN,
                              RESCUE_FLOORS, SCRIPTS, STRAND_FLOORS, kill, pair_text, pairs_of, planted_text, rc4, repeat_text, rescue_pairs_of,
                              table_of, text_of)
from tests.helpers import pack

pytestmark = pytest.mark.gpu

SEC = ("sec_off", "locus", "dist", "start", "end", "more")
NO = sn.NO_BEST


def naive_chain(text, ranks, roff, sigma, complement, k, band, min_votes, max_edits, max_span=0xFFFFFFFF):
    """The whole single-read chain on the CPU: a dictionary of the text's k-mers, vote_naive.vote, align_naive.align on
    fold_naive.double_reads, fold_naive.fold.  Returns (locus_off, dist, start, end, the fold's tuple).  How the expectations and the
    floors of this file were confirmed; not run by the tests (up to a minute per workload)."""
    ranks2, roff2 = fn.double_reads(ranks, roff, complement, sigma)
    raw, where = np.asarray(text, np.uint8).tobytes(), {}
    for i in range(len(raw) - k + 1):
        where.setdefault(raw[i:i + k], []).append(i)
    qranks, qoff, win_off = wn.expand(ranks2, roff2, k, 1)
    qraw = qranks.tobytes()
    hits = [where.get(qraw[int(a):int(b)], []) if max(qraw[int(a):int(b)], default=0) < sigma else [] for a, b in zip(qoff[:-1], qoff[1:])]
    hit_off = np.zeros(len(hits) + 1, np.uint64)
    hit_off[1:] = np.cumsum([len(h) for h in hits])
    positions = np.asarray([x for h in hits for x in h], np.uint32)
    locus_off, diag, span = vn.vote(hit_off, positions, win_off, 1, band, min_votes, 0)[:3]
    dist, start, end, best, _ = an.align(np.asarray(text), ranks2, roff2, locus_off, diag, span, max_edits, max_span, sigma)
    return locus_off, dist, start, end, fn.fold(locus_off, dist, start, end, best)


def check(sec, h_loci, h_al, pl, N, delta=None, ctg=None):
    """The secondaries handle against the oracle on these host loci, alignments and the placements as they are now; the device views
    against the host views.  Returns the oracle's result by name."""
    want = sn.secondaries(h_loci[0], h_al[0], h_al[1], h_al[2], pl.host(best2=False), N, delta)
    got = sec.host()
    same(SEC, got[:5] + (got[6],), want[:6])
    c = sec.counts()
    nr = (h_loci[0].size - 1) // 2
    assert (c["nr"], c["n_sec"], c["n_multi"], c["n_truncated"]) == (nr,) + want[6:]
    dv = sec.device_ptrs()
    if ctg is None:
        assert got[5] is None and dv[5] is None               # no contig table: no view
    else:
        assert got[5].dtype == np.uint32 and np.array_equal(got[5], ctg[got[1]])
        assert np.array_equal(dev_array(dv[5], c["n_sec"], np.uint32), got[5])
    sizes = (2 * nr + 1, c["n_sec"], c["n_sec"], c["n_sec"], c["n_sec"], None, nr)
    for name, p, n, g in zip(SEC[:5] + ("ctg", "more"), dv, sizes, got):
        if name != "ctg":
            assert (p is None) == (n == 0), name
            assert np.array_equal(dev_array(p, n, g.dtype), g), name
    return dict(zip(sn.NAMES, want))


def entries_of(out, i):
    """(strand, start, dist) of the entries of public read i"""
    a, b, c = (int(out["sec_off"][2 * i + k]) for k in range(3))
    return [(0 if e < b else 1, int(out["start"][e]), int(out["dist"][e])) for e in range(a, c)]


# ---- 1. the tandem repeat ---------------------------------------------------------------------------------------------------------------
def repeat_reads():
    text, unit = repeat_text()
    two, three = np.concatenate([unit, unit]), np.concatenate([unit, unit, unit])
    return [two, rc4(two), text[11000:11040].copy(), text[8970:9040].copy(), text[300:380].copy(), unit.copy(), three[:120].copy()]


# per read: loci on both strands, the primary (strand, start), and for N = 32 without a delta the number of entries, their strand,
# the first start, the step between starts, `more`.  Computed with naive_chain and secondary_naive on the CPU.
REPEAT_TABLE = (
    (141, (0, 2000), 32, 0, 2100, 100, 1),    # two units: every other copy
    (141, (1, 2000), 32, 1, 2100, 100, 1),    # its reverse complement: the same on strand 1
    (2, (0, 11000), 1, 1, 11000, 0, 0),       # the palindrome: its twin on the other strand
    (140, (0, 8970), 0, 0, 0, 0, 0),          # only the last of 140 loci aligns
    (1, (0, 300), 0, 0, 0, 0, 0),
    (140, (0, 2000), 32, 0, 2050, 50, 1),     # one unit: every copy
    (142, (0, 2000), 32, 0, 2150, 150, 1),    # 120 letters of three units: every third copy
)


@pytest.fixture(scope="module")
def repeat_index(engine):
    idx = engine.Index(repeat_text()[0], 4, [10], table=2)
    yield idx
    idx.close()


@pytest.fixture(scope="module")
def repeat_mapped(repeat_index):
    mp = MappedStrands(repeat_index, 4, *pack(repeat_reads()), 10, **REPEAT_CHAIN)
    yield mp
    mp.close()


def test_tandem_repeat_palindrome_and_one_sided_reads(repeat_mapped):
    mp = repeat_mapped
    n_loci = np.diff(mp.h_loci[0].astype(np.int64))
    pl = mp.pl.host()
    sec = None
    try:
        for N in (32, 3):
            sec = mp.pl.secondaries(mp.loci, mp.al, N, secondaries=sec)
            out = check(sec, mp.h_loci, mp.h_al, mp.pl, N)
            for i, (nl, (ps, p0), cnt, s, first, step, more) in enumerate(REPEAT_TABLE):
                assert int(n_loci[2 * i] + n_loci[2 * i + 1]) == nl and (int(pl[1][i]), int(pl[2][i]), int(pl[3][i])) == (ps, 0, p0), i
                want = [(s, first + j * step, 0) for j in range(min(cnt, N))]
                assert entries_of(out, i) == want and int(out["more"][i]) == (more if cnt >= N else 0), (N, i)
            assert max(n_loci) > 128                            # several strides of the wave, and 32 rounds
            assert (out["n_multi"], out["n_truncated"]) == (5, 4)
    finally:
        close_all([sec])


# ---- 2. planted copies ------------------------------------------------------------------------------------------------------------------
def planted_reads():
    text, seg = planted_text()
    return [seg.copy(), rc4(seg), text[PLANT_AT[1] - 40:PLANT_AT[1] + 60].copy()]


@pytest.fixture(scope="module")
def planted(engine):
    idx = engine.Index(planted_text()[0], 4, [10], table=2)
    mp = MappedStrands(idx, 4, *pack(planted_reads()), 10, **REPEAT_CHAIN)
    yield mp
    mp.close()
    idx.close()


def test_planted_copies_by_n_and_max_delta(planted):
    mp = planted
    a, b, c1, c3, r = PLANT_AT
    pl = mp.pl.host()
    # the reverse complement of the segment reads forward at the reverse-complemented copy: the forward strand wins the tie
    assert [(int(pl[1][i]), int(pl[2][i]), int(pl[3][i])) for i in range(3)] == [(0, 0, a), (0, 0, r), (0, 0, b - 40)]
    sec = None
    try:
        # (N, max_delta) -> the entries of the segment read and of its reverse complement, and `more` of both
        for (N, delta), want, want_rc, more in (
                ((32, None), [(0, b, 0), (0, c1, 1), (0, c3, 3), (1, r, 0)], [(1, a, 0), (1, b, 0), (1, c1, 1), (1, c3, 3)], 0),
                ((2, None), [(0, b, 0), (1, r, 0)], [(1, a, 0), (1, b, 0)], 1),
                ((32, 0), [(0, b, 0), (1, r, 0)], [(1, a, 0), (1, b, 0)], 0),
                ((32, 1), [(0, b, 0), (0, c1, 1), (1, r, 0)], [(1, a, 0), (1, b, 0), (1, c1, 1)], 0)):
            sec = mp.pl.secondaries(mp.loci, mp.al, N, delta, secondaries=sec)
            out = check(sec, mp.h_loci, mp.h_al, mp.pl, N, delta)
            assert entries_of(out, 0) == want and int(out["more"][0]) == more, (N, delta)
            assert entries_of(out, 1) == want_rc and int(out["more"][1]) == more, (N, delta)
            assert entries_of(out, 2) == [] and int(out["more"][2]) == 0       # 40 foreign letters: no other copy within 8 edits
    finally:
        close_all([sec])


# ---- 3. the ordinary workloads ----------------------------------------------------------------------------------------------------------
# (workload, band) -> the reads with at least one entry at N = 4 without a delta, at least: the placed reads whose `second` is not
# 255, from naive_chain on the CPU (never from the engine).  The reads are cut from random texts, so a second place is rare: two reads
# of the dna4 workload have one (3 entries in all), none of the 20-letter one.
MULTI_FLOORS = {("dna4_k10", 8): 2, ("aa20_k5", 8): 0, ("dna4_k10", 0): 2}


@pytest.fixture(scope="module")
def work(engine):
    w = StrandWork(engine)
    yield w
    w.close()


@pytest.mark.parametrize("name,band", sorted(MULTI_FLOORS))
def test_workloads_equal_the_oracle_and_leave_the_inputs_alone(work, name, band):
    mp = work.workload(name, band)
    before = (mp.loci.device_ptrs(), mp.al.device_ptrs(), mp.pl.device_ptrs(), mp.loci.counts(), mp.al.counts(), mp.pl.counts())
    pl_before = mp.pl.host()
    sec = mp.pl.secondaries(mp.loci, mp.al, 4)
    try:
        out = check(sec, mp.h_loci, mp.h_al, mp.pl, 4)
        strand, second = pl_before[1], pl_before[5]
        has = np.diff(out["sec_off"].astype(np.int64)[::2]) > 0
        assert np.array_equal(has, (strand != 255) & (second != 255))             # an entry exactly where the fold saw a runner-up
        assert out["n_multi"] == int(has.sum()) >= MULTI_FLOORS[(name, band)]
        aligned2 = np.add.reduceat(np.append(mp.h_al[4], 0).astype(np.int64), np.arange(0, 2 * N_READS, 2))
        shadows = (strand != 255) & (aligned2 >= 2) & (second == 255)             # two or more loci, one place
        assert int(shadows.sum()) >= STRAND_FLOORS[(name, band)][3] and not has[shadows].any()
        # the inputs are what they were
        assert before == (mp.loci.device_ptrs(), mp.al.device_ptrs(), mp.pl.device_ptrs(), mp.loci.counts(), mp.al.counts(), mp.pl.counts())
        same(LOCI, mp.loci.host(), mp.h_loci)
        same(ALIGN, mp.al.host(), mp.h_al)
        same(FOLD, mp.pl.host(), pl_before)
    finally:
        sec.close()


# ---- 4. paired reads --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,rescue", [("dna4_k10", False), ("aa20_k5", False), ("dna4_k10", True)])
def test_paired_reads_before_and_after_a_rescue(engine, name, rescue):
    sigma, k, n = PAIR_WORKLOADS[name]
    ranks, roff = rescue_pairs_of(name) if rescue else pairs_of(name)
    idx = engine.Index(text_of(sigma, n), sigma, [k], table=2)
    held = []
    try:
        held += list(idx.map_pairs(ranks, roff, k, np.asarray(COMPLEMENT[sigma], np.uint8), **CHAIN, **INSERT, rescue=rescue))
        loci, al, pl = held[1:4]
        sec = pl.secondaries(loci, al, 4)
        held.append(sec)
        out = check(sec, loci.host(), al.host(), pl, 4)        # the oracle runs on the final placements
        p_locus, p_strand, _, p_start, p_end = pl.host(best2=False)[:5]
        rescued = np.flatnonzero((p_strand != 255) & (p_locus == NO))
        assert rescued.size == (RESCUE_FLOORS[name] if rescue else 0) == (held[5].counts()["n_taken"] if rescue else 0)
        for i in rescued:                                      # never its own interval
            s = int(p_strand[i])
            for e in range(int(out["sec_off"][2 * i + s]), int(out["sec_off"][2 * i + s + 1])):
                assert max(int(out["start"][e]), int(p_start[i])) >= min(int(out["end"][e]), int(p_end[i])), (i, e)
        assert out["n_sec"] == sec.counts()["n_sec"]
    finally:
        close_all(held)
        idx.close()


def test_a_repeat_mate_that_followed_its_partner_lists_the_leftmost_copy(repeat_index):
    text, _ = repeat_text()
    mates = pack([text[8800:8900].copy(), rc4(text[9200:9300])])
    held = []
    try:
        held += list(repeat_index.map_pairs(*mates, 10, COMP4, **REPEAT_CHAIN, min_insert=450, max_insert=520))
        loci, al, pl = held[1:4]
        assert pl.host()[3].tolist() == [8800, 9200]           # mate 1 sits next to its unique partner, not at the leftmost copy
        sec = pl.secondaries(loci, al, 32)
        held.append(sec)
        out = check(sec, loci.host(), al.host(), pl, 32)
        ents = entries_of(out, 0)
        assert ents[0] == (0, 2000, 0) and len(ents) == 32 and int(out["more"][0]) == 1 and all(x != 8800 for _, x, _ in ents)
        assert entries_of(out, 1) == []
    finally:
        close_all(held)


# ---- 5. contigs -------------------------------------------------------------------------------------------------------------------------
def test_entries_carry_their_contig_and_xa_is_contig_local(engine):
    text, ctg_off = pair_text(), table_of(PAIR_SIZES)
    off = ctg_off.astype(np.int64)
    names = [f"ctg{c}" for c in range(len(PAIR_SIZES))]
    assert len(names) <= 40 and np.array_equal(text[off[12]:off[13]], text[off[13]:off[14]])
    reads = [text[int(off[12]) + 5 + 30 * i:int(off[12]) + 95 + 30 * i].copy() for i in range(6)]           # from the contig that stands twice
    reads += [rc4(reads[1]), text[int(off[3]) + 100:int(off[3]) + 200].copy(), rc4(text[int(off[20]) + 7:int(off[20]) + 99])]
    ranks, roff = pack(reads)
    idx = engine.Index(text, 4, [10], table=2)
    held = []
    try:
        idx.set_contigs(ctg_off)
        held += list(idx.map_reads_strands(ranks, roff, 10, COMP4, **CHAIN))
        rd, loci, al, pl = held
        ctg = al.contigs_host()
        sec = pl.secondaries(loci, al, 4)
        held.append(sec)
        out = check(sec, loci.host(), al.host(), pl, 4, ctg=ctg)
        e_ctg = sec.host()[5]
        p_locus, p_strand = pl.host()[:2]
        for i in range(7):                                     # the primary in one copy, the twin contig's copy an entry
            assert ctg[p_locus[i]] == 12 and p_strand[i] == (1 if i == 6 else 0)
            e0, e2 = int(out["sec_off"][2 * i]), int(out["sec_off"][2 * i + 2])
            assert e_ctg[e0:e2].tolist() == [13] and int(out["start"][e0]) - int(off[13]) == int(pl.host()[3][i]) - int(off[12])
        assert entries_of(out, 7) == [] and entries_of(out, 8) == []
        sc = sec.scripts(idx, rd)
        held.append(sc)
        xa = sec.xa(sc, located=(names, ctg_off))
        contigs = {nm: text[int(a):int(b)] for nm, a, b in zip(names, off[:-1], off[1:])}
        for i, s in enumerate(xa):
            assert bool(s) == (i < 7)
            for item in s.split(";")[:-1]:
                nm, pos, cigar, nm_i = item.split(",")
                assert nm == "ctg13" and pos[0] == ("-" if i == 6 else "+") and cigar == "90=" and nm_i == "0"
                q = reads[i] if pos[0] == "+" else rc4(reads[i])
                at = int(pos[1:]) - 1                          # contig-local, 0-based
                assert np.array_equal(contigs[nm][at:at + 90], q) and at == 5 + 30 * (1 if i == 6 else i)
        with pytest.raises(ValueError):
            sec.xa(sc)                                         # neither rname nor located
        # without a table the handle has no ctg, and located is refused
        idx.set_contigs(None)
        held += list(idx.map_reads_strands(ranks, roff, 10, COMP4, **CHAIN, secondaries=4))
        sec2 = held[-1]
        check(sec2, held[-4].host(), held[-3].host(), held[-2], 4)
        with pytest.raises(ValueError):
            sec2.xa(sc, located=(names, ctg_off))
        assert [s.replace("chr,", "") for s in sec2.xa(sc, rname="chr")[:1]] == [f"+{int(off[13]) + 6},90=,0;"]
    finally:
        close_all(held)
        idx.close()


# ---- 6. scripts and MD of the entries ---------------------------------------------------------------------------------------------------
def check_scripts_and_md(engine, idx, mp, text, sigma, sec, letters):
    """the scripts and MD strings of every entry of sec against the naive modules; returns (Scripts, Md, strings) for the caller to close"""
    sec_off, locus, dist, start, end, _, _ = sec.host()
    ranks2, roff2 = fn.double_reads(mp.ranks, mp.roff, COMPLEMENT[sigma], sigma)
    sc = sec.scripts(idx, mp.reads)
    md = None
    try:
        want = scn.scripts(text, ranks2, roff2, sec_off, dist, start, end, None, sigma, True, False)
        got = sc.host()
        same(SCRIPTS, got, want[:4])
        c = sc.counts()
        assert (c["nr"], c["n_sel"], c["n_mismatched"]) == (sec_off.size - 1, locus.size, 0) and want[4] == 0
        assert np.array_equal(got[1], np.arange(locus.size, dtype=np.uint32)) and np.array_equal(got[0], sec_off)      # sel[e] == e
        for e, r in enumerate(read_of_entries(got[0])):     # every script replays: the read, or its reverse complement, against the text
            runs = got[3][int(got[2][e]):int(got[2][e + 1])]
            q = ranks2[int(roff2[r]):int(roff2[r + 1])]
            assert scn.replay(q, text[int(start[e]):int(end[e])], runs, sigma) == (int(dist[e]), True), e
            assert sum(int(v) >> 4 for v in runs if engine.CIGAR_OPS[int(v) & 15] in "XID") == int(dist[e]), e
        assert sec.cigars(sc) == scn.strings(want[2], want[3])
        md = sec.md(idx, sc, letters)
        strings = check_md(md, sc, start, end, text, sigma, bound=locus.size)
        assert md.counts()["n_mismatched"] == 0 and len(strings) == locus.size
        check_rebuild(strings, sc, ranks2, roff2, start, end, text, sigma)
        return sc, md, strings
    except Exception:
        close_all([md, sc])
        raise


def test_scripts_and_md_of_the_planted_copies_and_the_script_flags(engine, planted):
    mp = planted
    text, _ = planted_text()
    idx = mp.idx
    sec = mp.pl.secondaries(mp.loci, mp.al, 32)
    held = [sec]
    try:
        sc, md, strings = check_scripts_and_md(engine, idx, mp, text, 4, sec, "ACGT")
        held += [sc, md]
        assert sorted(sec.cigars(sc)[:4]) == sorted(["120=", "120=", "60=1X59=", "25=1X34=1X34=1X24="])
        assert sorted(strings[:4], key=len)[:2] == ["120", "120"] and sum(len(re.findall("[ACGT]", s)) for s in strings[:4]) == 4
        # scratch_bytes changes nothing; KMX_SCRIPT_M joins '=' and 'X'; KMX_SCRIPT_ALL is refused and leaves the result in place
        sec_off, _, dist, start, end, _, _ = sec.host()
        ranks2, roff2 = fn.double_reads(mp.ranks, mp.roff, COMPLEMENT[4], 4)
        want = scn.scripts(text, ranks2, roff2, sec_off, dist, start, end, None, 4, True, False)
        same(SCRIPTS, sec.scripts(idx, mp.reads, scratch_bytes=1, scripts=sc).host(), want[:4])
        o = engine.ScriptOptions(C.sizeof(engine.ScriptOptions), engine.SCRIPT_ALL, 0)
        assert engine.lib().kmx_secondaries_scripts(idx._h, mp.reads._h, sec._h, C.byref(o), C.byref(sc._h)) == 1
        assert b"kmx_secondaries_scripts" in engine.lib().kmx_last_error() and b"KMX_SCRIPT_ALL" in engine.lib().kmx_last_error()
        same(SCRIPTS, sc.host(), want[:4])
        want_m = scn.scripts(text, ranks2, roff2, sec_off, dist, start, end, None, 4, True, True)
        same(SCRIPTS, sec.scripts(idx, mp.reads, m=True, scripts=sc).host(), want_m[:4])
        assert "120M" in sec.cigars(sc) and not any("X" in s for s in sec.cigars(sc))
        with pytest.raises(engine.KmxError) as e:              # an MD needs '=' and 'X' apart
            sec.md(idx, sc, "ACGT", md=md)
        assert "kmx_secondaries_md" in str(e.value) and "KMX_SCRIPT_M" in str(e.value)
        # the reads of another batch are refused
        other = idx.strand_reads(*pack([planted_text()[1].copy()]), COMP4)
        held.append(other)
        with pytest.raises(engine.KmxError) as e:
            sec.scripts(idx, other, scripts=sc)
        assert "kmx_secondaries_scripts" in str(e.value) and "nr2 differs" in str(e.value)
    finally:
        close_all(held)


def test_scripts_and_md_of_copies_with_a_deletion_and_an_insertion(engine):
    seg = synth.ranks(822, 120, 4)
    t = synth.ranks(821, 4000, 4).copy()
    t[300:420] = seg
    t[1300:1419] = np.delete(seg, 50)                          # the read has a letter more: an insertion
    extra = np.insert(seg, 70, (seg[70] + 1) % 4)
    extra[20] = (extra[20] + 2) % 4
    t[2300:2421] = extra                                       # the read has a letter less and a substitution
    t[3300:3419] = rc4(np.delete(seg, 90))
    idx = engine.Index(t, 4, [10], table=2)
    mp = MappedStrands(idx, 4, *pack([seg.copy(), rc4(seg)]), 10, **REPEAT_CHAIN)
    held = []
    try:
        sec = mp.pl.secondaries(mp.loci, mp.al, 32)
        held.append(sec)
        out = check(sec, mp.h_loci, mp.h_al, mp.pl, 32)
        assert [(s, x, d) for s, x, d in entries_of(out, 0)] == [(0, 1300, 1), (0, 2300, 2), (1, 3300, 1)]
        assert [(s, x, d) for s, x, d in entries_of(out, 1)] == [(0, 3300, 1), (1, 1300, 1), (1, 2300, 2)]
        sc, md, strings = check_scripts_and_md(engine, idx, mp, t, 4, sec, "ACGT")
        held += [sc, md]
        cigars = sec.cigars(sc)
        assert sum("I" in c for c in cigars) == 4 and sum("D" in c for c in cigars) == 2 and sum("^" in s for s in strings) == 2
    finally:
        close_all(held)
        mp.close()
        idx.close()


def test_scripts_md_and_xa_lines_of_the_tandem_repeat_and_a_workload(engine, repeat_index, repeat_mapped, work):
    text, _ = repeat_text()
    mp = repeat_mapped
    held = []
    try:
        sec = mp.pl.secondaries(mp.loci, mp.al, 32)
        held.append(sec)
        sc, md, _ = check_scripts_and_md(engine, repeat_index, mp, text, 4, sec, "ACGT")
        held += [sc, md]
        # SAM lines with XA: every item is rebuilt from the line alone against the text at its position
        psc = mp.pl.scripts(repeat_index, mp.reads, mp.loci, mp.al)
        held.append(psc)
        pmd = psc.md(repeat_index, mp.al, "ACGT")
        mq = mp.pl.mapq(8)
        held += [pmd, mq]
        xa = sec.xa(sc, rname="rep")
        nr = len(xa)
        args = ([f"q{i}" for i in range(nr)], mp.ranks, mp.roff, "ACGT", COMP4, 4, "rep", mp.pl.host(best2=False), mp.pl.cigars(psc), mp.pl.mds(pmd, psc), mq.host())
        lines = engine.sam_lines(*args, xa=xa)
        assert [ln for ln, s in zip(lines, xa) if not s] == [ln for ln, s in zip(engine.sam_lines(*args), xa) if not s]
        n_items = 0
        for i, ln in enumerate(lines):
            f = ln.split("\t")
            assert (f[-1].startswith("XA:Z:") and f[-2].startswith("MD:Z:")) == bool(xa[i])
            if not xa[i]:
                continue
            primary_reverse = int(f[1]) & 0x10
            for item in f[-1][5:].split(";")[:-1]:
                rname, pos, cigar, nm = item.split(",")
                assert rname == "rep" and re.fullmatch(r"[+-]\d+", pos)
                seq = np.asarray(["ACGT".index(x) for x in f[9]], np.uint8)
                if (pos[0] == "-") != bool(primary_reverse):
                    seq = rc4(seq)
                runs = [(int(a) << 4) | engine.CIGAR_OPS.index(b) for a, b in re.findall(r"([0-9]+)([MIDNSHP=X])", cigar)]
                ref_len = sum(v >> 4 for v in runs if engine.CIGAR_OPS[v & 15] in "=XD")
                at = int(pos[1:]) - 1
                assert scn.replay(seq, text[at:at + ref_len], np.asarray(runs, np.uint32), 4) == (int(nm), True), item
                n_items += 1
        assert n_items == sec.counts()["n_sec"] == 129
        # the entries of an ordinary workload (substitutions, a deletion and an insertion among the reads)
        wmp = work.workload("dna4_k10")
        wsec = wmp.pl.secondaries(wmp.loci, wmp.al, 4)
        held.append(wsec)
        held += list(check_scripts_and_md(engine, work.index("dna4_k10"), wmp, text_of(4, 50_000), 4, wsec, "ACGT")[:2])
    finally:
        close_all(held)


# ---- 7. handle reuse, the chain keyword, refusals -----------------------------------------------------------------------------------------
def test_one_handle_through_batches_of_every_size(repeat_index):
    pool = repeat_reads()
    sec = None
    held = []
    try:
        for nr, N in ((257, 32), (0, 32), (1, 1), (3, 1), (3, 32)):
            out = repeat_index.map_reads_strands(*pack([pool[i % len(pool)] for i in range(nr)]), 10, COMP4, **REPEAT_CHAIN)
            held += list(out)
            _, loci, al, pl = out
            sec = pl.secondaries(loci, al, N, secondaries=sec)
            want = check(sec, loci.host(), al.host(), pl, N)
            assert sec.counts()["nr"] == nr and (nr == 0) == (sec.device_ptrs()[6] is None)
            if nr == 0:
                assert sec.host()[0].tolist() == [0] and sec.device_ptrs()[0] is not None and sec.counts()["n_sec"] == 0
            if nr == 3:
                assert [len(entries_of(want, i)) for i in range(3)] == [N, N, 1]
            close_all(list(out))
            del held[-4:]
    finally:
        close_all(held + [sec])


def test_the_chain_keyword_appends_the_separate_call(engine, repeat_index):
    reads = pack(repeat_reads()[:4])
    held = []
    try:
        plain = repeat_index.map_reads_strands(*reads, 10, COMP4, **REPEAT_CHAIN, secondaries=0)
        held += list(plain)
        assert len(plain) == 4 and [type(h).__name__ for h in plain] == ["StrandReads", "Loci", "Alignments", "Placements"]
        out = repeat_index.map_reads_strands(*reads, 10, COMP4, **REPEAT_CHAIN, scripts=True, secondaries=3)
        held += list(out)
        assert len(out) == 6 and isinstance(out[5], engine.Secondaries) and isinstance(out[4], engine.Scripts)
        apart = plain[3].secondaries(plain[1], plain[2], 3)
        held.append(apart)
        for g, w in zip(out[5].host(), apart.host()):
            assert (g is None and w is None) or np.array_equal(g, w)
        assert out[5].counts() == apart.counts() and out[5].counts()["n_sec"] > 0
        check(out[5], out[1].host(), out[2].host(), out[3], 3)
        # pairs, and pairs with a rescue: the secondaries come last, behind the Rescues, and are those of the final placements
        text, _ = repeat_text()
        mates = pack([text[8800:8900].copy(), rc4(text[9200:9300]), text[300:400].copy(), kill(rc4(text[600:680]), 10)])
        kw = dict(REPEAT_CHAIN, min_insert=100, max_insert=600)
        for rescue in (False, True):
            plain = repeat_index.map_pairs(*mates, 10, COMP4, **kw, rescue=rescue, secondaries=0)
            held += list(plain)
            assert len(plain) == 5 + rescue and not any(isinstance(h, engine.Secondaries) for h in plain)
            out = repeat_index.map_pairs(*mates, 10, COMP4, **kw, rescue=rescue, secondaries=2)
            held += list(out)
            assert len(out) == 6 + rescue and isinstance(out[-1], engine.Secondaries) and (not rescue or isinstance(out[-2], engine.Rescues))
            for g, w in zip(out[3].host(), plain[3].host()):
                assert np.array_equal(g, w)
            apart = plain[3].secondaries(plain[1], plain[2], 2)
            held.append(apart)
            for g, w in zip(out[-1].host(), apart.host()):
                assert (g is None and w is None) or np.array_equal(g, w)
            want = check(out[-1], out[1].host(), out[2].host(), out[3], 2)
            assert len(entries_of(want, 0)) == 2 and int(want["more"][0]) == 1
            if rescue:
                assert out[-2].counts()["n_taken"] == 1 and out[3].host()[0][3] == NO and entries_of(want, 3) == []
    finally:
        close_all(held)


def test_refusals_after_looking_leave_an_empty_result(engine, repeat_index):
    """Untested: handles on different devices (one device)."""
    text, _ = repeat_text()
    idx = repeat_index
    four = pack([text[100:170].copy(), text[300:390].copy(), text[2000:2100].copy(), text[500:600].copy()])
    two = pack([text[100:170].copy(), text[2000:2100].copy()])
    two_b = pack([text[100:170].copy(), text[300:390].copy()])
    kw = dict(band=0, min_votes=8, max_edits=4)
    mp = MappedStrands(idx, 4, *two, 10, **kw)                     # 4 internal reads
    held = []
    try:
        loci3, al3 = idx.map_reads(*pack([text[100:170].copy()] * 3), 10, **kw)
        loci4, al4 = idx.map_reads(*four, 10, **kw)
        loci2, al2 = idx.map_reads(*two_b, 10, **kw)
        held += [loci3, al3, loci4, al4, loci2, al2]
        pl4 = al4.fold_strands(loci4)                          # 2 public reads, as mp.pl
        pl2 = al2.fold_strands(loci2)                          # 1 public read
        held += [pl4, pl2]
        assert loci4.counts()["n_loci"] != mp.loci.counts()["n_loci"] and loci4.counts()["nr"] == mp.loci.counts()["nr"] == 4
        sec = engine.Secondaries()
        held.append(sec)
        for call, word in ((lambda: pl2.secondaries(loci3, al3, 4, secondaries=sec), "odd"),
                           (lambda: pl4.secondaries(loci4, al2, 4, secondaries=sec), "the alignments handle's nr differs"),
                           (lambda: pl4.secondaries(loci2, al4, 4, secondaries=sec), "the alignments handle's nr differs"),
                           (lambda: pl4.secondaries(loci4, mp.al, 4, secondaries=sec), "the alignments handle's n_loci differs"),
                           (lambda: pl2.secondaries(loci4, al4, 4, secondaries=sec), "the placements are not those of these reads")):
            pl4.secondaries(loci4, al4, 4, secondaries=sec)
            assert sec.counts()["nr"] == 2 and sec.device_ptrs()[0] is not None
            said = refused(engine, call)
            assert "kmx_placements_secondaries" in said and word in said
            assert sec.counts() == {"nr": 0, "n_sec": 0, "n_multi": 0, "n_truncated": 0}
            h = sec.host()
            assert h[0].tolist() == [0] and all(x.size == 0 for x in h[1:5]) and h[5] is None and h[6].size == 0
            assert sec.device_ptrs() == (None,) * 7
        # before any handle is looked at: the result stays
        pl4.secondaries(loci4, al4, 4, secondaries=sec)
        L = engine.lib()
        for o in (engine.SecondaryOptions(16, 0, 0, 0), engine.SecondaryOptions(16, 33, 0, 0), engine.SecondaryOptions(16, 4, 0, 1), engine.SecondaryOptions(15, 4, 0, 0)):
            assert L.kmx_placements_secondaries(loci4._h, al4._h, pl4._h, C.byref(o), None, C.byref(sec._h)) == 1
            assert b"kmx_placements_secondaries" in L.kmx_last_error()
        assert sec.counts()["nr"] == 2
        # N of 1 and of 32 through the same handle
        for N in (1, 32):
            pl4.secondaries(loci4, al4, N, secondaries=sec)
            check(sec, loci4.host(), al4.host(), pl4, N)
    finally:
        close_all(held)
        mp.close()
