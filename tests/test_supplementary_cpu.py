"""Supplementary alignments without a device: tests/supp_naive.py on hand-made arrays with the expected output written out, the
planted reads of tests/chain_data.py through the CPU oracles alone (so that the GPU test's claims about its inputs are
shown before any device runs), the pure-Python SAM side of the engine on literal arrays, and the refusals of
kmx_clips_supplementaries that look at no handle."""
import ctypes as C

import numpy as np
import pytest

from tests import supp_naive as sp
from tests.chain_checks import supp_cpu_chain as cpu_chain, supp_oracle as oracle, supp_rows as rows
from tests.chain_data import COMP4, COPIES, LETTERS4 as LETTERS, SUPP_PLANTED as PLANTED, supp_planted_reads as planted_reads


# ---- 1. the contract on hand-made arrays ------------------------------------------------------------------------------------------------
def ent(strand, start, end, sl, sr, score, tl=0, tr=0, nm=0, low=0, runs=1):
    return dict(strand=strand, start=start, end=end, sl=sl, sr=sr, score=score, tl=tl, tr=tr, nm=nm, low=low, runs=runs)


def one_read(ents, primary=0, placed=None, m=150, **opt):
    """One public read of m letters whose entry e is ents[e] at a locus of its own (sel[e] = e), forward entries first; the
    placements name the locus `primary` on the strand of that entry (placed: another strand byte)."""
    strands = [x["strand"] for x in ents]
    assert strands == sorted(strands)
    n = len(ents)
    col = lambda k, dt: np.asarray([x[k] for x in ents], dt)
    clips = (col("score", np.int32), col("sl", np.uint16), col("sr", np.uint16), col("tl", np.uint16), col("tr", np.uint16), col("nm", np.uint16),
             col("low", np.uint8), np.concatenate([[0], np.cumsum([x["runs"] for x in ents])]).astype(np.uint64))
    strand = placed if placed is not None else (ents[primary]["strand"] if 0 <= primary < n else 0)
    pl = (np.asarray([primary], np.uint32), np.asarray([strand], np.uint8))
    return sp.supplementaries(np.asarray([0, m, 2 * m], np.uint64), col("start", np.uint32), col("end", np.uint32), None, pl,
                              np.asarray([0, strands.count(0), n], np.uint64), np.arange(n, dtype=np.uint32), clips, **opt)


PRIMARY = ent(0, 2000, 2150, 0, 50, 95, tr=50)                 # '100=50S': read [0, 100), text [2000, 2100)


def test_a_reverse_entry_covers_the_mirrored_read_interval():
    # '50=100S' of the reverse complement: the last 50 letters of the read as it was given
    out = one_read([PRIMARY, ent(1, 5500, 5650, 0, 100, 45, tr=100, nm=3)])
    assert rows(out) == [(1, 1, 100, 150, 5500, 5550, 45, 0)] and out["nm"].tolist() == [3] and out["locus"].tolist() == [1]
    assert out["more"].tolist() == [0] and (out["n_sup"], out["n_split"], out["n_truncated"]) == (1, 1, 0) and out["ctg"] is None
    # the same numbers on the forward strand are the FIRST 50 letters, inside the primary's: no entry
    assert rows(one_read([PRIMARY, ent(0, 5500, 5650, 0, 100, 45, tr=100)])) == []
    # the dtypes of the contract
    want = dict(sup_off=np.uint64, ent=np.uint32, locus=np.uint32, strand=np.uint8, q0=np.uint16, q1=np.uint16, t0=np.uint32, t1=np.uint32,
                score=np.int32, second_score=np.int32, nm=np.uint16, more=np.uint8)
    assert {k: out[k].dtype for k in want} == {k: np.dtype(v) for k, v in want.items()}


def test_a_tie_goes_to_the_least_entry():
    out = one_read([PRIMARY, ent(0, 5000, 5150, 100, 0, 45, tl=100), ent(0, 9000, 9150, 100, 0, 45, tl=100)])
    assert rows(out) == [(1, 0, 100, 150, 5100, 5150, 45, 45)]   # (and the loser, elsewhere in the text, is its runner-up)


def test_max_overlap_reached_and_exceeded_by_one():
    assert rows(one_read([PRIMARY, ent(0, 5000, 5150, 90, 0, 55, tl=90)])) == [(1, 0, 90, 150, 5090, 5150, 55, 0)]     # 10 letters shared
    assert rows(one_read([PRIMARY, ent(0, 5000, 5150, 89, 0, 56, tl=89)])) == []                                       # 11
    assert rows(one_read([PRIMARY, ent(0, 5000, 5150, 89, 0, 56, tl=89)], max_overlap=11)) == [(1, 0, 89, 150, 5089, 5150, 56, 0)]
    # against EVERY member of T: the third entry shares 5 letters with the primary and 25 with the part taken first
    ents = [PRIMARY, ent(0, 5000, 5150, 100, 0, 45, tl=100), ent(0, 7000, 7150, 95, 25, 25, tl=95, tr=25)]
    assert rows(one_read(ents)) == [(1, 0, 100, 150, 5100, 5150, 45, 25)]


def test_min_len_and_min_score_at_the_bound():
    assert rows(one_read([PRIMARY, ent(0, 5000, 5150, 130, 0, 20, tl=130)])) == [(1, 0, 130, 150, 5130, 5150, 20, 0)]
    assert rows(one_read([PRIMARY, ent(0, 5000, 5150, 131, 0, 20, tl=131)])) == []                                      # 19 letters
    assert rows(one_read([PRIMARY, ent(0, 5000, 5150, 130, 0, 19, tl=130)])) == []                                      # a score of 19
    assert rows(one_read([PRIMARY, ent(0, 5000, 5150, 131, 0, 19, tl=131)], min_len=19, min_score=19)) == [(1, 0, 131, 150, 5131, 5150, 19, 0)]


def test_low_entries_and_entries_without_runs_are_no_candidates():
    part = dict(strand=0, start=5000, end=5150, sl=100, sr=0, score=45, tl=100)
    assert rows(one_read([PRIMARY, ent(**part, low=1)])) == []
    assert rows(one_read([PRIMARY, ent(**part, runs=0)])) == []
    assert rows(one_read([PRIMARY, ent(**part)])) == [(1, 0, 100, 150, 5100, 5150, 45, 0)]
    # nor do they count as runners-up
    assert rows(one_read([PRIMARY, ent(**part), ent(0, 9000, 9150, 100, 0, 44, tl=100, low=1)])) == [(1, 0, 100, 150, 5100, 5150, 45, 0)]


def test_reads_without_a_usable_primary_have_no_entries():
    part = ent(0, 5000, 5150, 100, 0, 45, tl=100)
    assert rows(one_read([PRIMARY, part], primary=7)) == []                               # no entry at the placement's locus
    assert rows(one_read([PRIMARY, part], primary=0xFFFFFFFF, placed=0)) == []            # rescued
    assert rows(one_read([PRIMARY, part], placed=255)) == []                              # unplaced
    assert rows(one_read([dict(PRIMARY, runs=0), part])) == []                            # the primary has no runs
    out = one_read([PRIMARY, part], primary=7)
    assert out["sup_off"].tolist() == [0, 0] and out["more"].tolist() == [0] and (out["n_sup"], out["n_split"], out["n_truncated"]) == (0, 0, 0)
    # a LOW primary is a primary still
    assert rows(one_read([dict(PRIMARY, low=1), part])) == [(1, 0, 100, 150, 5100, 5150, 45, 0)]


def test_truncation_at_n_reports_more_and_the_entries_ascend():
    first = ent(0, 2000, 2150, 0, 120, 25, tr=120)             # read [0, 30)
    parts = [ent(0, 3000 + 1000 * k, 3150 + 1000 * k, 30 * k, 150 - 30 * (k + 1), s, tl=30 * k, tr=150 - 30 * (k + 1))
             for k, s in ((1, 25), (2, 28), (3, 26), (4, 27))]
    out = one_read([first] + parts, max_supplementary=3, max_overlap=0)
    assert [r[0] for r in rows(out)] == [2, 3, 4] and out["more"].tolist() == [1] and out["n_truncated"] == 1    # taken: 2, 4, 3
    out = one_read([first] + parts, max_supplementary=4, max_overlap=0)
    assert [r[:4] for r in rows(out)] == [(1, 0, 30, 60), (2, 0, 60, 90), (3, 0, 90, 120), (4, 0, 120, 150)] and out["more"].tolist() == [0]
    out = one_read([first] + parts, max_supplementary=1, max_overlap=0)
    assert [r[0] for r in rows(out)] == [2] and out["more"].tolist() == [1]


def test_the_shadow_of_the_primary_stays_out_and_a_part_on_its_text_interval_comes_in():
    shadow = ent(0, 2003, 2153, 0, 50, 90, tr=50)              # the same read letters from a neighbouring locus
    inside = ent(0, 1930, 2080, 100, 0, 45, tl=100)            # read [100, 150) on text [2030, 2080): a tandem duplication
    assert rows(one_read([PRIMARY, shadow, inside])) == [(2, 0, 100, 150, 2030, 2080, 45, 0)]


def test_the_runner_up_lies_elsewhere_in_the_text():
    ents = [PRIMARY,
            ent(0, 4900, 5050, 100, 0, 45, tl=100),            # the part: text [5000, 5050)
            ent(0, 4910, 5060, 100, 0, 44, tl=100),            # the same place, ten letters on: not a runner-up
            ent(0, 8895, 9045, 105, 0, 40, tl=105),            # elsewhere: the runner-up
            ent(1, 4900, 5050, 0, 100, 30, tr=100)]            # the same coordinates on the other strand: elsewhere too, but worse
    assert rows(one_read(ents)) == [(1, 0, 100, 150, 5000, 5050, 45, 40)]
    assert rows(one_read(ents[:3])) == [(1, 0, 100, 150, 5000, 5050, 45, 0)]
    assert rows(one_read(ents[:3] + ents[4:])) == [(1, 0, 100, 150, 5000, 5050, 45, 30)]


def test_offsets_are_clamped_and_foreign_loci_are_no_candidates():
    part = ent(0, 5000, 5150, 100, 0, 45, tl=100)
    clips = (np.asarray([95, 45], np.int32),) + tuple(np.asarray(v, np.uint16) for v in ([0, 100], [50, 0], [0, 100], [50, 0], [0, 0])) + (
        np.zeros(2, np.uint8), np.asarray([0, 1, 2], np.uint64))
    pl = (np.asarray([0], np.uint32), np.asarray([0], np.uint8))
    args = (np.asarray([0, 150, 300], np.uint64), np.asarray([2000, 5000], np.uint32), np.asarray([2150, 5150], np.uint32), None, pl)
    assert rows(sp.supplementaries(*args, np.asarray([0, 9, 5], np.uint64), np.asarray([0, 1], np.uint32), clips)) == [(1, 0, 100, 150, 5100, 5150, 45, 0)]
    assert rows(sp.supplementaries(*args, np.asarray([0, 2, 2], np.uint64), np.asarray([0, 7], np.uint32), clips)) == []   # sel beyond n_loci
    assert part["score"] == 45


# ---- 2. the planted reads of the GPU test, on the CPU ----------------------------------------------------------------------------------------
def test_the_planted_reads_yield_what_the_gpu_test_relies_on():
    c = cpu_chain()
    at = {name: i for i, name in enumerate(PLANTED)}
    strand, dist = c["placements"][1], c["placements"][2]
    ents = lambda i: int(c["read_sel_off"][2 * i + 2]) - int(c["read_sel_off"][2 * i])
    out = oracle(c)
    got = {name: [r[1:] for r in rows(out, at[name])] for name in PLANTED}
    # both halves of a 100 + 50 split are aligned at E = 110: the primary within 50 edits, the other half within 100
    assert got["plain"] == [] and strand[at["plain"]] == 0 and dist[at["plain"]] == 0
    assert got["split"] == [(0, 100, 150, 5000, 5050, 45, 0)] and dist[at["split"]] <= 50
    assert got["split_rc"] == [(1, 100, 150, 5500, 5550, 45, 0)] and strand[at["split_rc"]] == 0
    assert got["split_rc_whole"] == [(0, 0, 50, 5500, 5550, 45, 0)] and strand[at["split_rc_whole"]] == 1
    # (one letter of the neighbouring part fits the third part's script by chance)
    assert got["three"] == [(0, 60, 110, 6000, 6050, 40, 0), (0, 109, 150, 7499, 7540, 36, 0)]
    assert got["dup"] == [(0, 99, 150, 8999, 9050, 46, 46)]    # the copy at 11 000 scores the same: the runner-up, MAPQ 0
    assert got["adapter"] == [] and got["short"] == [] and got["outside"] == [] and strand[at["outside"]] == 255
    assert ents(at["adapter"]) == 1 and ents(at["short"]) >= 2 and ents(at["outside"]) == 0
    # A tandem duplication on one strand is NOT found through this chain: kmx_loci_align takes the least distance in a window of
    # max_edits letters around a locus, so the locus of the second part, 70 letters from the primary's, finds the primary's own
    # alignment again; the two entries are one place and cover the same read letters.  Inverted, the second part is a read of the
    # other strand and comes out, on the primary's own text interval
    e0 = int(c["read_sel_off"][2 * at["tandem"]])
    assert got["tandem"] == [] and ents(at["tandem"]) == 2 and c["strings"][e0] == c["strings"][e0 + 1] == "100=50S"
    assert c["start"][c["sel"][e0]] == c["start"][c["sel"][e0 + 1]] == 6500
    assert got["inverted"] == [(1, 100, 150, 7030, 7080, 45, 0)]
    # 132 entries, 131 candidates: three strides of a wave; every other copy of the second unit is a runner-up
    assert ents(at["many"]) == 2 * COPIES and len(got["many"]) == 1 and got["many"][0][5] == got["many"][0][6] >= 35
    assert out["more"].tolist() == [0] * len(planted_reads()) and out["n_truncated"] == 0
    assert sp.mapq(out["score"], out["second_score"])[int(out["sup_off"][at["dup"]])] == 0
    # N = 1: the three-part read keeps its better part and reports more
    one = oracle(c, max_supplementary=1)
    assert [r[1:] for r in rows(one, at["three"])] == [(0, 60, 110, 6000, 6050, 40, 0)]
    assert one["more"].tolist() == [int(i == at["three"]) for i in range(len(planted_reads()))] and one["n_truncated"] == 1
    # the fillers have no parts (a chance locus of theirs is junk: LOW, or short)
    assert out["sup_off"][-1] == out["sup_off"][len(PLANTED)] == out["n_sup"] == 8 and out["n_split"] == 7
    # the primary of every placed read is among the entries, with runs
    for i, (l, s) in enumerate(zip(c["placements"][0], strand)):
        if s != 255:
            e = [e for e in range(int(c["read_sel_off"][2 * i]), int(c["read_sel_off"][2 * i + 2])) if c["sel"][e] == l]
            assert len(e) == 1 and c["strings"][e[0]], i


# ---- 3. the SAM side, on literal arrays ------------------------------------------------------------------------------------------------------
def test_sa_strings_and_the_mapq_rule(engine):
    primary = ([2000, 1000], [0, 0], ["100=50S", "150="], [60, 37], [0, 2])
    entries = ([5000, 7000], [1, 0], ["50=100S", ""], [60, 0], [0, 4])
    got = engine.sa_strings([0, 2, 2], primary, entries, rname="chr")
    assert got == [["chr,5001,-,50=100S,60,0;chr,7001,+,*,0,4;", "chr,2001,+,100=50S,60,0;chr,7001,+,*,0,4;",
                    "chr,2001,+,100=50S,60,0;chr,5001,-,50=100S,60,0;"], [""]]
    located = (("c0", "c1"), np.asarray([0, 4000, 20_000], np.uint64))
    got = engine.sa_strings([0, 1, 1], tuple(primary) + ([0, 0],), tuple(x[:1] for x in entries) + ([1],), located=located)
    assert got == [["c1,1001,-,50=100S,60,0;", "c0,2001,+,100=50S,60,0;"], [""]]
    with pytest.raises(ValueError):
        engine.sa_strings([0, 1, 1], primary, entries)
    with pytest.raises(ValueError):
        engine.sa_strings([0, 1, 1], primary, entries, located=located)
    q = engine.supplementary_mapq([45, 46, 40, 10, 45], [0, 46, 20, 50, 44])
    assert q.dtype == np.uint8 and q.tolist() == [60, 0, 30, 0, 1] == sp.mapq([45, 46, 40, 10, 45], [0, 46, 20, 50, 44])
    assert engine.supplementary_mapq([45, 40], [0, 20], cap=30).tolist() == [30, 15]


def small_batch():
    ranks = np.asarray([0, 1, 2, 3, 0, 1, 3, 3, 2, 2, 1, 1], np.uint8)
    roff = np.asarray([0, 6, 12], np.uint64)
    placements = (np.asarray([0, 1], np.uint32), np.asarray([0, 1], np.uint8), np.asarray([0, 1], np.uint8), np.asarray([10, 20], np.uint32),
                  np.asarray([14, 26], np.uint32), np.asarray([255, 255], np.uint8))
    fields = (np.asarray([0, 0]), np.asarray([0, 1]), np.asarray([4, 1]), np.asarray([True, True]))
    args = (["r0", "r1"], ranks, roff, LETTERS, COMP4, 4, "chr", placements, ["4=2S", "6="], ["4", "6"], np.asarray([60, 30], np.uint8))
    return args, fields


def test_sam_lines_gain_sa_behind_xa_and_none_leaves_them(engine):
    args, fields = small_batch()
    xa = ["chr,+5,6=,0;", ""]
    sa = [["chr,31,-,2=4S,60,0;", "chr,11,+,4=2S,60,0;"], [""]]
    old = engine.sam_lines(*args, xa=xa, clip_fields=fields)
    assert old == ["r0\t0\tchr\t11\t60\t4=2S\t*\t0\t0\tACGTAC\t*\tNM:i:0\tMD:Z:4\tAS:i:4\tXA:Z:chr,+5,6=,0;",
                   "r1\t16\tchr\t21\t30\t6=\t*\t0\t0\tGGCCAA\t*\tNM:i:1\tMD:Z:6\tAS:i:1"]
    assert engine.sam_lines(*args, xa=xa, clip_fields=fields, sa=None) == old
    new = engine.sam_lines(*args, xa=xa, clip_fields=fields, sa=sa)
    assert new == [old[0] + "\tSA:Z:chr,31,-,2=4S,60,0;", old[1]]
    with pytest.raises(ValueError):
        engine.sam_lines(*args, sa=sa[:1])


def test_sam_supplementary_lines(engine):
    args, fields = small_batch()
    sa = [["chr,31,-,2=4S,60,0;", "chr,11,+,4=2S,60,0;"], [""]]
    primary = engine.sam_lines(*args, clip_fields=fields, sa=sa)
    u32 = lambda *v: np.asarray(v, np.uint32)
    host = (np.asarray([0, 1, 1], np.uint64), u32(3), u32(7), np.asarray([1], np.uint8), np.asarray([4], np.uint16), np.asarray([6], np.uint16), u32(30),
            u32(32), np.asarray([2], np.int32), np.asarray([0], np.int32), np.asarray([0], np.uint16), None, np.asarray([0, 0], np.uint8))
    ranks, roff = args[1], args[2]
    got = engine.sam_supplementary_lines(primary, ranks, roff, LETTERS, COMP4, 4, host, ["2=4S"], ["2"], [60], sa, rname="chr")
    assert got == ["r0\t2064\tchr\t31\t60\t2=4S\t*\t0\t0\tGTACGT\t*\tNM:i:0\tMD:Z:2\tAS:i:2\tSA:Z:chr,11,+,4=2S,60,0;"]
    # a mate: the pair bits without 0x2, RNEXT and PNEXT of the primary line, the mate's contig by name when the part lies on another
    paired = ["p\t99\tc0\t11\t60\t4=2S\t=\t301\t296\tACGTAC\t*\tNM:i:0", "p\t147\tc0\t301\t60\t6=\t=\t11\t-296\tGGCCAA\t*"]
    located = (("c0", "c1"), np.asarray([0, 25, 100], np.uint64))
    got = engine.sam_supplementary_lines(paired, ranks, roff, LETTERS, COMP4, 4, host[:11] + (u32(1),) + host[12:], ["2=4S"], ["2"], [60], sa,
                                         located=located)
    assert got == ["p\t2161\tc1\t6\t60\t2=4S\tc0\t301\t0\tGTACGT\t*\tNM:i:0\tMD:Z:2\tAS:i:2\tSA:Z:chr,11,+,4=2S,60,0;"]
    got = engine.sam_supplementary_lines(paired, ranks, roff, LETTERS, COMP4, 4, host[:6] + (u32(20),) + host[7:11] + (u32(0),) + host[12:], ["2=4S"],
                                         ["2"], [60], sa, located=located)
    assert got[0].split("\t")[:9] == ["p", "2161", "c0", "21", "60", "2=4S", "=", "301", "0"]
    with pytest.raises(ValueError):
        engine.sam_supplementary_lines(primary, ranks, roff, LETTERS, COMP4, 4, host, ["2=4S"], ["2"], [60], sa)
    with pytest.raises(ValueError):
        engine.sam_supplementary_lines(primary, ranks, roff, LETTERS, COMP4, 4, host, ["2=4S"], ["2"], [60], sa, located=located)
    with pytest.raises(ValueError):
        engine.sam_supplementary_lines(primary, ranks, roff, LETTERS, COMP4, 4, host, [], ["2"], [60], sa, rname="chr")


# ---- 4. the refusals that look at no handle --------------------------------------------------------------------------------------------------
def test_the_options_are_refused_before_any_handle_is_looked_at(engine):
    L = engine.lib()
    out = C.c_void_p()

    def call(*fields, o=True, inout=True):
        opt = engine.SupplementaryOptions(*fields)
        st = L.kmx_clips_supplementaries(None, None, None, None, None, None, C.byref(opt) if o else None, None, C.byref(out) if inout else None)
        assert st == 1 and out.value is None
        return L.kmx_last_error().decode()

    assert C.sizeof(engine.SupplementaryOptions) == 24 and engine.SUPPLEMENTARY_MAX == sp.SUPPLEMENTARY_MAX == 8
    good = (24, 4, 20, 10, 20, 0)
    assert "options is NULL" in call(*good, o=False) and "inout is NULL" in call(*good, inout=False)
    assert "struct_size" in call(20, 4, 20, 10, 20, 0) and "flags" in call(24, 4, 20, 10, 20, 1)
    assert "max_supplementary" in call(24, 0, 20, 10, 20, 0) and "max_supplementary" in call(24, 9, 20, 10, 20, 0)
    assert "min_len" in call(24, 4, 0, 10, 20, 0) and "min_len" in call(24, 4, 65536, 10, 20, 0)
    assert "min_score" in call(24, 4, 20, 10, 0, 0) and "min_score" in call(24, 4, 20, 10, -5, 0)
    # with options that pass, the first NULL handle is named
    assert "strand reads handle is NULL" in call(*good) and "strand reads handle is NULL" in call(24, 8, 65535, 0xFFFFFFFF, 1, 0)
    assert L.kmx_supplementaries_counts(None, None, None, None, None) == 1
    L.kmx_supplementaries_free(None)
