"""Affine-gap local realignment on the GPU: kmx_scripts_realign[_device] and the `realign=` keyword of the chain calls.  The oracle is
always tests/realign_naive.py on the host views of the engine's own handles (the scripts, the alignments, the reads as the device
holds them, the text); every array, its dtype and every counter must be identical, and the device views must equal the host views.
tests/test_realign_cpu.py shows on the CPU alone what the planted reads must give.  No batch is larger than those of the chain tests
(tests/chain_data.py).  Gaps in the classes of more than one diagonal per lane, the tie rules on texts of low complexity, the
scorings at the bounds of the header and seeded batches: tests/test_realign_bands_gpu.py.  Untested: an index with several replicas,
and the different-devices refusals."""
import ctypes as C

import numpy as np
import pytest

from kmer_index_amd import synth
from tests import clip_naive as cn
from tests import realign_naive as rn
from tests.chain_checks import check_clip_md, check_clips, check_realign, check_supp, close_all, doubled, entry_of, refused, same
from tests.chain_data import (CHAIN as PAIR_CHAIN, CLIP_CHAIN as CHAIN, CLIP_PLANTED, CLIPS, COMP4, INSERT, K, LETTERS4 as LETTERS, M, PAIR_WORKLOADS, SCRIPTS,
                              boundary_reads, clip_planted_reads, clip_text as text, edited, other, realign_batch as batch, rescue_pairs_of, table_reads,
                              text_of)
from tests.helpers import pack

pytestmark = pytest.mark.gpu

ZERO = dict(mismatch=0, gap_open=0, gap_extend=0, clip_penalty=0)
EMPTY = dict(n_sel=0, n_ops=0, n_clipped=0, n_low=0)


def oracle(sc, al, ranks, roff, txt=None, **opt):
    dist, start, end = al.host()[:3]
    return rn.realign(*sc.host(), dist, start, end, ranks, roff, text() if txt is None else txt, 4, **dict(rn.DEFAULTS, **opt))


@pytest.fixture(scope="module")
def index(engine):
    idx = engine.Index(text(), 4, [K], table=2)
    yield idx
    idx.close()


@pytest.fixture(scope="module")
def mapped(index):
    out = index.map_reads_strands(*pack(batch()), K, COMP4, **CHAIN, scripts=True)
    yield out
    close_all(list(out))


# ---- 1. the planted reads -----------------------------------------------------------------------------------------------------------------
def test_planted_reads_equal_the_oracle_at_four_settings_and_leave_the_scripts_alone(engine, index, mapped):
    reads, loci, al, pl, sc = mapped
    ranks2, roff2 = doubled(reads)
    d_ranks2, d_roff2, nr2, stream = reads.device_ptrs()
    before = (sc.host(), sc.device_ptrs(), sc.counts())
    at = {name: i for i, name in enumerate(CLIP_PLANTED + ("deletion", "insertion", "chimera"))}
    at = {name: (i if i < 7 else i + 40) for name, i in at.items()}                            # (the 40 fillers lie between)
    ent = {name: entry_of(pl, sc, i) for name, i in at.items() if name != "outside"}
    field = lambda out, name: (out["strings"][ent[name]], int(out["score"][ent[name]]), int(out["sl"][ent[name]]), int(out["sr"][ent[name]]),
                               int(out["tl"][ent[name]]), int(out["tr"][ent[name]]), int(out["nm"][ent[name]]), int(out["cflags"][ent[name]]))
    held = []
    try:
        cl = sc.realign_device(index, al, d_ranks2, d_roff2, nr2, stream=stream)
        held.append(cl)
        assert cl.scripts is sc
        five = check_realign(cl, sc, oracle(sc, al, ranks2, roff2))
        R = engine.CLIP_REALIGNED
        assert field(five, "unedited") == ("150=", 150, 0, 0, 0, 0, 0, R)
        assert field(five, "three_subs") == ("5S145=", 140, 5, 0, 2, 0, 0, R)
        assert field(five, "tail") == ("138=12S", 133, 0, 12, 0, 11, 0, R)
        assert field(five, "tail_reverse")[:4] == ("138=12S", 133, 0, 12)
        assert field(five, "over_end") == ("140=10S", 135, 0, 10, 0, 0, 0, R)
        assert field(five, "over_start") == ("10S140=", 135, 10, 0, 0, 0, 0, R)
        # the two reads that the unit-cost script breaks into pieces: the oracle decides whether the chain's loci give the table's CIGARs
        for name, op, whole, score in (("deletion", "D", "70=12D80=", 132), ("insertion", "I", "70=4I76=", 136)):
            got, script = field(five, name), sc.strings()[ent[name]]
            assert got[0].count(op) == 1 and got[7] == R, (name, script)
            if rn.strings(*oracle_one(sc, al, ranks2, roff2, ent[name])) == [whole]:
                assert got[:2] == (whole, score), name
        assert field(five, "chimera")[0].endswith("S") and field(five, "chimera")[2] == 0 and field(five, "chimera")[3] >= 25
        assert five["n_low"] == 0 and (five["cflags"] == R).all()
        # against the trimmer on the same handle: never less, and more where a gap was in pieces
        trimmed = sc.clip()
        held.append(trimmed)
        assert (five["score"] >= trimmed.host()[0]).all() and int(five["score"][ent["deletion"]]) > int(trimmed.host()[0][ent["deletion"]])
        # MD of the realigned entries, over [start + tl, end - tr)
        md = cl.md(index, sc, al, LETTERS)
        held.append(md)
        _, start, end = al.host()[:3]
        strings = check_clip_md(md, five, start, end, text())
        assert md.counts()["n_mismatched"] == 0 and strings[ent["three_subs"]] == "145" and "^" in strings[ent["deletion"]]
        tl, nm, score, has = pl.clip_fields(cl, sc)
        assert (tl[at["three_subs"]], nm[at["three_subs"]], score[at["three_subs"]]) == (2, 0, 140) and not has[at["outside"]]
        # p = 0 and all-zero penalties through the same handle, by the host form; a floor that flips entries to LOW
        assert sc.realign(index, al, ranks2, roff2, clip_penalty=0, clips=cl) is cl
        zero = check_realign(cl, sc, oracle(sc, al, ranks2, roff2, clip_penalty=0))
        assert zero["n_clipped"] > five["n_clipped"] and field(zero, "three_subs") == ("5S145=", 145, 5, 0, 2, 0, 0, R)
        sc.realign(index, al, ranks2, roff2, **ZERO, clips=cl)
        check_realign(cl, sc, oracle(sc, al, ranks2, roff2, **ZERO))
        sc.realign_device(index, al, d_ranks2, d_roff2, nr2, min_score=134, stream=stream, clips=cl)
        low = check_realign(cl, sc, oracle(sc, al, ranks2, roff2, min_score=134))
        assert field(low, "tail") == (sc.strings()[ent["tail"]], 117, 0, 0, 0, 0, 6, engine.CLIP_LOW)
        assert field(low, "over_end") == field(five, "over_end") and 0 < low["n_low"] < low["sel"].size
        # the scripts are untouched
        after = (sc.host(), sc.device_ptrs(), sc.counts())
        assert before[1:] == after[1:]
        same(SCRIPTS, after[0], before[0])
    finally:
        close_all(held)


def oracle_one(sc, al, ranks, roff, e):
    """(cig_off, cigar) of the oracle for entry e alone"""
    read_sel_off, sel, cig_off, cigar = sc.host()
    dist, start, end = al.host()[:3]
    r = int(np.searchsorted(read_sel_off, e, side="right")) - 1
    l = int(sel[e])
    runs = rn.realign_one(ranks[int(roff[r]):int(roff[r + 1])], text()[int(start[l]):int(end[l])], int(dist[l]), 4,
                          cigar[int(cig_off[e]):int(cig_off[e + 1])])[0]
    return [0, len(runs)], runs


# ---- 2. every class of the band and every boundary of the 64-row store, one entry per chunk ---------------------------------------------
def test_every_class_and_row_boundary_with_one_entry_per_chunk(engine, index):
    voters, aligned = boundary_reads()
    ranks, roff = pack(aligned)
    held = [index.vote_windows(*pack(voters), K, 1, 8, 2, 0)]
    try:
        loci = held[0]
        al = loci.align(index, ranks, roff, 250, 64)
        held.append(al)
        sc = al.scripts(index, loci, ranks, roff)
        held.append(sc)
        sel = sc.host()[1]
        d = al.host()[0][sel]
        assert sel.size == len(aligned) and sc.counts()["n_mismatched"] == 0
        assert {0, 1, 2, 3} == {0 if x < 32 else 1 if x < 64 else 2 if x < 128 else 3 for x in d.tolist()} and d.max() >= 240
        want = oracle(sc, al, ranks, roff)
        cl = sc.realign(index, al, ranks, roff, scratch_bytes=1)                # clamped up to the largest entry: a chunk per long read
        held.append(cl)
        out = check_realign(cl, sc, want)
        assert (out["cflags"] == engine.CLIP_REALIGNED).all() and out["strings"][4] == "249S51=1X99=1X99=1X99=1X99=1X73=250S"
        assert (int(out["tl"][4]), int(out["tr"][4]), int(out["nm"][4]), int(out["score"][4])) == (243, 223, 5, 490)
        assert out["strings"][5] == "1=" and out["n_clipped"] >= 9
        read_ops = (rn.OP_EQ, rn.OP_X, rn.OP_I, rn.OP_S)
        assert [cn.letters_of(cn.parse(c), read_ops) for c in out["strings"]] == [len(q) for q in aligned]
        other_cl = sc.realign(index, al, ranks, roff)
        held.append(other_cl)
        same(CLIPS, other_cl.host(), cl.host())
        assert other_cl.counts() == cl.counts()
    finally:
        close_all(held)


# ---- 3. reads of letters outside the alphabet --------------------------------------------------------------------------------------------
def test_reads_of_nothing_but_insertions_stay_whole_and_low(engine, index):
    ranks, roff = pack(clip_planted_reads()[:6] + [text()[9000:9120].copy()])
    blank = np.full(ranks.size, 255, np.uint8)
    held = [index.vote_windows(ranks, roff, K, 1, 8, 2, 0)]
    try:
        loci = held[0]
        al = loci.align(index, blank, roff, 250, 64)
        held.append(al)
        sc = al.scripts(index, loci, blank, roff, all=True)
        held.append(sc)
        m = np.repeat(np.diff(roff.astype(np.int64)), np.diff(sc.host()[0].astype(np.int64)))
        assert m.size >= 6 and sc.strings() == [f"{x}I" for x in m]
        cl = sc.realign(index, al, blank, roff)
        held.append(cl)
        want = check_realign(cl, sc, oracle(sc, al, blank, roff))
        assert want["strings"] == sc.strings() and want["score"].tolist() == (-(6 + m)).tolist() and want["nm"].tolist() == m.tolist()
        assert (want["cflags"] == engine.CLIP_LOW).all() and want["n_low"] == m.size and want["n_clipped"] == 0
        assert not any(want[k].any() for k in ("sl", "sr", "tl", "tr"))
        # a floor that they meet changes nothing: there is no path to take
        sc.realign(index, al, blank, roff, clip_penalty=0, min_score=-1000, clips=cl)
        free = check_realign(cl, sc, oracle(sc, al, blank, roff, clip_penalty=0, min_score=-1000))
        assert free["strings"] == sc.strings() and free["n_low"] == m.size
    finally:
        close_all(held)


# ---- 4. every aligned locus of 30 reads, and the supplementary alignments on top ----------------------------------------------------------
def test_all_loci_of_thirty_reads_and_their_supplementaries(engine, index):
    t = text()
    pool = [x for x in batch() if x.max() < 4]
    reads30 = pool[:26] + table_reads() + [np.concatenate([t[13_000:13_100], t[15_000:15_050]])]       # the last one: 100 + 50 letters of two places
    assert len(reads30) == 30
    # (within 110 edits, as in tests/test_supplementary_gpu.py: either part of a split read is aligned as a whole read)
    held = list(index.map_reads_strands(*pack(reads30), K, COMP4, **dict(CHAIN, max_edits=110)))
    try:
        reads, loci, al, pl = held
        ranks2, roff2 = doubled(reads)
        d_ranks2, d_roff2, nr2, stream = reads.device_ptrs()
        asc = al.scripts_device(index, loci, d_ranks2, d_roff2, nr2, all=True, stream=stream)
        held.append(asc)
        acl = asc.realign_device(index, al, d_ranks2, d_roff2, nr2, clip_penalty=2, stream=stream)
        held.append(acl)
        want = check_realign(acl, asc, oracle(asc, al, ranks2, roff2, clip_penalty=2))
        assert asc.counts()["n_sel"] == al.counts()["n_aligned"] >= 30 and want["n_clipped"] >= 3
        trimmed = asc.clip(clip_penalty=2, stream=stream)
        held.append(trimmed)
        assert (want["score"] >= trimmed.host()[0]).all() and (want["score"] > trimmed.host()[0]).any()
        sup = acl.supplementaries(reads, loci, al, pl, asc, stream=stream)
        held.append(sup)
        got = check_supp(sup, reads, al, pl, asc, acl)
        assert got["n_sup"] >= 1 and "100S50=" in sup.cigars()  # the second part of the last read
    finally:
        close_all(held)


# ---- 5. refusals and lifecycle ---------------------------------------------------------------------------------------------------------------
def test_refusals_no_entries_and_one_handle_through_sizes_and_both_calls(engine, index):
    pool = [x for x in batch() if x.max() < 4]
    ranks, roff = pack(pool[:30])
    held = list(index.map_reads(ranks, roff, K, **CHAIN))
    try:
        loci, al = held
        sc = al.scripts(index, loci, ranks, roff, all=True)
        held.append(sc)
        cl = sc.realign(index, al, ranks, roff)
        held.append(cl)
        check_realign(cl, sc, oracle(sc, al, ranks, roff))
        # '=' and 'X' joined: refused after looking, and the handle then holds an empty result
        joined = al.scripts(index, loci, ranks, roff, m=True)
        held.append(joined)
        assert "KMX_SCRIPT_M" in refused(engine, lambda: joined.realign(index, al, ranks, roff, clips=cl), "kmx_scripts_realign")
        assert cl.counts() == EMPTY and cl.device_ptrs() == (None,) * 9
        h = cl.host()
        assert h[7].tolist() == [0] and all(x.size == 0 for x in h[:7] + h[8:]) and cl.strings() == []
        # other reads than the scripts': refused after looking
        sc.realign(index, al, ranks, roff, clips=cl)
        assert "nr differs" in refused(engine, lambda: sc.realign(index, al, ranks[:int(roff[29])], roff[:30], clips=cl), "kmx_scripts_realign")
        assert cl.counts() == EMPTY
        # a refusal before looking leaves the result
        sc.realign(index, al, ranks, roff, clips=cl)
        n_sel = sc.counts()["n_sel"]
        for o in (engine.RealignOptions(32, 1, 4, 6, 1, 5, 0, 0, 0), engine.RealignOptions(40, 0, 4, 6, 1, 5, 0, 0, 0),
                  engine.RealignOptions(40, 1, 256, 6, 1, 5, 0, 0, 0), engine.RealignOptions(40, 1, 4, 6, 1, 65536, 0, 0, 0),
                  engine.RealignOptions(40, 1, 4, 6, 1, 5, 0, 1, 0)):
            assert engine.lib().kmx_scripts_realign(index._h, al._h, sc._h, ranks.ctypes.data, roff.ctypes.data, roff.size - 1, C.byref(o),
                                                    C.byref(cl._h)) == 1
            assert cl.counts()["n_sel"] == n_sel
        # no entries: a read without a window
        nothing = list(index.map_reads(*pack([np.full(M, 4, np.uint8)]), K, **CHAIN))
        held += nothing
        none = pack([np.full(M, 4, np.uint8)])
        empty = nothing[1].scripts(index, nothing[0], *none)
        held.append(empty)
        empty.realign(index, nothing[1], *none, clips=cl)
        assert empty.counts()["n_sel"] == 0 and cl.counts() == EMPTY and cl.host()[7].tolist() == [0] and cl.device_ptrs()[7] is not None
        # small / large / small through the one handle, the trimmer and the realignment by turns
        for n_reads in (2, 30, 1):
            rk, ro = pack(pool[:n_reads])
            lo2, al2 = index.map_reads(rk, ro, K, **CHAIN)
            held += [lo2, al2]
            sc2 = al2.scripts(index, lo2, rk, ro, all=True)
            held.append(sc2)
            sc2.realign(index, al2, rk, ro, clip_penalty=0, clips=cl)
            check_realign(cl, sc2, oracle(sc2, al2, rk, ro, clip_penalty=0))
            sc2.clip(clip_penalty=0, clips=cl)
            check_clips(cl, sc2, clip_penalty=0)
            sc2.realign(index, al2, rk, ro, clips=cl)
            check_realign(cl, sc2, oracle(sc2, al2, rk, ro))
    finally:
        close_all(held)


# ---- 6. the chain keyword -------------------------------------------------------------------------------------------------------------------
def test_the_chain_keyword_puts_the_realignment_in_the_trimmer_s_place(engine, index):
    picked = clip_planted_reads()[:6] + clip_planted_reads()[7:11] + table_reads()[:2]        # (sam_lines refuses a letter outside the alphabet)
    reads = pack(picked)
    held = []
    try:
        for kw in (dict(scripts=True), dict(clip={}), dict()):
            with pytest.raises(ValueError):
                index.map_reads_strands(*reads, K, COMP4, **CHAIN, **kw, realign={})
        # realign=None: the tuple of today, the trimmer's clips
        plain = index.map_reads_strands(*reads, K, COMP4, **CHAIN, scripts=True, clip=dict(clip_penalty=2), realign=None)
        held += list(plain)
        assert [type(h).__name__ for h in plain] == ["StrandReads", "Loci", "Alignments", "Placements", "Scripts", "Clips"]
        check_clips(plain[5], plain[4], clip_penalty=2)
        out = index.map_reads_strands(*reads, K, COMP4, **CHAIN, scripts=True, tags=True, letters=LETTERS, clip=dict(clip_penalty=2),
                                      realign=dict(scratch_bytes=1 << 20))
        held += list(out)
        assert [type(h).__name__ for h in out] == ["StrandReads", "Loci", "Alignments", "Placements", "Scripts", "SamTags", "Clips"]
        rd, loci, al, pl, sc, tags, cl = out
        assert cl.scripts is sc
        same(SCRIPTS, sc.host(), plain[4].host())
        ranks2, roff2 = doubled(rd)
        d_ranks2, d_roff2, nr2, stream = rd.device_ptrs()
        want = check_realign(cl, sc, oracle(sc, al, ranks2, roff2, clip_penalty=2))
        apart = sc.realign_device(index, al, d_ranks2, d_roff2, nr2, clip_penalty=2, stream=stream)
        held.append(apart)
        same(CLIPS, cl.host(), apart.host())
        assert cl.counts() == apart.counts() and (want["cflags"] == engine.CLIP_REALIGNED).all()
        _, start, end = al.host()[:3]
        check_clip_md(tags.md, want, start, end, text())  # with tags the MD is that of the realigned entries
        # SAM lines from the fields of the realigned clips: the CIGAR, POS moved by tl, AS behind MD
        fields = pl.clip_fields(cl, sc)
        lines = engine.sam_lines([f"q{i}" for i in range(len(picked))], *reads, LETTERS, COMP4, 4, "chr", pl.host(best2=False), pl.cigars(sc, cl),
                                 pl.mds(tags.md, sc), tags.mapq.host(), clip_fields=fields)
        f = lines[1].split("\t")
        assert f[3] == str(2000 + 5 + 1) and f[5] == "5S145=" and f[11:] == ["NM:i:0", "MD:Z:145", "AS:i:143"]
        e = entry_of(pl, sc, 10)                               # the deletion of 12 letters
        f = lines[10].split("\t")
        assert f[5] == want["strings"][e] and f[5].count("D") == 1 and f[13] == f"AS:i:{int(want['score'][e])}" and f[11] == f"NM:i:{int(want['nm'][e])}"
        assert f[5] != plain[5].strings()[entry_of(plain[3], plain[4], 10)] and int(want["score"][e]) > int(plain[5].host()[0][e])
        # pairs with a rescue and supplementaries: the placements' clips and the all-loci clips are realigned, the rescue's stay trimmed
        name = "dna4_k10"
        sigma, k, n = PAIR_WORKLOADS[name]
        txt = text_of(sigma, n)
        idx2 = engine.Index(txt, sigma, [k], table=2)
        held.append(idx2)
        ranks, roff = rescue_pairs_of(name)
        mates = (ranks[:int(roff[32])], roff[:33])
        kw = dict(PAIR_CHAIN, **INSERT)
        with pytest.raises(ValueError):
            idx2.map_pairs(*mates, k, COMP4, **kw, scripts=True, realign={})
        base = idx2.map_pairs(*mates, k, COMP4, **kw, scripts=True, rescue=True, clip=dict(clip_penalty=0), supplementary={})
        held += list(base)
        got = idx2.map_pairs(*mates, k, COMP4, **kw, scripts=True, rescue=True, clip=dict(clip_penalty=0), supplementary={}, realign={})
        held += list(got)
        names = ["StrandReads", "Loci", "Alignments", "Placements", "Pairs", "Scripts", "Rescues", "Clips", "Clips", "Supplementaries"]
        assert [type(h).__name__ for h in got] == names == [type(h).__name__ for h in base]
        rd, loci, al, pl, pairs, sc, res, cl, rcl, sup = got
        for g, w in zip(pl.host(), base[3].host()):
            assert np.array_equal(g, w)
        same(SCRIPTS, sc.host(), base[5].host())
        ranks2, roff2 = doubled(rd)
        check_realign(cl, sc, oracle(sc, al, ranks2, roff2, txt, clip_penalty=0))
        check_clips(rcl, rcl.scripts, clip_penalty=0)
        same(CLIPS, rcl.host(), base[8].host())
        assert rcl.counts()["n_sel"] == res.counts()["n_taken"] == 4
        check_realign(sup.all_clips, sup.all_scripts, oracle(sup.all_scripts, al, ranks2, roff2, txt, clip_penalty=0))
        check_supp(sup, rd, al, pl, sup.all_scripts, sup.all_clips)
        check_clips(base[9].all_clips, base[9].all_scripts, clip_penalty=0)
    finally:
        close_all(held)


# ---- 7. an entry that stays whole is the same entry in the trimmer and in the realignment ------------------------------------------------
def short_reads():
    """(64 reads of 40 .. 80 letters from random places with 0 .. 3 edits and one with a letter outside the alphabet, the first read
    without an edit)"""
    t = text()
    z = synth.u64_stream(913, 16 * 64).astype(np.int64) & 0x7FFFFFFF
    reads, edits = [], []
    for p in range(64):
        zz = z[16 * p:16 * p + 16]
        s = 1000 + int(zz[0] % 17_000)
        edits.append(int(zz[1] % 4))
        reads.append(edited(zz[2:], t[s:s + 40 + p % 41], edits[-1]))
    foreign = t[3000:3060].copy()
    foreign[30] = 4
    return reads + [foreign], edits.index(0)


def test_a_floor_nothing_meets_leaves_the_same_whole_entries_in_both_calls(engine, index):
    reads, x = short_reads()
    ranks, roff = pack(reads)
    floor = 2 ** 31 - 1
    held = list(index.map_reads(ranks, roff, K, **CHAIN))
    try:
        loci, al = held
        # the scripts of other letters in read x than were aligned: its entries are mismatched and have no runs
        swapped = ranks.copy()
        swapped[int(roff[x]):int(roff[x + 1])] = other(swapped[int(roff[x]):int(roff[x + 1])])
        sc = al.scripts(index, loci, swapped, roff, all=True)
        held.append(sc)
        read_sel_off, sel, cig_off, cigar = sc.host()
        runs = np.diff(cig_off.astype(np.int64))
        of_read = lambda r: slice(int(read_sel_off[r]), int(read_sel_off[r + 1]))
        assert sel.size >= 50 and runs[of_read(x)].size >= 1 and not runs[of_read(x)].any() and sc.counts()["n_mismatched"] >= 1
        assert runs[of_read(64)].size >= 1 and runs[of_read(64)].min() >= 3                    # '=', an X at the foreign letter, '='
        trimmed = sc.clip(min_score=floor)
        held.append(trimmed)
        again = sc.realign(index, al, swapped, roff, min_score=floor)
        held.append(again)
        got, want = again.host(), trimmed.host()
        for name, g, w in zip(CLIPS, got, want):
            assert g.dtype == w.dtype and g.tobytes() == w.tobytes(), name
        assert again.counts() == trimmed.counts() == dict(n_sel=sel.size, n_ops=cigar.size, n_clipped=0, n_low=sel.size)
        # ... and what the oracle says (tests/realign_naive.py takes a whole entry from tests/clip_naive.py): the script, whole
        check_clips(trimmed, sc, min_score=floor)
        assert np.array_equal(got[7], cig_off) and np.array_equal(got[8], cigar) and (got[6] == engine.CLIP_LOW).all()
    finally:
        close_all(held)
