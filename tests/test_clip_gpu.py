"""Soft clipping on the GPU: kmx_scripts_clip, kmx_clips_md, kmx_clips_rescues_md, Secondaries.xa(clips=) and the `clip=` keyword of
the chain calls.  The oracle is always tests/clip_naive.py on the host views of the engine's own scripts; every array, its dtype and
every counter must be identical.  The planted reads say what the batch must hold.  Nothing is larger than the shapes of the other
chain tests.  Untested: an index with several replicas, and the different-devices refusals."""
import ctypes as C

import numpy as np
import pytest

from tests import clip_naive as cn
from tests.chain_checks import check_clip_md, check_clips, close_all, entry_of, refused, same
from tests.chain_data import (CHAIN as PAIR_CHAIN, CLIP_CHAIN as CHAIN, CLIP_PLANTED as PLANTED, CLIP_SIZES as SIZES, CLIPS, COMP4, INSERT, K,
                              LETTERS4 as LETTERS, M, MD, PAIR_WORKLOADS, REPEAT_CHAIN, SCRIPTS, clip_planted_reads as planted_reads, clip_text as text,
                              other, rc4, repeat_text, rescue_pairs_of, text_of)
from tests.helpers import pack

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def index(engine):
    idx = engine.Index(text(), 4, [K], table=2)
    yield idx
    idx.close()


@pytest.fixture(scope="module")
def mapped(index):
    out = index.map_reads_strands(*pack(planted_reads()), K, COMP4, **CHAIN, scripts=True)
    yield out
    close_all(list(out))


# ---- 1. the planted reads -----------------------------------------------------------------------------------------------------------------
def test_planted_reads_equal_the_oracle_at_three_settings_and_leave_the_scripts_alone(engine, index, mapped):
    reads, loci, al, pl, sc = mapped
    before = (sc.host(), sc.device_ptrs(), sc.counts())
    at = {name: i for i, name in enumerate(PLANTED)}
    strand = pl.host(best2=False)[1]
    # a read of letters outside the alphabet has no window and stays unplaced here; its script mI is made further down, by aligning
    # blanked reads at the loci of the real ones
    assert strand[at["outside"]] == 255 and strand[at["tail_reverse"]] == 1 and (strand[:6] != 255).all()
    held = []
    try:
        cl = sc.clip()
        held.append(cl)
        five = check_clips(cl, sc)
        ent = {name: entry_of(pl, sc, at[name]) for name in PLANTED[:6]}
        field = lambda out, name: (out["strings"][ent[name]], int(out["score"][ent[name]]), int(out["sl"][ent[name]]), int(out["sr"][ent[name]]),
                                   int(out["tl"][ent[name]]), int(out["tr"][ent[name]]), int(out["nm"][ent[name]]), int(out["cflags"][ent[name]]))
        assert field(five, "unedited") == ("150=", 150, 0, 0, 0, 0, 0, 0)
        # the largest-start / smallest-end rule of the aligner makes insertions of edits at a read's end: '1I2=2I145=' here, so that
        # two text letters go with the five read letters; 11 and 8 text letters with the 12 of the tails
        assert field(five, "three_subs") == ("5S145=", 140, 5, 0, 2, 0, 0, 0)
        assert field(five, "tail") == ("138=12S", 133, 0, 12, 0, 11, 0, 0)
        assert field(five, "tail_reverse") == ("138=12S", 133, 0, 12, 0, 8, 0, 0)
        assert field(five, "over_end") == ("140=10S", 135, 0, 10, 0, 0, 0, 0)                 # the overhang: no text letter goes
        assert field(five, "over_start") == ("10S140=", 135, 10, 0, 0, 0, 0, 0)
        assert five["n_low"] == 0 and five["n_clipped"] == 5
        # MD of the clipped entries, over [start + tl, end - tr)
        md = cl.md(index, sc, al, LETTERS)
        held.append(md)
        _, start, end = al.host()[:3]
        strings = check_clip_md(md, five, start, end, text())
        assert md.counts()["n_mismatched"] == 0
        assert [strings[ent[name]] for name in PLANTED[:6]] == ["150", "145", "138", "138", "140", "140"]
        plain = sc.md(index, al, LETTERS)
        held.append(plain)
        assert len(plain.strings()[ent["tail"]]) > 3 and plain.strings()[ent["unedited"]] == "150"
        # per read: where the CIGARs are
        tl, nm, score, has = pl.clip_fields(cl, sc)
        assert has.tolist() == [s != 255 for s in strand] and (tl[at["three_subs"]], nm[at["three_subs"]], score[at["three_subs"]]) == (2, 0, 140)
        # p = 0 through the same handle: every terminal mismatch goes; a floor that flips entries to LOW
        assert sc.clip(clip_penalty=0, clips=cl) is cl
        zero = check_clips(cl, sc, clip_penalty=0)
        assert zero["n_clipped"] > five["n_clipped"] and field(zero, "three_subs") == ("5S145=", 145, 5, 0, 2, 0, 0, 0)
        sc.clip(min_score=134, clips=cl)
        low = check_clips(cl, sc, min_score=134)
        assert field(low, "tail")[-1] == cn.LOW and field(low, "tail")[:2] == (sc.strings()[ent["tail"]], int(low["score"][ent["tail"]]))
        assert field(low, "over_end") == field(five, "over_end") and 0 < low["n_low"] < low["sel"].size
        assert int(low["score"][ent["tail"]]) == 117           # the score of the whole script, '138=1I3X1=2X5=', not of the part
        # the scripts are untouched
        after = (sc.host(), sc.device_ptrs(), sc.counts())
        assert before[1:] == after[1:]
        same(SCRIPTS, after[0], before[0])
    finally:
        close_all(held)


def test_an_overhang_across_a_junction_is_clipped_under_a_contig_table(engine):
    t = text()
    reads = [t[7000 - 140:7000 + 10].copy(), rc4(t[12_000 - 10:12_000 + 140]), t[8000:8000 + M].copy()]
    idx = engine.Index(t, 4, [K], table=2)
    held = [idx]
    try:
        idx.set_contigs(np.concatenate([[0], np.cumsum(SIZES)]).astype(np.uint64))
        out = idx.map_reads_strands(*pack(reads), K, COMP4, **CHAIN, scripts=True, clip={})
        held += list(out)
        reads_h, loci, al, pl, sc, cl = out
        assert isinstance(cl, engine.Clips) and cl.scripts is sc
        want = check_clips(cl, sc)
        got = [want["strings"][entry_of(pl, sc, i)] for i in range(3)]
        # (three of the letters beyond the junction fit the script of the first read by chance: '137=1I2=6I1=3I' is what is trimmed)
        assert got == ["137=13S", "10S140=", "150="] and want["n_clipped"] == 2
        loc = pl.locate(idx, al)
        held.append(loc)
        tl = pl.clip_fields(cl, sc)[0]
        # the first read ends at its contig's end; the second starts at its contig's start, its clip takes no text letter
        assert tl.tolist() == [0, 0, 0] and loc.host()[0].tolist() == [0, 2, 1] and loc.host()[1].tolist() == [7000 - 140, 0, 1000]
    finally:
        close_all(held[1:])
        idx.close()


# ---- 2. a long read with both ends clipped ---------------------------------------------------------------------------------------------
def test_a_read_of_1024_letters_at_250_edits_is_clipped_on_both_sides(engine, index):
    t = text()
    q = t[6000:6000 + 1024].copy()
    q[0:250:2] = other(q[0:250:2])                             # 125 substitutions at either end: 245 edits as the aligner counts them,
    q[1024 - 250::2] = other(q[1024 - 250::2])
    q[300:701:100] = other(q[300:701:100])                     # and five in the middle, which the clipped script keeps
    held = list(index.map_reads_strands(*pack([q]), K, COMP4, band=8, min_votes=2, max_edits=250, max_span=64, scripts=True))
    try:
        reads, loci, al, pl, sc = held
        assert al.host()[0][int(pl.host()[0][0])] == 250 and sc.counts()["n_ops"] >= 400
        cl = sc.clip()
        held.append(cl)
        want = check_clips(cl, sc)
        e = entry_of(pl, sc, 0)
        assert want["strings"][e] == "249S51=1X99=1X99=1X99=1X99=1X73=250S"
        assert (int(want["tl"][e]), int(want["tr"][e]), int(want["nm"][e]), int(want["score"][e])) == (243, 223, 5, 490)
        md = cl.md(index, sc, al, LETTERS)
        held.append(md)
        _, start, end = al.host()[:3]
        assert check_clip_md(md, want, start, end, t)[e] == "51T99T99T99G99G73"
    finally:
        close_all(held)


def test_reads_of_nothing_but_insertions_stay_whole_and_low(engine, index):
    """The reads given to kmx_loci_align and to the scripts hold no letter of the alphabet (the loci are those of the real reads), so
    every entry is the single run mI against the empty substring: no '=' run, hence never clipped, a negative score, and LOW at the
    default floor."""
    ranks, roff = pack(planted_reads()[:6] + [text()[9000:9120].copy()])
    blank = np.full(ranks.size, 255, np.uint8)
    held = [index.vote_windows(ranks, roff, K, 1, 8, 2, 0)]
    try:
        loci = held[0]
        al = loci.align(index, blank, roff, 250, 64)
        held.append(al)
        sc = al.scripts(index, loci, blank, roff, all=True)
        held.append(sc)
        read_sel_off = sc.host()[0]
        m = np.repeat(np.diff(roff.astype(np.int64)), np.diff(read_sel_off.astype(np.int64)))
        assert m.size >= 6 and set(m.tolist()) == {120, 150} and sc.strings() == [f"{x}I" for x in m]
        cl = sc.clip()
        held.append(cl)
        want = check_clips(cl, sc)
        assert want["strings"] == sc.strings() and want["score"].tolist() == (-(6 + m)).tolist() and want["nm"].tolist() == m.tolist()
        assert (want["cflags"] == cn.LOW).all() and want["n_low"] == m.size and want["n_clipped"] == 0
        assert not any(want[k].any() for k in ("sl", "sr", "tl", "tr"))
        # under a floor that they meet, and with clips for free, they still stay whole: there is no '=' run to border a clip
        sc.clip(clip_penalty=0, min_score=-156, clips=cl)
        free = check_clips(cl, sc, clip_penalty=0, min_score=-156)
        assert free["strings"] == sc.strings() and free["n_low"] == free["n_clipped"] == 0 and np.array_equal(free["score"], want["score"])
        sc.clip(min_score=-155, clips=cl)
        assert check_clips(cl, sc, min_score=-155)["cflags"].tolist() == [cn.LOW if x == 150 else 0 for x in m]
        md = cl.md(index, sc, al, LETTERS)
        held.append(md)
        _, start, end = al.host()[:3]
        assert set(check_clip_md(md, want, start, end, text())) == {"0"} and md.counts()["n_mismatched"] == 0
    finally:
        close_all(held)


# ---- 3. every aligned locus, the refusals after looking, no entries, one handle through sizes --------------------------------------------
def test_all_scripts_the_m_refusal_no_entries_and_one_handle_through_sizes(engine, index):
    t = text()
    pool = [x for x in planted_reads() if x.max() < 4]
    ranks, roff = pack(pool[:30])
    held = list(index.map_reads(ranks, roff, K, **CHAIN))
    try:
        loci, al = held
        sc = al.scripts(index, loci, ranks, roff, all=True)
        held.append(sc)
        cl = sc.clip(clip_penalty=2)
        held.append(cl)
        want = check_clips(cl, sc, clip_penalty=2)
        assert sc.counts()["n_sel"] == al.counts()["n_aligned"] >= 15 and want["n_clipped"] >= 3
        md = cl.md(index, sc, al, LETTERS)
        held.append(md)
        _, start, end = al.host()[:3]
        check_clip_md(md, want, start, end, t)
        assert md.counts()["n_mismatched"] == 0
        # '=' and 'X' joined: refused after looking, and the handle then holds an empty result
        joined = al.scripts(index, loci, ranks, roff, m=True)
        held.append(joined)
        assert "KMX_SCRIPT_M" in refused(engine, lambda: joined.clip(clips=cl), "kmx_scripts_clip")
        assert cl.counts() == dict(n_sel=0, n_ops=0, n_clipped=0, n_low=0) and cl.device_ptrs() == (None,) * 9
        h = cl.host()
        assert h[7].tolist() == [0] and all(x.size == 0 for x in h[:7] + h[8:]) and cl.strings() == []
        # a refusal before looking leaves the result
        sc.clip(clips=cl)
        o = engine.ClipOptions(32, 0, 4, 6, 1, 5, 0, 0)
        assert engine.lib().kmx_scripts_clip(sc._h, C.byref(o), None, C.byref(cl._h)) == 1 and cl.counts()["n_sel"] == sc.counts()["n_sel"]
        # no entries: a read without a window; then small / large / small through the one handle
        nothing = list(index.map_reads(*pack([np.full(M, 4, np.uint8)]), K, **CHAIN))
        held += nothing
        empty = nothing[1].scripts(index, nothing[0], *pack([np.full(M, 4, np.uint8)]))
        held.append(empty)
        # clips of other scripts: n_sel differs, and the md handle then holds an empty result
        assert "n_sel differs" in refused(engine, lambda: cl.md(index, empty, nothing[1], LETTERS, md=md), "kmx_clips_md")
        assert md.counts() == dict(n_sel=0, n_bytes=0, n_mismatched=0) and md.host()[0].tolist() == [0] and md.device_ptrs() == (None, None)
        empty.clip(clips=cl)
        assert empty.counts()["n_sel"] == 0 and check_clips(cl, empty)["n_clipped"] == 0 and cl.host()[7].tolist() == [0]
        for n_reads in (2, 30, 1):
            rk, ro = pack(pool[:n_reads])
            lo2, al2 = index.map_reads(rk, ro, K, **CHAIN)
            held += [lo2, al2]
            sc2 = al2.scripts(index, lo2, rk, ro, all=True)
            held.append(sc2)
            sc2.clip(clip_penalty=0, clips=cl)
            check_clips(cl, sc2, clip_penalty=0)
    finally:
        close_all(held)


# ---- 4. the scripts of a rescue and of secondaries ------------------------------------------------------------------------------------------
def test_clips_and_md_of_rescued_mates(engine):
    name = "dna4_k10"
    sigma, k, n = PAIR_WORKLOADS[name]
    txt = text_of(sigma, n)
    idx = engine.Index(txt, sigma, [k], table=2)
    held = []
    try:
        ranks, roff = rescue_pairs_of(name)
        ranks, roff = ranks[:int(roff[80])], roff[:81]          # 40 pairs, 10 of them to rescue
        held += list(idx.map_pairs(ranks, roff, k, COMP4, **PAIR_CHAIN, **INSERT, rescue=True))
        reads, res = held[0], held[5]
        rsc = res.scripts(idx, reads)
        held.append(rsc)
        rcl = rsc.clip(clip_penalty=0)
        held.append(rcl)
        want = check_clips(rcl, rsc, clip_penalty=0)
        # kill() puts a substitution next to the last letter of every rescued mate: at p = 0 that end goes
        assert res.counts()["n_taken"] == rsc.counts()["n_sel"] == 10 and want["n_clipped"] == 10
        rmd = rcl.md(idx, rsc, res, LETTERS)
        held.append(rmd)
        jobs = res.host()
        strings = check_clip_md(rmd, want, jobs[5], jobs[6], txt, bound=jobs[5].size)
        assert rmd.counts()["n_mismatched"] == 0 and all(strings)
        tl, nm, score, has = res.clip_fields(rcl, rsc)
        assert int(has.sum()) == 10 and [bool(c) for c in res.cigars(rsc)] == has.tolist()
        # the wrong source is refused by its n_sel or served harmlessly; the alignments' entry point on the rescue's scripts
        sc = held[3].scripts(idx, reads, held[1], held[2])
        held.append(sc)
        assert "n_sel differs" in refused(engine, lambda: rcl.md(idx, sc, held[2], LETTERS, md=rmd), "kmx_clips_md")
    finally:
        close_all(held)
        idx.close()


def test_clips_of_secondaries_and_their_xa(engine):
    txt, _ = repeat_text()
    idx = engine.Index(txt, 4, [10], table=2)
    held = []
    try:
        unit3 = np.concatenate([txt[2000:2150].copy()])
        reads = [np.concatenate([other(unit3[:4]), unit3[4:100]]), txt[300:380].copy()]
        out = idx.map_reads_strands(*pack(reads), 10, COMP4, **REPEAT_CHAIN, secondaries=4)
        held += list(out)
        reads_h, loci, al, pl, sec = out
        ssc = sec.scripts(idx, reads_h)
        held.append(ssc)
        scl = ssc.clip()
        held.append(scl)
        want = check_clips(scl, ssc)
        assert sec.counts()["n_sec"] == 4 == ssc.counts()["n_sel"] and want["n_clipped"] == 4 and set(want["strings"]) == {"4S96="}
        sec_off, _, dist, start, _, _, _ = sec.host()
        assert (dist > 0).all() and want["nm"].tolist() == [0] * 4 and (want["tl"] <= 4).all() and want["sl"].tolist() == [4] * 4
        old = sec.xa(ssc, rname="chr")
        new = sec.xa(ssc, rname="chr", clips=scl)
        assert new == engine.xa_strings(sec_off, want["nm"], start, None, want["strings"], rname="chr", shift=want["tl"])
        assert old[1] == new[1] == "" and old[0] != new[0]
        first = new[0].split(";")[0].split(",")
        assert first[2:] == ["4S96=", "0"] and int(first[1]) == int(old[0].split(";")[0].split(",")[1]) + int(want["tl"][0])
    finally:
        close_all(held)
        idx.close()


# ---- 5. the chain keyword -------------------------------------------------------------------------------------------------------------------
def test_the_chain_keyword_appends_the_separate_calls(engine, index, mapped):
    reads = pack(planted_reads()[:6] + planted_reads()[7:13])   # (sam_lines refuses a read with a letter outside the alphabet)
    held = []
    try:
        with pytest.raises(ValueError):
            index.map_reads_strands(*reads, K, COMP4, **CHAIN, clip={})
        plain = index.map_reads_strands(*reads, K, COMP4, **CHAIN, scripts=True, tags=True, letters=LETTERS)
        held += list(plain)
        assert len(plain) == 6 and [type(h).__name__ for h in plain[:5]] == ["StrandReads", "Loci", "Alignments", "Placements", "Scripts"]
        out = index.map_reads_strands(*reads, K, COMP4, **CHAIN, scripts=True, tags=True, letters=LETTERS, clip=dict(clip_penalty=2), secondaries=2)
        held += list(out)
        assert len(out) == 8 and isinstance(out[-1], engine.Clips) and isinstance(out[-2], engine.Secondaries) and isinstance(out[5], engine.SamTags)
        same(SCRIPTS, out[4].host(), plain[4].host())
        apart = plain[4].clip(clip_penalty=2)
        held.append(apart)
        same(CLIPS, out[-1].host(), apart.host())
        assert out[-1].counts() == apart.counts() and apart.counts()["n_clipped"] >= 4
        want = check_clips(out[-1], out[4], clip_penalty=2)
        _, start, end = out[2].host()[:3]
        check_clip_md(out[5].md, want, start, end, text())     # with tags the MD is the clipped one
        amd = apart.md(index, plain[4], plain[2], LETTERS)
        held.append(amd)
        same(MD, out[5].md.host(), amd.host())
        assert out[5].md.strings() != plain[5].md.strings()
        # SAM lines from the clipped fields: POS moves by tl, AS follows MD
        pl, sc, cl = out[3], out[4], out[-1]
        fields = pl.clip_fields(cl, sc)
        names = [f"q{i}" for i in range(12)]
        lines = engine.sam_lines(names, *reads, LETTERS, COMP4, 4, "chr", pl.host(best2=False), pl.cigars(sc, cl), pl.mds(out[5].md, sc),
                                 out[5].mapq.host(), clip_fields=fields)
        f = lines[1].split("\t")
        assert f[3] == str(2000 + 5 + 1) and f[5] == "5S145=" and f[11:] == ["NM:i:0", "MD:Z:145", "AS:i:143"]
        # pairs with a rescue and tags: the clips of both scripts come last, and the MDs are the clipped ones
        name = "dna4_k10"
        sigma, k, n = PAIR_WORKLOADS[name]
        idx2 = engine.Index(text_of(sigma, n), sigma, [k], table=2)
        held.append(idx2)
        ranks, roff = rescue_pairs_of(name)
        mates = (ranks[:int(roff[32])], roff[:33])
        kw = dict(PAIR_CHAIN, **INSERT)
        with pytest.raises(ValueError):
            idx2.map_pairs(*mates, k, COMP4, **kw, clip={})
        base = idx2.map_pairs(*mates, k, COMP4, **kw, scripts=True, rescue=True, tags=True, letters=LETTERS)
        held += list(base)
        assert len(base) == 8 and isinstance(base[-1], engine.SamTags) and isinstance(base[6], engine.Rescues)
        got = idx2.map_pairs(*mates, k, COMP4, **kw, scripts=True, rescue=True, tags=True, letters=LETTERS, clip=dict(clip_penalty=0))
        held += list(got)
        assert len(got) == 10 and isinstance(got[-3], engine.SamTags) and isinstance(got[-2], engine.Clips) and isinstance(got[-1], engine.Clips)
        tags, cl, rcl = got[-3:]
        assert cl.scripts is got[5] and rcl.scripts is tags.rescue_scripts
        for g, w in zip(got[3].host(), base[3].host()):
            assert np.array_equal(g, w)
        same(SCRIPTS, got[5].host(), base[5].host())
        w1 = check_clips(cl, got[5], clip_penalty=0)
        w2 = check_clips(rcl, tags.rescue_scripts, clip_penalty=0)
        assert w2["n_clipped"] == rcl.counts()["n_sel"] == got[6].counts()["n_taken"] == 4
        _, start, end = got[2].host()[:3]
        check_clip_md(tags.md, w1, start, end, text_of(sigma, n))
        jobs = got[6].host()
        check_clip_md(tags.rescue_md, w2, jobs[5], jobs[6], text_of(sigma, n))
        assert tags.rescue_md.strings() != base[-1].rescue_md.strings()
        fields = (got[3].clip_fields(cl, got[5]), got[6].clip_fields(rcl, tags.rescue_scripts))
        assert int(fields[1][3].sum()) == 4 and not (fields[0][3] & fields[1][3]).any()   # a rescued read has no script of its own
        cigars = (got[3].cigars(got[5], cl), got[6].cigars(tags.rescue_scripts, rcl))
        mds = (got[3].mds(tags.md, got[5]), got[6].mds(tags.rescue_md, tags.rescue_scripts))
        names = [f"p{i // 2}" for i in range(32)]
        lines = engine.sam_lines(names, *mates, LETTERS, COMP4, 4, "chr", got[3].host(best2=False), cigars, mds, tags.mapq.host(), got[4].host(),
                                 clip_fields=fields)
        i = int(np.flatnonzero(fields[1][3])[0])
        f = lines[i].split("\t")
        assert "S" in f[5] and f[13] == f"AS:i:{int(fields[1][2][i])}" and f[11] == f"NM:i:{int(fields[1][1][i])}"
        assert int(f[3]) == int(got[3].host(best2=False)[3][i]) + int(fields[1][0][i]) + 1
    finally:
        close_all(held)
