"""Supplementary alignments on the GPU: kmx_clips_supplementaries, the SAM side on the engine's own handles and the `supplementary=`
keyword of the chain calls.  The oracle is always tests/supp_naive.py on the host views of the engine's own handles; every array,
its dtype and every counter must be identical, and the device views must equal the host views.  The planted reads, and what
tests/test_supplementary_cpu.py shows about them on the CPU alone, say what the batch must hold.  Nothing is larger than the shapes
of the other chain tests.  Untested: an index with several replicas, the different-devices refusals, and the refusal of an odd
nr2 (a StrandReads never holds one)."""
import numpy as np
import pytest

from tests import chain_naive as ch
from tests import clip_naive as cn
from tests import supp_naive as sp
from tests.chain_checks import (check_clip_md, check_clips, check_supp, close_all, entry_of, refused, same, supp_cpu_chain, supp_oracle,
                                supp_rows as rows)
from tests.chain_data import (CLIPS, COMP4, COPIES, K, LETTERS4 as LETTERS, M, SUPP_CHAIN as CHAIN, SUPP_PLANTED, kill, rc4,
                              supp_planted_reads, supp_text)
from tests.helpers import pack

pytestmark = pytest.mark.gpu

EMPTY = dict(nr=0, n_sup=0, n_split=0, n_truncated=0)


@pytest.fixture(scope="module")
def index(engine):
    idx = engine.Index(supp_text(), 4, [K], table=2)
    yield idx
    idx.close()


@pytest.fixture(scope="module")
def mapped(index):
    """the planted batch through the chain with the keyword: (reads, loci, al, pl, sc, tags, cl, sup)"""
    out = index.map_reads_strands(*pack(supp_planted_reads()), K, COMP4, **CHAIN, scripts=True, tags=True, letters=LETTERS, clip={}, supplementary={})
    yield out
    close_all(list(out))


# ---- 1. the planted reads -----------------------------------------------------------------------------------------------------------------
def test_planted_reads_equal_the_oracle_and_the_cpu_chain(engine, mapped):
    reads, loci, al, pl, sc, tags, cl, sup = mapped
    assert isinstance(sup, engine.Supplementaries) and isinstance(sup.all_scripts, engine.Scripts) and isinstance(sup.all_clips, engine.Clips)
    asc, acl = sup.all_scripts, sup.all_clips
    assert asc.counts()["n_sel"] == al.counts()["n_aligned"] == acl.counts()["n_sel"] and asc.counts()["nr"] == 2 * len(supp_planted_reads())
    check_clips(acl, asc)
    want = check_supp(sup, reads, al, pl, asc, acl)
    # what the CPU chain alone gave for these reads (tests/test_supplementary_cpu.py asserts the per-read figures on it)
    cpu = supp_oracle(supp_cpu_chain())
    for name in sp.ARRAYS[:11] + ("more",) + sp.COUNTERS:
        assert np.array_equal(want[name], cpu[name]), name
    at = {name: i for i, name in enumerate(SUPP_PLANTED)}
    assert rows(want, at["split"]) and rows(want, at["split_rc"])[0][1] == 1 and rows(want, at["split_rc_whole"])[0][1] == 0
    assert len(rows(want, at["three"])) == 2 and rows(want, at["many"])[0][6] == rows(want, at["many"])[0][7] and want["n_sup"] == 8
    assert asc.host()[0][2 * at["many"] + 2] - asc.host()[0][2 * at["many"]] == 2 * COPIES > 64
    x = int(want["sup_off"][at["dup"]])
    assert sup.mapq()[x] == 0 and sup.mapq().tolist() == sp.mapq(want["score"], want["second_score"]) and sup.mapq().dtype == np.uint8
    assert sup.cigars() == [cn.strings(acl.host()[7], acl.host()[8])[int(e)] for e in want["ent"]]
    assert sup.cigars()[int(want["sup_off"][at["split"]])] == "100S50="


def test_the_primary_has_the_same_clip_among_all_loci_as_among_the_winners(mapped):
    reads, loci, al, pl, sc, tags, cl, sup = mapped
    asc, acl = sup.all_scripts, sup.all_clips
    locus, strand = pl.host(best2=False)[:2]
    read_sel_off, sel = asc.host()[:2]
    all_strings, own_strings = acl.strings(), cl.strings()
    all_h, own_h = acl.host(), cl.host()
    n = 0
    for i, (l, s) in enumerate(zip(locus, strand)):
        if s == 255 or l == 0xFFFFFFFF:
            continue
        p = [e for e in range(int(read_sel_off[2 * i]), int(read_sel_off[2 * i + 2])) if sel[e] == l]
        e = entry_of(pl, sc, i)
        assert len(p) == 1 and all_strings[p[0]] == own_strings[e] != ""
        assert all_h[3][p[0]] == own_h[3][e] and all_h[0][p[0]] == own_h[0][e]                 # tl, score
        n += 1
    assert n == len(supp_planted_reads()) - 1                    # every read but the one without a letter of the alphabet


# ---- 2. the batch four times over ------------------------------------------------------------------------------------------------------------
def test_four_copies_of_the_batch_give_four_copies_of_the_result(index, mapped):
    base = mapped[-1]
    R = 4
    ranks, roff = pack(supp_planted_reads())
    out = index.map_reads_strands(*ch.tile_reads(ranks, roff, R), K, COMP4, **CHAIN, scripts=True, clip={}, supplementary={})
    try:
        reads, loci, al, pl, sc, cl, sup = out
        nr = len(supp_planted_reads())
        assert sup.counts()["nr"] == R * nr > 64 and 2 * R * nr < 8193
        check_supp(sup, reads, al, pl, sup.all_scripts, sup.all_clips)
        b, g = base.host(), sup.host()
        per = dict(ent=base.all_scripts.counts()["n_sel"], locus=mapped[1].counts()["n_loci"])
        for name, x, y in zip(sp.ARRAYS, b, g):
            if name == "sup_off":
                w = ch._tile_off(x, R)
            elif name in per:
                w = (np.tile(x.astype(np.int64), R) + np.repeat(np.arange(R) * per[name], x.size)).astype(x.dtype)
            elif name == "ctg":
                assert x is None and y is None
                continue
            else:
                w = np.tile(x, R)
            same((name,), (y,), (w,))
        assert sup.counts() == {k: R * v for k, v in base.counts().items()}
    finally:
        close_all(list(out))


# ---- 3. no reads, no loci, one handle through options ---------------------------------------------------------------------------------------
def test_an_empty_batch_and_a_batch_without_a_locus(engine, index):
    held = []
    try:
        out = index.map_reads_strands(*pack([]), K, COMP4, **CHAIN, scripts=True, clip={}, supplementary={})
        held += list(out)
        sup = out[-1]
        assert sup.counts() == EMPTY and sup.host()[0].tolist() == [0] and sup.host()[11] is None
        assert all(x.size == 0 for x in sup.host()[1:11] + sup.host()[12:])
        assert sup.device_ptrs()[0] is not None and sup.device_ptrs()[1:] == (None,) * 12
        check_supp(sup, out[0], out[2], out[3], sup.all_scripts, sup.all_clips)
        out = index.map_reads_strands(*pack([np.full(M, 4, np.uint8)] * 3), K, COMP4, **CHAIN, scripts=True, clip={}, supplementary={})
        held += list(out)
        sup = out[-1]
        assert out[1].counts()["n_loci"] == 0 and sup.counts() == dict(EMPTY, nr=3)
        assert sup.host()[0].tolist() == [0, 0, 0, 0] and sup.host()[12].tolist() == [0, 0, 0] and sup.device_ptrs()[12] is not None
        check_supp(sup, out[0], out[2], out[3], sup.all_scripts, sup.all_clips)
    finally:
        close_all(held)


def test_one_handle_through_other_options_ends_the_earlier_views(engine, mapped):
    reads, loci, al, pl, sc, tags, cl, base = mapped
    asc, acl = base.all_scripts, base.all_clips
    at = {name: i for i, name in enumerate(SUPP_PLANTED)}
    sup = engine.Supplementaries()
    try:
        assert acl.supplementaries(reads, loci, al, pl, asc, supplementaries=sup) is sup and sup.all_clips is acl
        first = check_supp(sup, reads, al, pl, asc, acl)
        # N = 1: the read of three parts keeps one and reports more
        acl.supplementaries(reads, loci, al, pl, asc, max_supplementary=1, supplementaries=sup)
        one = check_supp(sup, reads, al, pl, asc, acl, max_supplementary=1)
        assert one["more"][at["three"]] == 1 and len(rows(one, at["three"])) == 1 and sup.counts()["n_truncated"] == 1 and first["n_truncated"] == 0
        # a low floor for the length and the score, and no overlap allowed
        opt = dict(max_supplementary=8, min_len=10, max_overlap=0, min_score=5)
        acl.supplementaries(reads, loci, al, pl, asc, **opt, supplementaries=sup)
        low = check_supp(sup, reads, al, pl, asc, acl, **opt)
        assert low["n_sup"] != first["n_sup"] and rows(low, at["dup"]) == []          # (its second part shares a letter with the primary)
        acl.supplementaries(reads, loci, al, pl, asc, max_overlap=0xFFFFFFFF, supplementaries=sup)
        check_supp(sup, reads, al, pl, asc, acl, max_overlap=0xFFFFFFFF)
        sup.close()
        assert asc.counts()["n_sel"] and acl.counts()["n_sel"]      # a handle of Clips.supplementaries closes neither
    finally:
        sup.close()


# ---- 4. pairs with a rescue: the SAM lines -----------------------------------------------------------------------------------------------------
def test_pairs_with_a_rescue_and_their_sam_lines(engine, index):
    t, cat = supp_text(), np.concatenate
    mates = [cat([t[2000:2100], t[5000:5050]]), rc4(t[2300:2450]),               # a split mate 1, its mate 2 concordant with the primary
             t[1000:1150].copy(), kill(rc4(t[1300:1450]), K),                  # mate 2 has no intact window: rescued
             t[6700:6850].copy(), rc4(cat([t[7000:7100], rc4(t[7030:7080])])),    # mate 2 split, its primary on the reverse strand
             t[8200:8350].copy(), rc4(t[8500:8650])]                              # an ordinary pair
    ranks, roff = pack(mates)
    # (three votes: at two, chance hits of the broken mate's windows make loci, and within 110 edits any locus is aligned)
    kw = dict(CHAIN, min_votes=3, min_insert=100, max_insert=600)
    held = []
    try:
        base = index.map_pairs(ranks, roff, K, COMP4, **kw, scripts=True, rescue=True, tags=True, letters=LETTERS, clip={})
        held += list(base)
        out = index.map_pairs(ranks, roff, K, COMP4, **kw, scripts=True, rescue=True, tags=True, letters=LETTERS, clip={}, supplementary={})
        held += list(out)
        assert len(out) == len(base) + 1 == 11 and isinstance(out[-1], engine.Supplementaries)
        reads, loci, al, pl, pairs, sc, res, tags, cl, rcl, sup = out
        asc, acl = sup.all_scripts, sup.all_clips
        want = check_supp(sup, reads, al, pl, asc, acl)
        locus = pl.host(best2=False)[0]
        assert res.counts()["n_taken"] == 1 and locus[3] == 0xFFFFFFFF and rows(want, 3) == []     # the rescued mate has no entries
        assert [len(rows(want, i)) for i in range(8)] == [1, 0, 0, 0, 0, 1, 0, 0]
        assert rows(want, 0)[0][1:6] == (0, 100, 150, 5000, 5050) and rows(want, 5)[0][1:6] == (0, 0, 50, 7030, 7080)
        # the primary lines with SA, then the supplementary lines, against strings built from the oracle's arrays
        fields = (pl.clip_fields(cl, sc), res.clip_fields(rcl, tags.rescue_scripts))
        cigars = (pl.cigars(sc, cl), res.cigars(tags.rescue_scripts, rcl))
        mds = (pl.mds(tags.md, sc), res.mds(tags.rescue_md, tags.rescue_scripts))
        names = [f"p{i // 2}" for i in range(8)]
        args = (names, ranks, roff, LETTERS, COMP4, 4, "chr", pl.host(best2=False), cigars, mds, tags.mapq.host(), pairs.host())
        plain = engine.sam_lines(*args, clip_fields=fields)
        assert engine.sam_lines(*args, clip_fields=fields, sa=None) == plain
        tl, nm = (np.where(fields[0][3], a, b) for a, b in zip(fields[0][:2], fields[1][:2]))
        sa = sup.sa(pl.host(best2=False), engine._first_given(cigars), (tl, nm), tags.mapq.host(), rname="chr")
        lines = engine.sam_lines(*args, clip_fields=fields, sa=sa)
        clip_strings = cn.strings(acl.host()[7], acl.host()[8])
        q = sp.mapq(want["score"], want["second_score"])
        rec = lambda x: f"chr,{int(want['t0'][x]) + 1},{'+-'[int(want['strand'][x])]},{clip_strings[int(want['ent'][x])]},{q[x]},{int(want['nm'][x])};"
        for i in range(8):
            f = plain[i].split("\t")
            if not rows(want, i):
                assert lines[i] == plain[i] and sa[i] == [""]
                continue
            x = int(want["sup_off"][i])
            first = f"chr,{f[3]},{'-' if int(f[1]) & 0x10 else '+'},{f[5]},{f[4]},{f[11][5:]};"
            assert lines[i] == plain[i] + "\tSA:Z:" + rec(x) and sa[i] == [rec(x), first]
        assert lines[0].split("\t")[5] == "100=50S" and sa[0][0] == "chr,5001,+,100S50=,60,0;" and sa[0][1].startswith("chr,2001,+,100=50S,")
        amd = acl.md(index, asc, al, LETTERS)
        held.append(amd)
        _, start, end = al.host()[:3]
        md_strings = check_clip_md(amd, check_clips(acl, asc), start, end, t)
        got = engine.sam_supplementary_lines(lines, ranks, roff, LETTERS, COMP4, 4, sup.host(), sup.cigars(), sup.mds(amd), sup.mapq(), sa, rname="chr")
        expect = []
        for i in (0, 5):
            x = int(want["sup_off"][i])
            f = lines[i].split("\t")
            flag = 0x800 | (0x10 if want["strand"][x] else 0) | (int(f[1]) & 0xE9)
            seq = mates[i] if want["strand"][x] == 0 else rc4(mates[i])
            e = int(want["ent"][x])
            expect.append("\t".join([f[0], str(flag), "chr", str(int(want["t0"][x]) + 1), str(q[x]), clip_strings[e], f[6], f[7], "0",
                                     "".join(LETTERS[int(v)] for v in seq), "*", f"NM:i:{int(want['nm'][x])}", f"MD:Z:{md_strings[e]}",
                                     f"AS:i:{int(want['score'][x])}", f"SA:Z:{sa[i][1]}"]))
        assert got == expect
        f0, f5 = got[0].split("\t"), got[1].split("\t")
        assert f0[:9] == ["p0", str(0x800 | 0x1 | 0x20 | 0x40), "chr", "5001", "60", "100S50=", "=", lines[0].split("\t")[7], "0"]
        assert f0[11:14] == ["NM:i:0", "MD:Z:50", "AS:i:45"] and int(f5[1]) & 0x810 == 0x800 and int(f5[1]) & 0x80 and not int(f5[1]) & 0x2
        assert f5[5] == "50=100S" and f5[3] == "7031"
        # the placements are those of the chain without the keyword
        for g, w in zip(pl.host(), base[3].host()):
            assert np.array_equal(g, w)
    finally:
        close_all(held)


# ---- 5. a contig table ---------------------------------------------------------------------------------------------------------------------------
def test_under_a_contig_table_the_entries_carry_their_contig(engine):
    t = supp_text()
    at = {name: i for i, name in enumerate(SUPP_PLANTED)}
    pick = ("plain", "split", "split_rc", "dup")
    reads_in = [supp_planted_reads()[at[n]] for n in pick]
    ctg_off = np.asarray([0, 4000, 12_000, 20_000], np.uint64)
    names = ("c0", "c1", "c2")
    idx = engine.Index(t, 4, [K], table=2)
    held = []
    try:
        idx.set_contigs(ctg_off)
        out = idx.map_reads_strands(*pack(reads_in), K, COMP4, **CHAIN, scripts=True, tags=True, letters=LETTERS, clip={}, supplementary={})
        held += list(out)
        reads, loci, al, pl, sc, tags, cl, sup = out
        want = check_supp(sup, reads, al, pl, sup.all_scripts, sup.all_clips)
        ctg = sup.host()[11]
        assert ctg is not None and ctg.dtype == np.uint32 and np.array_equal(ctg, al.contigs_host()[sup.host()[2]]) and ctg.tolist() == [1, 1, 1]
        assert [len(rows(want, i)) for i in range(4)] == [0, 1, 1, 1]
        loc = pl.locate(idx, al)
        held.append(loc)
        sa = sup.sa(pl.host(best2=False), pl.cigars(sc, cl), pl.clip_fields(cl, sc), tags.mapq.host(), located=(names, ctg_off), located_host=loc.host())
        assert sa[0] == [""] and sa[1][0] == "c1,1001,+,100S50=,60,0;" and sa[1][1].startswith("c0,2001,+,100=50S,")
        assert sa[2][0] == "c1,1501,-,50=100S,60,0;" and sa[3][0] == "c1,5000,+,99S51=,0,0;"
        with pytest.raises(ValueError):
            sup.sa(pl.host(best2=False), pl.cigars(sc, cl), pl.clip_fields(cl, sc), tags.mapq.host(), located=(names, ctg_off))
    finally:
        close_all(held)
        idx.close()


# ---- 6. the refusals after looking, the chain keyword -----------------------------------------------------------------------------------------
def test_refusals_after_looking_leave_an_empty_result(engine, index, mapped):
    reads, loci, al, pl, sc, tags, cl, base = mapped
    asc, acl = base.all_scripts, base.all_clips
    d_ranks2, d_roff2, nr2, stream = reads.device_ptrs()
    held = []
    try:
        other = index.map_reads_strands(*pack(supp_planted_reads()[:3]), K, COMP4, **CHAIN, scripts=True, clip={}, supplementary={})
        held += list(other)
        o_reads, o_loci, o_al, o_pl, o_sc, o_cl, o_sup = other
        # the same reads under another vote: as many reads, other loci
        again = index.map_reads_strands(*pack(supp_planted_reads()), K, COMP4, **dict(CHAIN, min_votes=8))
        held += list(again)
        assert again[1].counts()["n_loci"] != loci.counts()["n_loci"] and again[1].counts()["nr"] == loci.counts()["nr"]
        joined = al.scripts_device(index, loci, d_ranks2, d_roff2, nr2, all=True, m=True, stream=stream)
        held.append(joined)
        assert joined.counts()["n_sel"] == asc.counts()["n_sel"]
        sup = engine.Supplementaries()
        held.append(sup)
        cases = ((lambda: acl.supplementaries(reads, loci, al, o_pl, asc, supplementaries=sup), "the placements are not those of these reads"),
                 (lambda: acl.supplementaries(reads, o_loci, al, pl, asc, supplementaries=sup), "the loci handle's nr differs"),
                 (lambda: acl.supplementaries(reads, loci, o_al, pl, asc, supplementaries=sup), "the alignments handle's nr differs"),
                 (lambda: acl.supplementaries(o_reads, loci, al, pl, asc, supplementaries=sup), "the loci handle's nr differs"),
                 (lambda: acl.supplementaries(reads, loci, again[2], pl, asc, supplementaries=sup), "the alignments handle's n_loci differs"),
                 (lambda: acl.supplementaries(reads, loci, al, pl, o_sup.all_scripts, supplementaries=sup), "the scripts are not those of these reads"),
                 (lambda: acl.supplementaries(reads, loci, al, pl, joined, supplementaries=sup), "KMX_SCRIPT_M"),
                 (lambda: cl.supplementaries(reads, loci, al, pl, asc, supplementaries=sup), "n_sel differs"))
        for call, word in cases:
            acl.supplementaries(reads, loci, al, pl, asc, supplementaries=sup)
            assert sup.counts()["n_sup"] == 8 and sup.device_ptrs()[0] is not None
            assert word in refused(engine, call, "kmx_clips_supplementaries")
            assert sup.counts() == EMPTY and sup.device_ptrs() == (None,) * 13
            h = sup.host()
            assert h[0].tolist() == [0] and h[11] is None and all(x.size == 0 for x in h[1:11] + h[12:])
        # a refusal before looking leaves the result
        acl.supplementaries(reads, loci, al, pl, asc, supplementaries=sup)
        with pytest.raises(engine.KmxError):
            acl.supplementaries(reads, loci, al, pl, asc, max_supplementary=9, supplementaries=sup)
        assert sup.counts()["n_sup"] == 8
        # scripts of the winners alone (no KMX_SCRIPT_ALL) and their clips: served, without a candidate
        cl.supplementaries(reads, loci, al, pl, sc, supplementaries=sup)
        assert check_supp(sup, reads, al, pl, sc, cl)["n_sup"] == 0
    finally:
        close_all(held)


def test_the_chain_keyword_appends_the_separate_calls(engine, index, mapped):
    reads, loci, al, pl, sc, tags, cl, sup = mapped
    ranks, roff = pack(supp_planted_reads())
    held = []
    try:
        for kw in (dict(supplementary={}), dict(scripts=True, supplementary={}), dict(clip={}, supplementary={})):
            with pytest.raises(ValueError):
                index.map_reads_strands(ranks, roff, K, COMP4, **CHAIN, **kw)
        with pytest.raises(ValueError):
            index.map_pairs(ranks, roff, K, COMP4, 100, 600, **CHAIN, scripts=True, supplementary={})
        plain = index.map_reads_strands(ranks, roff, K, COMP4, **CHAIN, scripts=True, tags=True, letters=LETTERS, clip={})
        held += list(plain)
        assert len(plain) == 7 == len(mapped) - 1 and isinstance(plain[-1], engine.Clips)
        assert [type(h).__name__ for h in mapped] == [type(h).__name__ for h in plain] + ["Supplementaries"]
        p_reads, p_loci, p_al, p_pl = plain[:4]
        d_ranks2, d_roff2, nr2, stream = p_reads.device_ptrs()
        asc = p_al.scripts_device(index, p_loci, d_ranks2, d_roff2, nr2, all=True, stream=stream)
        held.append(asc)
        acl = asc.clip(stream=stream)
        held.append(acl)
        apart = acl.supplementaries(p_reads, p_loci, p_al, p_pl, asc, stream=stream)
        held.append(apart)
        for name, g, w in zip(sp.ARRAYS, sup.host(), apart.host()):
            assert (g is None and w is None) or (g.dtype == w.dtype and np.array_equal(g, w)), name
        assert sup.counts() == apart.counts() and apart.counts()["n_sup"] == 8
        same(CLIPS, sup.all_clips.host(), acl.host())
        # other arguments, and other clip scoring, through the keyword
        opt = dict(max_supplementary=1, min_len=30)
        out = index.map_reads_strands(ranks, roff, K, COMP4, **CHAIN, scripts=True, clip=dict(clip_penalty=2), supplementary=opt)
        held += list(out)
        assert len(out) == 7
        check_clips(out[-1].all_clips, out[-1].all_scripts, clip_penalty=2)
        check_supp(out[-1], out[0], out[2], out[3], out[-1].all_scripts, out[-1].all_clips, **opt)
        # the handle of the chain closes the two it was made from
        a, b = out[-1].all_scripts, out[-1].all_clips
        out[-1].close()
        assert not a._h and not b._h and out[-1].all_scripts is None and out[-1].all_clips is None
    finally:
        close_all(held)
