"""The contig table on the GPU (KMX_MAP_CONTIGS): kmx_index_set_contigs, the clamped windows of kmx_loci_align, the contig rule of
kmx_alignments_fold_pairs, the clamped jobs of kmx_pairs_rescue, kmx_placements_locate and engine.sam_lines over contigs.  The oracle
is always tests/contig_naive.py applied to the engine's own host views of the loci and alignments (the pattern of
tests/chain_checks.check_pairs); every array and every counter must be bit-identical.  Texts have at most 50 000 letters and batches at most
300 pairs.  Untested: an index with more than one replica (more than one device)."""
import functools
import re

import numpy as np
import pytest

from kmer_index_amd import synth
from tests import align_naive as an
from tests import contig_naive as cn
from tests import fold_naive as fn
from tests import md_naive as mn
from tests import pair_naive as pn
from tests import rescue_naive as rn
from tests.chain_checks import close_all, counters_of, dev_array, same, spell
from tests.chain_data import (ALIGN as ALIGN5, CHAIN, COMPLEMENT, INSERT, JOBS, LETTERS, PAIRS, PAIR_SIZES, PAIR_WORKLOADS as WORKLOADS, PLACEMENTS, kill,
                              pair_text, rc, rescue_pairs_of, table_of, text_of)
from tests.helpers import pack

pytestmark = pytest.mark.gpu

ALIGN = ALIGN5 + ("ctg",)
E = CHAIN["max_edits"]
NO, NC = pn.NO_BEST, cn.NO_CONTIG
PER = {4: 32, 20: 8}                                           # letters per word of the packed text


def comp_of(sigma):
    return np.asarray(COMPLEMENT[sigma], np.uint8)


def check_align(al, h_loci, text, ctg_off, ranks, roff, sigma, max_edits, max_span):
    """the alignments handle against contig_naive.align on these host loci; returns the oracle's arrays"""
    want = cn.align(text, ctg_off, ranks, roff, h_loci[0], h_loci[1], h_loci[2], max_edits, max_span, sigma)
    got = al.host() + (al.contigs_host(),)
    same(ALIGN, got, want)
    d_ctg, nc = al.contigs_device_ptr()
    assert nc == len(ctg_off) - 1 and np.array_equal(dev_array(d_ctg, want[5].size, np.uint32), want[5])
    c = al.counts()
    assert c["n_aligned"] == int((want[0] <= max_edits).sum()) and c["n_skipped"] == int((want[0] == an.SKIPPED).sum())
    return want


def check_fold(pl, pairs, h_loci, h_al, ctg, min_insert, max_insert, orientation=pn.FR, unpaired_penalty=pn.NO_PENALTY):
    want = cn.fold_pairs(h_loci[0], h_al[0], h_al[1], h_al[2], h_al[3], ctg, min_insert, max_insert, orientation, unpaired_penalty)
    same(PLACEMENTS, pl.host(), want[:7])
    same(PAIRS, pairs.host(), want[7:11])
    assert counters_of(pl, pairs) == want[11]
    return dict(zip(PLACEMENTS + PAIRS, want))


def check_rescue(idx, text, ctg_off, sigma, reads, loci, al, pl, pairs, ranks2, roff2, h_loci, h_al, ctg, min_insert, max_insert, max_edits,
                 orientation=pn.FR, discordant=False, rescues=None):
    """the rescue on these handles against contig_naive.rescue on their state before the call; (Rescues, the oracle's tuple)"""
    want = cn.rescue(text, ctg_off, ctg, sigma, ranks2, roff2, h_loci[0], h_al[0], h_al[1], h_al[2], pl.host(), pairs.host(), min_insert, max_insert,
                     max_edits, orientation, discordant)
    res = pairs.rescue(idx, reads, loci, al, pl, min_insert, max_insert, max_edits, orientation, discordant, rescues=rescues)
    same(PLACEMENTS, pl.host(), want[0])
    same(PAIRS, pairs.host(), want[1])
    same(JOBS, res.host(), want[3])
    assert counters_of(pl, pairs) == want[2] and res.counts() == want[4]
    return res, want


def check_locate(loc, pl, ctg_off, ctg, mates):
    locus, strand, _, start = pl.host(best2=False)[:4]
    want = cn.locate(ctg_off, ctg if ctg is not None else [], locus, strand, start, mates)
    got = loc.host()
    same(("ctg", "pos"), got, want[:2])
    assert loc.counts() == dict(nr=strand.size, n_located=want[2], n_mismatched=want[3])
    d = loc.device_ptrs()
    same(("ctg", "pos"), tuple(dev_array(p, strand.size, np.uint32) for p in d), got)
    if strand.size == 0:
        assert d == (None, None)
    return got


def chain_against_naive(idx, text, ctg_off, sigma, k, ranks, roff, orientation=pn.FR, discordant=False, rescue_edits=E):
    """map_pairs, the rescue and the locate of one batch on an index that carries ctg_off, every stage against contig_naive"""
    idx.set_contigs(ctg_off)
    reads, loci, al, pl, pairs = idx.map_pairs(ranks, roff, k, comp_of(sigma), **CHAIN, **INSERT, orientation=orientation)
    held = [reads, loci, al, pl, pairs]
    try:
        ranks2, roff2 = fn.double_reads(ranks, roff, COMPLEMENT[sigma], sigma)
        h_loci = loci.host()
        h_al = check_align(al, h_loci, text, ctg_off, ranks2, roff2, sigma, E, CHAIN["max_span"])
        ctg = h_al[5]
        aligned = h_al[0] <= E
        off = np.asarray(ctg_off).astype(np.int64)
        c = ctg[aligned].astype(np.int64)
        assert (h_al[1][aligned] >= off[c]).all() and (h_al[2][aligned] <= off[c + 1]).all()     # no alignment contains a junction
        folded = check_fold(pl, pairs, h_loci, h_al, ctg, **INSERT, orientation=orientation)
        res, want = check_rescue(idx, text, ctg_off, sigma, reads, loci, al, pl, pairs, ranks2, roff2, h_loci, h_al, ctg, **INSERT, max_edits=rescue_edits,
                                 orientation=orientation, discordant=discordant)
        held.append(res)
        loc = pl.locate(idx, al, mates=True)
        held.append(loc)
        lctg, lpos = check_locate(loc, pl, ctg_off, ctg, True)
        assert loc.counts()["n_mismatched"] == 0
        # a pair lies in one contig; a rescued mate in its anchor's
        conc = np.flatnonzero(want[1][0] == pn.CONCORDANT)
        assert (lctg[2 * conc] == lctg[2 * conc + 1]).all() and (lctg[2 * conc] != NC).all()
        return folded, want
    finally:
        close_all(held)


# ---- 1. one contig [0, n] ---------------------------------------------------------------------------------------------------------------
def everything(out):
    """every array and every counter of map_pairs(rescue=True, tags=True)"""
    reads, loci, al, pl, pairs, sc, res, tags = out
    arrays = loci.host() + al.host() + pl.host() + pairs.host() + sc.host() + res.host() + (tags.mapq.host(),) + tags.md.host() + \
        tags.rescue_scripts.host() + tags.rescue_md.host()
    counts = [h.counts() for h in (loci, al, pl, pairs, sc, res, tags.mapq, tags.md, tags.rescue_scripts, tags.rescue_md)]
    return arrays, counts


def test_one_contig_changes_nothing_and_removing_the_table_restores_the_handles(engine):
    name = "dna4_k10"
    sigma, k, n = WORKLOADS[name]
    ranks, roff = rescue_pairs_of(name)
    idx = engine.Index(text_of(sigma, n), sigma, [k], table=2)
    held = []
    try:
        run = lambda: idx.map_pairs(ranks, roff, k, comp_of(sigma), **CHAIN, **INSERT, rescue=True, tags=True, letters=LETTERS[sigma])
        assert idx.contigs() is None
        plain = run()
        held += list(plain)
        assert plain[2].contigs_host() is None and plain[2].contigs_device_ptr() == (None, 0)
        base = everything(plain)
        assert base[1][5]["n_taken"] >= 75
        idx.set_contigs([0, n])
        assert idx.contigs().tolist() == [0, n]
        one = run()
        held += list(one)
        got = everything(one)
        assert got[1] == base[1]
        for i, (g, w) in enumerate(zip(got[0], base[0])):
            assert g.dtype == w.dtype and np.array_equal(g, w), i
        ctg = one[2].contigs_host()
        skipped = one[2].host()[0] == an.SKIPPED
        assert ctg.size == base[1][1]["n_loci"] and (ctg[~skipped] == 0).all() and (ctg[skipped] == NC).all()
        loc = one[3].locate(idx, one[2], mates=True)
        held.append(loc)
        lctg, lpos = loc.host()
        _, strand, _, start = one[3].host(best2=False)[:4]
        placed = strand != 255
        assert loc.counts() == dict(nr=strand.size, n_located=int(placed.sum()), n_mismatched=0)
        assert (lctg[placed] == 0).all() and (lctg[~placed] == NC).all() and np.array_equal(lpos, np.where(placed, start, 0))
        idx.set_contigs(None)
        assert idx.contigs() is None
        again = run()
        held += list(again)
        assert again[2].contigs_host() is None
        back = everything(again)
        assert back[1] == base[1] and all(np.array_equal(g, w) for g, w in zip(back[0], base[0]))
    finally:
        close_all(held)
        idx.close()


# ---- 2. the window clamp ----------------------------------------------------------------------------------------------------------------
CLAMP_SIZES = (1280, 1, 30, 100, 1149, 1281, 1278, 1300)       # junctions at 1280 and 2560 (multiples of 32 and of 8), 3841 and 5119 (+1, -1)


@functools.lru_cache(maxsize=None)
def clamp_text(sigma):
    t = synth.ranks(40 + sigma, sum(CLAMP_SIZES), sigma)
    t.setflags(write=False)
    return t


def clamp_reads(sigma, budget):
    """reads of 64, 65, 150 and 1024 letters cut from the text around the junctions between long contigs: flush with the contig's end,
    over either end by 1, 4, budget and budget + 1 letters, half and half over the junction"""
    text, off = clamp_text(sigma), table_of(CLAMP_SIZES).astype(np.int64)
    reads = []
    for j in (int(off[1]), int(off[5]), int(off[6]), int(off[7])):
        for m in (64, 65, 150, 1024):
            if m == 1024 and j != int(off[5]):                 # (contigs 4 and 5 both hold a read of 1024 letters)
                continue
            reads.append(text[j - m:j])                        # flush with the end of the contig
            reads.append(text[j:j + m])                        # ... and with the start of the next
            for h in (1, 4, budget, budget + 1):
                reads.append(text[j - m + h:j + h])            # over the end
                reads.append(text[j - h:j - h + m])            # over the start
            reads.append(text[j - m // 2:j - m // 2 + m])      # half and half: even and odd lengths
    return pack([np.asarray(q, np.uint8) for q in reads])


def clamp_statistics(h_loci, h_al, whole, text, off, roff, max_edits):
    """(loci whose unclamped window crosses a junction, clamped at lo only, at hi only, at both, results that differ from the whole text's)"""
    locus_off, diag, span = h_loci[:3]
    n = text.size
    crosses = at_lo = at_hi = both = differs = 0
    for r in range(roff.size - 1):
        m = int(roff[r + 1]) - int(roff[r])
        for l in range(int(locus_off[r]), int(locus_off[r + 1])):
            if h_al[0][l] == an.SKIPPED:
                continue
            D, S, c = int(diag[l]), int(span[l]), int(h_al[5][l])
            lo, hi = an.window(n, m, D, S, max_edits)
            crosses += any(lo < int(j) < hi for j in off[1:-1])
            lo_c, hi_c = D - max_edits < int(off[c]), D + S + m + max_edits > int(off[c + 1])
            at_lo += lo_c and not hi_c
            at_hi += hi_c and not lo_c
            both += lo_c and hi_c
            differs += any(int(h_al[k][l]) != int(whole[k][l]) for k in range(3))
    return crosses, at_lo, at_hi, both, differs


@pytest.mark.parametrize("name", sorted(WORKLOADS))
def test_windows_are_clamped_to_the_contig(engine, name):
    sigma, k, _ = WORKLOADS[name]
    text, ctg_off = clamp_text(sigma), table_of(CLAMP_SIZES)
    off = ctg_off.astype(np.int64)
    assert [int(j) % PER[sigma] for j in off[[1, 5]]] == [0, 0] and int(off[6]) % PER[sigma] == 1 and int(off[7]) % PER[sigma] == PER[sigma] - 1
    idx = engine.Index(text, sigma, [k], table=2)
    held = []
    try:
        idx.set_contigs(ctg_off)
        ranks, roff = clamp_reads(sigma, E)
        loci, al = idx.map_reads(ranks, roff, k, **CHAIN)
        held += [loci, al]
        h_loci = loci.host()
        h_al = check_align(al, h_loci, text, ctg_off, ranks, roff, sigma, E, CHAIN["max_span"])
        whole = an.align(text, ranks, roff, h_loci[0], h_loci[1], h_loci[2], E, CHAIN["max_span"], sigma)
        crosses, at_lo, at_hi, both, differs = clamp_statistics(h_loci, h_al, whole, text, off, roff, E)
        assert crosses >= 60 and at_lo >= 1 and at_hi >= 1 and differs >= 1, (crosses, at_lo, at_hi, both, differs)
        aligned = h_al[0] <= E
        c = h_al[5][aligned].astype(np.int64)
        assert aligned.sum() >= 60 and (h_al[1][aligned] >= off[c]).all() and (h_al[2][aligned] <= off[c + 1]).all()
        # a read over the end by h <= E letters comes out with the overhang deleted: distance h, flush with the junction
        assert {1, 4, E} <= set(h_al[0][aligned].tolist())
        # reads longer than their contig: one call with a large budget over the contigs of 1, 30 and 100 letters
        big = 125
        long_reads = [text[int(off[1]) - 60:int(off[4]) + 19], text[int(off[3]) - 25:int(off[4]) + 25], text[int(off[2]) - 17:int(off[3]) + 17],
                      text[int(off[3]) - 10:int(off[3]) + 54], text[int(off[1]) - 32:int(off[1]) + 33]]
        lr, lo_ = pack([np.asarray(q, np.uint8) for q in long_reads])
        loci2, al2 = idx.map_reads(lr, lo_, k, band=8, min_votes=2, max_edits=big, max_span=64)
        held += [loci2, al2]
        h2 = loci2.host()
        a2 = check_align(al2, h2, text, ctg_off, lr, lo_, sigma, big, 64)
        st = clamp_statistics(h2, a2, an.align(text, lr, lo_, h2[0], h2[1], h2[2], big, 64, sigma), text, off, lo_, big)
        assert st[3] >= 1 and st[4] >= 1, st                   # clamped at both ends
        spans = (a2[2].astype(np.int64) - a2[1])[a2[0] <= big]
        assert {1, 30, 100} & set(a2[5][a2[0] <= big].tolist()) and (spans <= 1300).all()
    finally:
        close_all(held)
        idx.close()


# ---- 3. pairs ---------------------------------------------------------------------------------------------------------------------------
def oriented(frag, m, orientation):
    """the mates of a fragment, m letters each, concordant under the orientation"""
    if orientation == pn.FR:
        return frag[:m].copy(), rc(frag[-m:])
    if orientation == pn.RF:
        return rc(frag[:m]), frag[-m:].copy()
    return frag[:m].copy(), frag[-m:].copy()


def junction_pairs(orientation):
    """per junction between two long contigs two pairs whose fragment spans it (each mate inside its own contig) and one pair inside
    the contig; then 6 pairs inside the contig that stands twice"""
    text, off = pair_text(), table_of(PAIR_SIZES).astype(np.int64)
    reads, kind = [], []
    for c in range(len(PAIR_SIZES) - 1):
        j = int(off[c + 1])
        if PAIR_SIZES[c] < 1500 or PAIR_SIZES[c + 1] < 1500:
            continue
        for s, f in ((j - 150, 300), (j - 260, 420)):
            reads += oriented(text[s:s + f], 100, orientation)
            kind.append(1)
        reads += oriented(text[j - 700:j - 350], 100, orientation)
        kind.append(0)
    for i in range(6):
        s = int(off[12]) + 5 + 3 * i
        reads += oriented(text[s:s + 260], 90, orientation)
        kind.append(2)
    return pack([np.asarray(q, np.uint8) for q in reads]), np.asarray(kind)


@pytest.mark.parametrize("orientation", (pn.FR, pn.RF, pn.FF))
def test_pairs_across_a_junction_are_discordant_and_copies_are_not_joined(engine, orientation):
    text, ctg_off = pair_text(), table_of(PAIR_SIZES)
    (ranks, roff), kind = junction_pairs(orientation)
    idx = engine.Index(text, 4, [10], table=2)
    held = []
    try:
        idx.set_contigs(ctg_off)
        out = idx.map_pairs(ranks, roff, 10, comp_of(4), **CHAIN, **INSERT, orientation=orientation, tags=True, letters=LETTERS[4])
        held += list(out)
        reads, loci, al, pl, pairs, sc, tags = out
        h_loci, h_al, ctg = loci.host(), al.host(), al.contigs_host()
        want = check_fold(pl, pairs, h_loci, h_al, ctg, **INSERT, orientation=orientation)
        without = pn.fold_pairs(h_loci[0], *h_al[:4], **INSERT, orientation=orientation)
        across = kind == 1
        assert int((without[7][across] == pn.CONCORDANT).sum()) >= 20 and across.sum() == int((without[7][across] == pn.CONCORDANT).sum())
        assert (want["cls"][across] == pn.DISCORDANT).all() and (want["tlen"][across] == 0).all()
        assert (want["cls"][kind == 0] == pn.CONCORDANT).all()
        # the contig that stands twice: an equal pair in the other copy, MAPQ 0, and no pair that joins the copies
        twice = np.flatnonzero(kind == 2)
        assert (want["cls"][twice] == pn.CONCORDANT).all() and (want["second_score"][twice] == want["score"][twice]).all()
        assert (without[7][twice] == pn.CONCORDANT).all()
        x, y = want["locus"][2 * twice], want["locus"][2 * twice + 1]
        assert (ctg[x] == ctg[y]).all() and set(ctg[x].tolist()) <= {12, 13}
        mapq = tags.mapq.host()
        assert (mapq[2 * twice] == 0).all() and (mapq[2 * twice + 1] == 0).all() and (mapq[2 * np.flatnonzero(kind == 0)] > 0).all()
        # a template across the copies fits the insert range: only the contig rule keeps it out of second_score's sight ... and the same
        # walk without the rule finds nothing better, so the rule is seen in the pairs across the junctions
        assert pairs.counts()["n_discordant"] == int(across.sum())
    finally:
        close_all(held)
        idx.close()


# ---- 4. rescue --------------------------------------------------------------------------------------------------------------------------
RESCUE_SIZES = (3000,) * 10
RESCUE_EDITS = 12


def rescue_reads():
    """per junction three pairs whose mate 1 (100 letters, intact) ends 300 letters before the contig's end and whose mate 2 (80 letters,
    a substitution in every window of 10: 8 edits, no seed) lies inside the contig, 50 letters beyond the junction, over the contig's
    end by 3 letters"""
    text, off = text_of(4, 30_000), table_of(RESCUE_SIZES).astype(np.int64)
    reads, kind = [], []
    for c in range(len(RESCUE_SIZES) - 1):
        j = int(off[c + 1])
        for i, s in enumerate((j - 200, j + 50, j - 77)):
            reads += [text[j - 400:j - 300].copy(), kill(rc(text[s:s + 80]), 10)]
            kind.append(i)
    return pack([np.asarray(q, np.uint8) for q in reads]), np.asarray(kind)


@pytest.mark.parametrize("discordant", (False, True))
def test_rescue_stays_inside_the_anchors_contig(engine, discordant):
    sigma, k = 4, 10
    text, ctg_off = text_of(4, 30_000), table_of(RESCUE_SIZES)
    off = ctg_off.astype(np.int64)
    (ranks, roff), kind = rescue_reads()
    idx = engine.Index(text, sigma, [k], table=2)
    held = []
    try:
        idx.set_contigs(ctg_off)
        reads, loci, al, pl, pairs = idx.map_pairs(ranks, roff, k, comp_of(sigma), **CHAIN, **INSERT)
        held += [reads, loci, al, pl, pairs]
        ranks2, roff2 = fn.double_reads(ranks, roff, COMPLEMENT[sigma], sigma)
        h_loci = loci.host()
        h_al = al.host() + (al.contigs_host(),)
        before_pl, before_pr = pl.host(), pairs.host()
        assert (before_pr[0] == pn.MATE1_ONLY).all()
        plain = rn.rescue(text, sigma, ranks2, roff2, h_loci[0], *h_al[:3], before_pl, before_pr, **INSERT, max_edits=RESCUE_EDITS, discordant=discordant)
        res, want = check_rescue(idx, text, ctg_off, sigma, reads, loci, al, pl, pairs, ranks2, roff2, h_loci, h_al, h_al[5], **INSERT,
                                 max_edits=RESCUE_EDITS, discordant=discordant)
        held.append(res)
        status = want[3][7]
        assert status.size == kind.size and (status[kind == 0] == 3).all() and (status[kind == 2] == 3).all() and (status[kind == 1] == 0).all()
        assert (plain[3][7][kind == 1] == 3).all()             # without the table the mate beyond the junction would have been taken
        # the windows equal the clamped formula; the overhanging mate ends flush with the contig, its overhang deleted
        job_read, lo, hi, jd, js, je = want[3][1], want[3][2], want[3][3], want[3][4], want[3][5], want[3][6]
        for j, r in enumerate(job_read):
            p = int(r) // 4
            c = int(h_al[5][int(before_pl[0][2 * p])])
            assert (int(lo[j]), int(hi[j])) == cn.rescue_window(ctg_off, c, True, int(before_pl[3][2 * p]), int(before_pl[4][2 * p]), INSERT["max_insert"])
            assert int(hi[j]) == int(off[c + 1]) and int(hi[j]) - int(lo[j]) == 400
        over = np.flatnonzero(kind == 2)
        assert (jd[over] == 11).all() and (je[over] == off[1 + over // 3]).all() and (je[over].astype(np.int64) - js[over] <= 77).all()
        assert (jd[kind == 0] == 8).all()
        loc = pl.locate(idx, al, mates=True)
        held.append(loc)
        lctg, _ = check_locate(loc, pl, ctg_off, h_al[5], True)
        assert loc.counts()["n_mismatched"] == 0 and (lctg[1::2][kind != 1] == np.arange(kind.size)[kind != 1] // 3).all()
        assert (lctg[1::2][kind == 1] == NC).all()
        # the same placements without the flag: every rescued read is a mismatch, nothing else changes
        loc2 = pl.locate(idx, al, mates=False, located=None)
        held.append(loc2)
        check_locate(loc2, pl, ctg_off, h_al[5], False)
        assert loc2.counts()["n_mismatched"] == int((kind != 1).sum())
    finally:
        close_all(held)
        idx.close()


# ---- 5. locate and SAM ------------------------------------------------------------------------------------------------------------------
SAM_SIZES = (700, 1, 30, 100, 2169, 3000, 4000, 5000, 15000)   # 30 000 letters
SAM_NAMES = [f"ctg{c}" for c in range(len(SAM_SIZES))]


def sam_check(engine, lines, header, text, ctg_off, sigma, pl, located, paired):
    off = np.asarray(ctg_off).astype(np.int64)
    assert header == ["@HD\tVN:1.6\tSO:unsorted"] + [f"@SQ\tSN:{nm}\tLN:{ln}" for nm, ln in zip(SAM_NAMES, SAM_SIZES)]
    contigs = {nm: spell(text[int(a):int(b)], sigma) for nm, a, b in zip(SAM_NAMES, off[:-1], off[1:])}
    strand = pl.host(best2=False)[1]
    lctg, lpos = located
    n_placed = n_split = 0
    fields = [ln.split("\t") for ln in lines]
    for i, f in enumerate(fields):
        if strand[i] == 255:
            mate_placed = paired and strand[i ^ 1] != 255
            assert f[5] == "*" and (f[2:4] == fields[i ^ 1][2:4] if mate_placed else f[2:4] == ["*", "0"])
            continue
        n_placed += 1
        assert f[2] == SAM_NAMES[int(lctg[i])] and int(f[3]) == int(lpos[i]) + 1
        runs = [(int(a) << 4) | engine.CIGAR_OPS.index(b) for a, b in re.findall(r"([0-9]+)([MIDNSHP=X])", f[5])]
        ref = mn.rebuild(f[9], runs, f[12][5:])                # from the line alone
        pos = int(f[3])
        assert ref == contigs[f[2]][pos - 1:pos - 1 + len(ref)] and pos - 1 + len(ref) <= len(contigs[f[2]])
        if paired:
            m = fields[i ^ 1]
            if strand[i ^ 1] == 255:
                assert f[6:8] == ["=", f[3]]
            else:
                assert f[7] == m[3] and f[6] == ("=" if m[2] == f[2] else m[2])
                n_split += m[2] != f[2]
        else:
            assert f[6:8] == ["*", "0"]
    return n_placed, n_split


def test_locate_and_sam_lines_over_contigs(engine):
    sigma, k = 4, 10
    text, ctg_off = text_of(4, 30_000), table_of(SAM_SIZES)
    off = ctg_off.astype(np.int64)
    assert int(off[-1]) == 30_000
    # the rescue workload's shapes on this text, then pairs whose mates lie in different contigs
    reads = []
    z = synth.u64_stream(4242, 400).astype(np.int64) & 0x7FFFFFFF
    for p in range(120):
        s = int(z[2 * p] % (30_000 - 600))
        f = 250 + int(z[2 * p + 1] % 200)
        frag = rc(text[s:s + f]) if p % 2 else text[s:s + f]
        m1, m2 = frag[:90].copy(), rc(frag[-90:])
        if p % 5 == 0:
            m2 = kill(m2[:80], 10)                          # a mate for the rescue
        if p % 7 == 0:
            m1 = synth.ranks(9000 + p, 90, sigma)
        if p % 11 == 0:
            m2 = rc(text[(s + 9000) % 29_000:(s + 9000) % 29_000 + 90])
        reads += [m1, m2]
    ranks, roff = pack([np.asarray(q, np.uint8) for q in reads])
    idx = engine.Index(text, sigma, [k], table=2)
    held = []
    try:
        idx.set_contigs(ctg_off)
        header = engine.sam_header(SAM_NAMES, idx.contigs())
        qn = [f"q{i // 2}" for i in range(roff.size - 1)]
        # pairs, rescued
        out = idx.map_pairs(ranks, roff, k, comp_of(sigma), **CHAIN, **INSERT, rescue=True, tags=True, letters=LETTERS[sigma])
        held += list(out)
        reads_h, loci, al, pl, pairs, sc, res, tags = out
        ctg = al.contigs_host()
        loc = pl.locate(idx, al, mates=True)
        held.append(loc)
        located = check_locate(loc, pl, ctg_off, ctg, True)
        assert loc.counts()["n_mismatched"] == 0 and res.counts()["n_taken"] >= 10
        cigars, mds = (pl.cigars(sc), res.cigars(tags.rescue_scripts)), (pl.mds(tags.md, sc), res.mds(tags.rescue_md, tags.rescue_scripts))
        lines = engine.sam_lines(qn, ranks, roff, LETTERS[sigma], comp_of(sigma), sigma, SAM_NAMES, pl.host(best2=False), cigars, mds, tags.mapq.host(),
                                 pairs.host(), located_host=located)
        n_placed, n_split = sam_check(engine, lines, header, text, ctg_off, sigma, pl, located, True)
        assert n_placed == pl.counts()["n_placed"] >= 150 and n_split >= 4
        # fold_pairs without the rescue, through the same located handle
        pl2, pr2 = al.fold_pairs(loci, **INSERT)
        held += [pl2, pr2]
        pl2._reads = pr2._reads = reads_h
        assert pl2.locate(idx, al, mates=True, located=loc) is loc
        check_locate(loc, pl2, ctg_off, ctg, True)
        assert loc.counts()["n_mismatched"] == 0
        # single reads: fold_strands, and one located handle at 257, 0, 1 and 3 reads
        for nr in (257, 0, 1, 3):
            sub = pack([np.asarray(reads[i % len(reads)], np.uint8) for i in range(nr)])
            o2 = idx.map_reads_strands(*sub, k, comp_of(sigma), **CHAIN, tags=nr == 257, letters=LETTERS[sigma])
            try:
                al_s, pl_s = o2[2], o2[3]
                sc_s, tags_s = o2[4:] if nr == 257 else (None, None)
                pl_s.locate(idx, al_s, located=loc)
                got = check_locate(loc, pl_s, ctg_off, al_s.contigs_host(), False)
                assert loc.counts()["n_mismatched"] == 0 and loc.counts()["nr"] == nr
                if nr == 257:
                    sl = engine.sam_lines([f"s{i}" for i in range(nr)], *sub, LETTERS[sigma], comp_of(sigma), sigma, SAM_NAMES, pl_s.host(best2=False),
                                          pl_s.cigars(sc_s), pl_s.mds(tags_s.md, sc_s), tags_s.mapq.host(), None, located_host=got)
                    assert sam_check(engine, sl, header, text, ctg_off, sigma, pl_s, got, False)[0] == pl_s.counts()["n_placed"] >= 150
            finally:
                close_all(list(o2))
    finally:
        close_all(held)
        idx.close()


# ---- 6. fuzz ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", range(5))
def test_random_tables_over_the_pairs_workload(engine, seed):
    name = ("dna4_k10", "aa20_k5")[seed % 2]
    sigma, k, _ = WORKLOADS[name]
    n = 12_000
    text = text_of(sigma, 50_000)[:n].copy()
    rng = np.random.default_rng(1000 + seed)
    nc = int(rng.integers(1, 41))
    cuts = np.sort(rng.choice(np.arange(1, n), nc - 1, replace=False)) if nc > 1 else np.zeros(0, np.int64)
    ctg_off = np.concatenate([[0], cuts, [n]]).astype(np.uint64)
    # 60 pairs cut as the rescue workload cuts them (ordinary, broken, random and far mates), in this text
    reads = []
    for p in range(60):
        s = int(rng.integers(0, n - 700))
        f = int(rng.integers(200, 501))
        frag = rc(text[s:s + f], sigma) if p % 2 else text[s:s + f]
        mates = [frag[:int(rng.integers(80, 151))].copy(), rc(frag[f - int(rng.integers(80, 151)):], sigma)]
        lost = (p // 4) % 2
        if p % 4 == 0:
            mates[lost] = kill(mates[lost][:8 * k], k)
        elif p % 4 == 1:
            mates[lost] = rng.integers(0, sigma, 90).astype(np.uint8)
        reads += mates
    ranks, roff = pack([np.asarray(q, np.uint8) for q in reads])
    idx = engine.Index(text, sigma, [k], table=2)
    try:
        orientation = (pn.FR, pn.FR, pn.RF, pn.FF, pn.FR)[seed]
        folded, want = chain_against_naive(idx, text, ctg_off, sigma, k, ranks, roff, orientation=orientation, discordant=bool(seed % 2))
        assert idx.contigs().tolist() == ctg_off.tolist()
        if orientation == pn.FR:
            assert int((want[1][0] == pn.CONCORDANT).sum()) >= 10
    finally:
        idx.close()


# ---- 7. the saved image, refusals -------------------------------------------------------------------------------------------------------
def test_the_table_is_not_part_of_the_saved_image(engine, tmp_path):
    text, good = text_of(4, 30_000), table_of(RESCUE_SIZES)
    idx = engine.Index(text, 4, [10], table=2)
    try:
        plain, with_table = tmp_path / "plain.kmx", tmp_path / "table.kmx"
        idx.save(str(plain))
        idx.set_contigs(good)
        idx.save(str(with_table))
        assert plain.stat().st_size == with_table.stat().st_size   # the image holds no table: its format is what it was
        loaded = engine.Index.load(str(with_table))
        try:
            assert loaded.contigs() is None
            loaded.set_contigs(good)                           # a caller sets it again
            assert loaded.contigs().tolist() == good.tolist() == idx.contigs().tolist()
        finally:
            loaded.close()
    finally:
        idx.close()


def test_refusals_leave_every_handle_as_it_was(engine):
    sigma, k, n = 4, 10, 30_000
    text = text_of(4, n)
    (ranks, roff), _ = rescue_reads()
    idx = engine.Index(text, sigma, [k], table=2)
    held = []
    try:
        good = table_of(RESCUE_SIZES)
        idx.set_contigs(good)
        L = engine.lib()
        # a bad table, in each way: the table that was there stays
        for bad, word in (([1, n], "ctg_off[0]"), ([0, n - 1], "text length"), ([0, n + 1], "text length"), ([0, 500, 500, n], "strictly ascending"),
                          ([0, 600, 500, n], "strictly ascending")):
            with pytest.raises(engine.KmxError, match=re.escape(word)) as e:
                idx.set_contigs(bad)
            assert e.value.status == 1 and idx.contigs().tolist() == good.tolist()
        assert L.kmx_index_set_contigs(idx._h, None, 3) == 1 and b"ctg_off is NULL" in L.kmx_last_error()
        assert L.kmx_index_set_contigs(idx._h, good.ctypes.data, 0xFFFFFFFF) == 1 and b"contigs" in L.kmx_last_error()
        assert L.kmx_index_set_contigs(None, good.ctypes.data, 10) == 1
        assert idx.contigs().tolist() == good.tolist()
        few = np.zeros(3, np.uint64)
        assert L.kmx_index_contigs(idx._h, None, few.ctypes.data, 3) == 1 and not few.any()
        # a chain under `good`
        reads, loci, al, pl, pairs = idx.map_pairs(ranks, roff, k, comp_of(sigma), **CHAIN, **INSERT)
        held += [reads, loci, al, pl, pairs]
        state = lambda: ([a.copy() for a in loci.host() + al.host() + (al.contigs_host(),) + pl.host() + pairs.host()],
                         [h.counts() for h in (loci, al, pl, pairs)])
        before = state()
        res = pairs.rescue(idx, reads, loci, al, pl, **INSERT, max_edits=RESCUE_EDITS)
        loc = pl.locate(idx, al, mates=True)
        held += [res, loc]
        assert res.counts()["n_taken"] >= 10 and loc.counts()["n_mismatched"] == 0
        after_rescue = state()
        # the flag with an odd nr: single reads
        o3 = idx.map_reads_strands(*pack([np.asarray(text[100:200]), np.asarray(text[5000:5100]), np.asarray(text[9000:9100])]), k, comp_of(sigma), **CHAIN)
        held += list(o3)
        with pytest.raises(engine.KmxError, match="odd number of reads") as e:
            o3[3].locate(idx, o3[2], mates=True, located=loc)
        assert e.value.status == 1 and loc.counts() == dict(nr=0, n_located=0, n_mismatched=0) and loc.host()[0].size == 0
        assert o3[3].locate(idx, o3[2], located=loc).counts() == dict(nr=3, n_located=3, n_mismatched=0)
        # a generation mismatch: the alignments were made before this set_contigs (the same offsets, another generation) ...
        idx.set_contigs(good)
        for _ in range(2):
            with pytest.raises(engine.KmxError, match="another contig table") as e:
                pairs.rescue(idx, reads, loci, al, pl, **INSERT, max_edits=RESCUE_EDITS, rescues=res)
            assert e.value.status == 1 and res.counts() == dict(nr2=0, n_jobs=0, n_found=0, n_concordant=0, n_taken=0)
            with pytest.raises(engine.KmxError, match="another contig table") as e:
                pl.locate(idx, al, mates=True, located=loc)
            assert e.value.status == 1 and loc.counts() == dict(nr=0, n_located=0, n_mismatched=0)
            now = state()
            assert now[1] == after_rescue[1] and all(np.array_equal(a, b) for a, b in zip(now[0], after_rescue[0]))     # inputs untouched
            idx.set_contigs(table_of((15_000, 15_000)))        # ... and after a second one
        # alignments made without a table, an index that has one since
        idx.set_contigs(None)
        plain = idx.map_pairs(ranks, roff, k, comp_of(sigma), **CHAIN, **INSERT)
        held += list(plain)
        with pytest.raises(engine.KmxError, match="no contig table"):
            plain[3].locate(idx, plain[2], mates=True, located=loc)
        idx.set_contigs(good)
        with pytest.raises(engine.KmxError, match="another contig table"):
            plain[4].rescue(idx, plain[0], plain[1], plain[2], plain[3], **INSERT, max_edits=RESCUE_EDITS, rescues=res)
        with pytest.raises(engine.KmxError, match="another contig table"):
            plain[3].locate(idx, plain[2], mates=True, located=loc)
        # the fold needs no index: it goes by the handle, and realigning under the table in place makes everything work again
        fresh = idx.map_pairs(ranks, roff, k, comp_of(sigma), **CHAIN, **INSERT)
        held += list(fresh)
        got = [a for a in fresh[1].host() + fresh[2].host() + (fresh[2].contigs_host(),) + fresh[3].host() + fresh[4].host()]
        assert all(np.array_equal(a, b) for a, b in zip(got, before[0]))
        assert fresh[4].rescue(idx, *fresh[:3], fresh[3], **INSERT, max_edits=RESCUE_EDITS, rescues=res).counts()["n_taken"] >= 10
        assert fresh[3].locate(idx, fresh[2], mates=True, located=loc).counts()["n_mismatched"] == 0
    finally:
        close_all(held)
        idx.close()
