"""Paired-end reads on the GPU: kmx_alignments_fold_pairs, Index.map_pairs and kmx_placements_scripts on its placements.  The oracle
is tests/pair_naive.py applied to the host arrays of the engine's own loci and alignments (chain_checks.check_pairs); the texts, the
pairs and their floors are those of tests/chain_data.py."""
import ctypes as C

import numpy as np
import pytest

from kmer_index_amd import synth
from tests import fold_naive as fn
from tests import pair_naive as pn
from tests import script_naive as sn
from tests.chain_checks import MappedPairs, check_pairs, dev_array, refused, same
from tests.chain_data import (ALIGN, CHAIN, COMPLEMENT, INSERT, LOCI, N_PAIRS, PAIRS, PAIR_FLOORS as FLOORS, PAIR_WORKLOADS as WORKLOADS, PLACEMENTS,
                              REPEAT_CHAIN, SCRIPTS, pairs_of, rc, repeat_pair, repeat_text, text_of)
from tests.helpers import pack

pytestmark = pytest.mark.gpu

NO, NONE16 = pn.NO_BEST, pn.NO_SCORE


class Work:
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
            self.mapped[name] = MappedPairs(self.index(name), sigma, *pairs_of(name), k, **CHAIN, **INSERT)
        return self.mapped[name]

    def close(self):
        for m in self.mapped.values():
            m.close()
        for idx in self.indexes.values():
            idx.close()


@pytest.fixture(scope="module")
def work(engine):
    w = Work(engine)
    yield w
    w.close()


# ---- 1. the workload -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(FLOORS))
def test_pairs_of_the_workload_equal_the_oracle(work, name):
    mp = work.workload(name)
    want = check_pairs(mp.pl, mp.pairs, mp.h_loci, mp.h_al, **INSERT)
    n_concordant, n_discordant, n_single = FLOORS[name]
    assert want["np"] == N_PAIRS and want["nr"] == 2 * N_PAIRS
    assert want["n_concordant"] >= n_concordant and want["n_discordant"] >= n_discordant and want["n_single"] >= n_single
    assert set(want["cls"].tolist()) == {pn.UNPLACED, pn.CONCORDANT, pn.DISCORDANT, pn.MATE1_ONLY, pn.MATE2_ONLY}
    conc = want["cls"] == pn.CONCORDANT
    assert int((want["tlen"][conc] < 0).sum()) * 4 >= int(conc.sum()) and int((want["tlen"][conc] > 0).sum()) * 4 >= int(conc.sum())
    assert (want["tlen"][~conc] == 0).all() and (np.abs(want["tlen"][conc]) >= 100).all() and (np.abs(want["tlen"][conc]) <= 600).all()


# ---- 2. the case that needs the feature ------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def repeat_index(engine):
    idx = engine.Index(repeat_text()[0], 4, [10], table=2)
    yield idx
    idx.close()


def test_unique_mate_pulls_its_partner_out_of_the_repeat(repeat_index):
    mp = MappedPairs(repeat_index, 4, *repeat_pair(), 10, **REPEAT_CHAIN, min_insert=450, max_insert=520)
    pl2 = None
    try:
        want = check_pairs(mp.pl, mp.pairs, mp.h_loci, mp.h_al, 450, 520)
        assert want["cls"].tolist() == [pn.CONCORDANT] and want["start"].tolist() == [8800, 9200] and want["end"].tolist() == [8900, 9300]
        assert want["strand"].tolist() == [0, 1] and want["tlen"].tolist() == [500]
        assert want["score"].tolist() == [0] and want["second_score"].tolist() == [NONE16] and want["n_pairs_ambiguous"] == 0
        assert want["second"].tolist() == [0, 255] and want["n_ambiguous"] == 1      # mate 1 alone stays a repeat read
        assert int(np.diff(mp.h_loci[0].astype(np.int64))[0]) > 128
        assert want["best2"][0] != mp.h_al[3][0] and want["best2"][0] != NO         # not the read's best
        # the strand fold on the same handles: the leftmost copy
        pl2 = mp.al.fold_strands(mp.loci)
        assert pl2.host()[3].tolist() == [2000, 9200] and pl2.host()[0][0] != want["locus"][0]
        # every copy within reach: the leftmost concordant one, and a disjoint one at the same score
        mp.al.fold_pairs(mp.loci, 0, 600, placements=mp.pl, pairs=mp.pairs)
        want = check_pairs(mp.pl, mp.pairs, mp.h_loci, mp.h_al, 0, 600)
        assert want["cls"].tolist() == [pn.CONCORDANT] and want["start"].tolist() == [8700, 9200] and want["tlen"].tolist() == [600]
        assert want["score"].tolist() == [0] and want["second_score"].tolist() == [0] and want["n_pairs_ambiguous"] == 1
    finally:
        if pl2 is not None:
            pl2.close()
        mp.close()


def test_both_mates_in_the_repeat_take_more_than_two_rounds_of_the_lanes(repeat_index):
    _, unit = repeat_text()
    two = np.concatenate([unit, unit])
    three = np.concatenate([unit, unit, unit[:30]])
    # pair 0: 139 forward loci against 139 reverse ones; pair 1: the mates differ in their numbers of loci, mate 2 the upstream one
    mp = MappedPairs(repeat_index, 4, *pack([two, rc(two), rc(two), three]), 10, **REPEAT_CHAIN, min_insert=100, max_insert=600)
    try:
        want = check_pairs(mp.pl, mp.pairs, mp.h_loci, mp.h_al, 100, 600)
        n_loci = np.diff(mp.h_loci[0].astype(np.int64))
        assert n_loci[0] > 128 and n_loci[3] > 128 and n_loci[5] > 128 and n_loci[6] > 128 and n_loci[5] != n_loci[6]
        assert n_loci[1] == n_loci[2] == n_loci[4] == n_loci[7] == 0
        assert want["cls"].tolist() == [pn.CONCORDANT] * 2 and want["score"].tolist() == [0, 0] and want["second_score"].tolist() == [0, 0]
        assert want["start"][0] == 2000 and want["tlen"][0] > 0 > want["tlen"][1] and want["n_pairs_ambiguous"] == 2
        # in a repeat the mates face away just as well, with the other mate upstream; on one strand nothing fits
        mp.al.fold_pairs(mp.loci, 100, 600, orientation=pn.RF, placements=mp.pl, pairs=mp.pairs)
        want = check_pairs(mp.pl, mp.pairs, mp.h_loci, mp.h_al, 100, 600, pn.RF)
        assert want["cls"].tolist() == [pn.CONCORDANT] * 2 and want["tlen"][0] < 0 < want["tlen"][1]
        mp.al.fold_pairs(mp.loci, 100, 600, orientation=pn.FF, placements=mp.pl, pairs=mp.pairs)
        assert check_pairs(mp.pl, mp.pairs, mp.h_loci, mp.h_al, 100, 600, pn.FF)["cls"].tolist() == [pn.DISCORDANT] * 2
    finally:
        mp.close()


# ---- 3. shapes -------------------------------------------------------------------------------------------------------------------------
def test_batches_of_every_size_through_one_pair_of_handles(work):
    name = "dna4_k10"
    sigma, k, _ = WORKLOADS[name]
    idx = work.index(name)
    ranks, roff = pairs_of(name)
    pl, pr = work.engine.Placements(), work.engine.Pairs()
    try:
        for n_pairs in (257, 0, 1, 3, 4, 5, 257):             # four pairs to a block; the handles grow and shrink
            sub_off = roff[:2 * n_pairs + 1]
            mp = MappedPairs(idx, sigma, ranks[:int(sub_off[-1])], sub_off, k, **CHAIN, **INSERT)
            try:
                mp.al.fold_pairs(mp.loci, **INSERT, unpaired_penalty=3, placements=pl, pairs=pr)
                want = check_pairs(pl, pr, mp.h_loci, mp.h_al, **INSERT, unpaired_penalty=3)
                assert want["np"] == n_pairs
                if n_pairs == 0:
                    assert pl.device_ptrs() == (None,) * 7 and pr.device_ptrs() == (None,) * 4
                    assert pr.counts() == dict(np=0, n_concordant=0, n_discordant=0, n_single=0, n_unplaced=0, n_ambiguous=0)
            finally:
                mp.close()
    finally:
        pr.close()
        pl.close()


def test_overhanging_empty_and_short_mates(work):
    name = "dna4_k10"
    sigma, k, n = WORKLOADS[name]
    text = text_of(sigma, n)
    junk = synth.ranks(4711, 5, sigma)
    reads = [np.concatenate([junk, text[:95]]), rc(text[300:400]),                   # mate 1 overhangs the start of the text
             text[n - 400:n - 300].copy(), rc(np.concatenate([text[n - 95:], junk])),  # mate 2 overhangs its end
             np.zeros(0, np.uint8), rc(text[1300:1400]),                             # a mate of no letters
             text[2000:2100].copy(), rc(text[2300:2300 + k - 1]),                     # a mate shorter than k: no windows
             text[3000:3100].copy(), rc(text[3300:3400])]
    mp = MappedPairs(work.index(name), sigma, *pack(reads), k, **CHAIN, **INSERT)
    try:
        want = check_pairs(mp.pl, mp.pairs, mp.h_loci, mp.h_al, **INSERT)
        assert want["cls"].tolist() == [pn.CONCORDANT, pn.CONCORDANT, pn.MATE2_ONLY, pn.MATE1_ONLY, pn.CONCORDANT]
        assert want["start"][0] == 0 and want["end"][3] == n and 0 < want["dist"][0] <= 5 and 0 < want["dist"][3] <= 5
        assert want["tlen"].tolist()[2:] == [0, 0, 400] and want["score"].tolist()[2:] == [0, 0, 0]
    finally:
        mp.close()


def test_pair_of_skipped_loci(repeat_index):
    text, _ = repeat_text()
    gapped = np.delete(text[100:171], 35)                     # two diagonals one apart: a locus of span 1 at band 4
    other = np.delete(text[400:471], 35)
    mp = MappedPairs(repeat_index, 4, *pack([gapped, rc(other)]), 10, band=4, min_votes=8, max_edits=8, max_span=0, min_insert=0, max_insert=1000)
    try:
        want = check_pairs(mp.pl, mp.pairs, mp.h_loci, mp.h_al, 0, 1000)
        assert mp.h_al[0].size >= 2 and (mp.h_al[0] == fn.SKIPPED).all()
        assert want["cls"].tolist() == [pn.UNPLACED] and want["score"].tolist() == [NONE16] and want["best2"].tolist() == [NO] * 4
        assert (want["n_unplaced"], want["n_placed"]) == (1, 0)
    finally:
        mp.close()


def test_orientations_on_pairs_built_for_them(work):
    name = "dna4_k10"
    sigma, k, n = WORKLOADS[name]
    text = text_of(sigma, n)
    a, b = text[7000:7100].copy(), text[7300:7400].copy()     # upstream and downstream
    reads = [a, rc(b), rc(b), a,                              # FR, mate 1 upstream; FR, mate 2 upstream
             rc(a), b, b, rc(a),                              # RF
             a, b, rc(b), rc(a),                              # FF on the forward strand, on the reverse strand
             b, a, rc(a), rc(b)]                              # FF the wrong way round
    mp = MappedPairs(work.index(name), sigma, *pack(reads), k, **CHAIN, **INSERT)
    try:
        C_, D_ = pn.CONCORDANT, pn.DISCORDANT
        for o, cls, tlen in ((pn.FR, [C_, C_, D_, D_, D_, D_, D_, D_], [400, -400, 0, 0, 0, 0, 0, 0]),
                             (pn.RF, [D_, D_, C_, C_, D_, D_, D_, D_], [0, 0, 400, -400, 0, 0, 0, 0]),
                             (pn.FF, [D_, D_, D_, D_, C_, C_, D_, D_], [0, 0, 0, 0, 400, -400, 0, 0])):
            mp.al.fold_pairs(mp.loci, 100, 600, orientation=o, placements=mp.pl, pairs=mp.pairs)
            want = check_pairs(mp.pl, mp.pairs, mp.h_loci, mp.h_al, 100, 600, o)
            assert want["cls"].tolist() == cls and want["tlen"].tolist() == tlen, o
    finally:
        mp.close()


# ---- 4. the scripts of the chosen loci -------------------------------------------------------------------------------------------------
def check_scripts(mp, text, sigma):
    """pl.scripts on a fold_pairs placements handle against script_naive with the placements' best2; returns the reads whose chosen
    locus is not their best"""
    ranks2, roff2 = fn.double_reads(mp.ranks, mp.roff, COMPLEMENT[sigma], sigma)
    dist, start, end, best, _ = mp.h_al
    locus, strand, p_dist, p_start, p_end, _, best2 = mp.pl.host()
    placed = strand != 255
    scr = mp.pl.scripts(mp.idx, mp.reads, mp.loci, mp.al)
    try:
        want = sn.scripts(text, ranks2, roff2, mp.h_loci[0], dist, start, end, best2, sigma, False, False)
        got = scr.host()
        same(SCRIPTS, got, want[:4])
        c = scr.counts()
        assert (c["nr"], c["n_sel"], c["n_mismatched"]) == (2 * strand.size, int(placed.sum()), 0) and want[4] == 0
        assert np.array_equal(got[1], locus[placed])
        for e, i in enumerate(np.flatnonzero(placed)):        # every script replays: the read, or its reverse complement, against the text
            q = mp.ranks[int(mp.roff[i]):int(mp.roff[i + 1])]
            q = rc(q, sigma) if strand[i] else q
            runs = got[3][int(got[2][e]):int(got[2][e + 1])]
            assert sn.replay(q, text[int(p_start[i]):int(p_end[i])], runs, sigma) == (int(p_dist[i]), True), i
        cigars = mp.pl.cigars(scr)
        assert [bool(s) for s in cigars] == placed.tolist()
    finally:
        scr.close()
    internal = 2 * np.arange(strand.size) + np.minimum(strand, 1)
    return np.flatnonzero(placed & (best2[internal] != best[internal]))


def test_scripts_of_the_chosen_loci(work, repeat_index):
    name = "dna4_k10"
    sigma, _, n = WORKLOADS[name]
    mp = work.workload(name)
    check_pairs(mp.pl, mp.pairs, mp.h_loci, mp.h_al, **INSERT)
    check_scripts(mp, text_of(sigma, n), sigma)
    mp = MappedPairs(repeat_index, 4, *repeat_pair(), 10, **REPEAT_CHAIN, min_insert=450, max_insert=520)
    try:
        assert check_scripts(mp, repeat_text()[0], 4).tolist() == [0]          # mate 1 at 8800 and not at its best, 2000
        assert mp.pl.cigars(mp.pl.scripts(mp.idx, mp.reads, mp.loci, mp.al)) == ["100=", "100="]
    finally:
        mp.close()


# ---- 5. plumbing -----------------------------------------------------------------------------------------------------------------------
def test_refusals_and_the_state_of_both_handles(engine, repeat_index):
    text, _ = repeat_text()
    idx, L = repeat_index, engine.lib()
    kw = dict(band=0, min_votes=8, max_edits=4)                # (no locus of a chance match of 11 letters)
    batch = [text[100:170].copy(), rc(text[300:390]), text[500:600].copy(), rc(text[700:800])]
    mp = MappedPairs(idx, 4, *pack(batch), 10, **kw, min_insert=0, max_insert=1000)
    held = []
    try:
        loci6, al6 = idx.map_reads(*pack([text[100:170].copy()] * 6), 10, **kw)
        loci8, al8 = idx.map_reads(*pack(batch + batch), 10, **kw)
        loci8b, al8b = idx.map_reads(*pack(batch + [text[1000:1100].copy()] * 4), 10, **kw)
        loci4, al4 = idx.map_reads(*pack(batch), 10, **kw)
        held += [loci6, al6, loci8, al8, loci8b, al8b, loci4, al4]
        pl, pr = mp.pl, mp.pairs
        full = (dict(nr=4, n_placed=4, n_reverse=2, n_ambiguous=0), dict(np=2, n_concordant=2, n_discordant=0, n_single=0, n_unplaced=0, n_ambiguous=0))
        assert (pl.counts(), pr.counts()) == full
        assert loci8.counts()["nr"] == 8 and loci8.counts()["n_loci"] != loci8b.counts()["n_loci"]
        # after looking at the handles: both hold an empty result
        for call, word in ((lambda: al6.fold_pairs(loci6, 0, 1000, placements=pl, pairs=pr), "multiple of 4"),
                           (lambda: al4.fold_pairs(loci8, 0, 1000, placements=pl, pairs=pr), "nr differs"),
                           (lambda: al8.fold_pairs(loci4, 0, 1000, placements=pl, pairs=pr), "nr differs"),
                           (lambda: al8.fold_pairs(loci8b, 0, 1000, placements=pl, pairs=pr), "n_loci differs")):
            al8.fold_pairs(loci8, 0, 1000, placements=pl, pairs=pr)
            assert (pl.counts()["nr"], pr.counts()["np"]) == (4, 2) and pl.counts()["n_placed"] > 0
            assert word in refused(engine, call)
            assert pl.counts() == dict(nr=0, n_placed=0, n_reverse=0, n_ambiguous=0)
            assert pr.counts() == dict(np=0, n_concordant=0, n_discordant=0, n_single=0, n_unplaced=0, n_ambiguous=0)
            assert all(x.size == 0 for x in pl.host()) and all(x.size == 0 for x in pr.host())
            assert pl.device_ptrs() == (None,) * 7 and pr.device_ptrs() == (None,) * 4
        # before any handle is looked at: both results stay
        mp.al.fold_pairs(mp.loci, 0, 1000, placements=pl, pairs=pr)
        size = C.sizeof(engine.PairOptions)
        assert size == 24
        good = engine.PairOptions(size, 0, 1000, engine.PAIR_FR, engine.PAIR_NO_PENALTY, 0)
        for o, word in ((engine.PairOptions(size - 1, 0, 1000, 0, 0, 0), "struct_size"), (engine.PairOptions(size, 0, 1000, 0, 0, 1), "flags"),
                        (engine.PairOptions(size, 0, 1000, 3, 0, 0), "orientation"), (engine.PairOptions(size, 1001, 1000, 0, 0, 0), "min_insert"),
                        (engine.PairOptions(size, 0, 1 << 31, 0, 0, 0), "2^31")):
            assert L.kmx_alignments_fold_pairs(mp.loci._h, mp.al._h, C.byref(o), None, C.byref(pl._h), C.byref(pr._h)) == 1
            assert word.encode() in L.kmx_last_error()
        assert L.kmx_alignments_fold_pairs(None, mp.al._h, C.byref(good), None, C.byref(pl._h), C.byref(pr._h)) == 1
        assert L.kmx_alignments_fold_pairs(mp.loci._h, None, C.byref(good), None, C.byref(pl._h), C.byref(pr._h)) == 1
        assert L.kmx_alignments_fold_pairs(mp.loci._h, mp.al._h, None, None, C.byref(pl._h), C.byref(pr._h)) == 1
        assert L.kmx_alignments_fold_pairs(mp.loci._h, mp.al._h, C.byref(good), None, None, C.byref(pr._h)) == 1
        assert L.kmx_alignments_fold_pairs(mp.loci._h, mp.al._h, C.byref(good), None, C.byref(pl._h), None) == 1
        assert L.kmx_pairs_counts(None, *[None] * 6) == 1 and L.kmx_pairs_view(None, *[None] * 4) == 1 and L.kmx_pairs_view_device(None, *[None] * 4) == 1
        L.kmx_pairs_free(None)
        assert (pl.counts(), pr.counts()) == full
        check_pairs(pl, pr, mp.h_loci, mp.h_al, 0, 1000)
        # the greatest max_insert and a NULL-allocated pair of handles
        pl2, pr2 = mp.al.fold_pairs(mp.loci, 0, (1 << 31) - 1)
        held += [pl2, pr2]
        check_pairs(pl2, pr2, mp.h_loci, mp.h_al, 0, (1 << 31) - 1)
    finally:
        for h in held:
            h.close()
        mp.close()


def test_views_agree_inputs_stay_and_map_pairs_is_the_calls_it_is_made_of(work):
    name = "dna4_k10"
    sigma, k, _ = WORKLOADS[name]
    mp, idx, engine = work.workload(name), work.index(name), work.engine
    ptrs = (mp.loci.device_ptrs(), mp.al.device_ptrs())
    mp.al.fold_pairs(mp.loci, **INSERT, placements=mp.pl, pairs=mp.pairs)
    check_pairs(mp.pl, mp.pairs, mp.h_loci, mp.h_al, **INSERT)
    dts = (np.uint32, np.uint8, np.uint8, np.uint32, np.uint32, np.uint8, np.uint32)
    same(PLACEMENTS, [dev_array(p, (4 if x == "best2" else 2) * N_PAIRS, d) for p, d, x in zip(mp.pl.device_ptrs(), dts, PLACEMENTS)], mp.pl.host())
    same(PAIRS, [dev_array(p, N_PAIRS, d) for p, d in zip(mp.pairs.device_ptrs(), (np.uint8, np.int32, np.uint16, np.uint16))], mp.pairs.host())
    # the strand fold on the same handles is what it was, and the inputs are untouched
    pl = mp.al.fold_strands(mp.loci)
    try:
        dist, start, end, best, _ = mp.h_al
        want = fn.fold(mp.h_loci[0], dist, start, end, best)
        same(PLACEMENTS, pl.host(), want[:7])
        c = pl.counts()
        assert (c["nr"], c["n_placed"], c["n_reverse"], c["n_ambiguous"]) == (2 * N_PAIRS,) + want[7:]
    finally:
        pl.close()
    assert ptrs == (mp.loci.device_ptrs(), mp.al.device_ptrs())
    same(LOCI, mp.loci.host(), mp.h_loci)
    same(ALIGN, mp.al.host(), mp.h_al)
    # map_pairs: the calls it is made of
    ranks, roff = pairs_of(name)
    comp = np.asarray(COMPLEMENT[sigma], np.uint8)
    reads = idx.strand_reads(ranks, roff, comp)
    held = [reads]
    try:
        d_ranks2, d_roff2, nr2, stream = reads.device_ptrs()
        r = idx.search_windows_device(d_ranks2, d_roff2, nr2, k, 1, stream=stream)
        try:
            loci = r.vote(CHAIN["band"], CHAIN["min_votes"], 0)
        finally:
            r.close()
        held.append(loci)
        al = loci.align_device(idx, d_ranks2, d_roff2, nr2, CHAIN["max_edits"], CHAIN["max_span"], stream=stream)
        held.append(al)
        pl, pr = al.fold_pairs(loci, **INSERT, stream=stream)
        held += [pl, pr]
        same(LOCI, loci.host(), mp.h_loci)
        same(ALIGN, al.host(), mp.h_al)
        same(PLACEMENTS, pl.host(), mp.pl.host())
        same(PAIRS, pr.host(), mp.pairs.host())
        assert (pl.counts(), pr.counts()) == (mp.pl.counts(), mp.pairs.counts())
    finally:
        for h in reversed(held):
            h.close()
    # with scripts, and the SAM fields of the result
    out = idx.map_pairs(ranks, roff, k, comp, **INSERT, **CHAIN, scripts=True)
    try:
        assert len(out) == 6 and out[5].counts()["n_sel"] == mp.pl.counts()["n_placed"]
        same(PAIRS, out[4].host(), mp.pairs.host())
        strand, start = out[3].host(best2=False)[1], out[3].host(best2=False)[3]
        cls, tlen = out[4].host()[:2]
        flag, pos, pnext, t = engine.sam_pair_fields(strand, start, cls, tlen)
        assert int(((flag & 0x2) != 0).sum()) == 2 * mp.pairs.counts()["n_concordant"] and np.array_equal(t[0::2], tlen)
        assert np.array_equal(pos[strand != 255], start[strand != 255].astype(np.int64) + 1)
    finally:
        for h in reversed(out):
            h.close()


def test_map_pairs_refuses_an_odd_number_of_reads(work):
    name = "dna4_k10"
    sigma, k, n = WORKLOADS[name]
    text = text_of(sigma, n)
    with pytest.raises(ValueError):
        work.index(name).map_pairs(*pack([text[:100].copy(), text[200:300].copy(), text[400:500].copy()]), k, np.asarray(COMPLEMENT[sigma], np.uint8),
                                   **INSERT, **CHAIN)
