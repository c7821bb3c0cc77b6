"""Both strands of the mapping chain on the GPU: kmx_reads_strands, kmx_alignments_fold_strands, kmx_placements_scripts and
Index.map_reads_strands.  The oracles are tests/fold_naive.py (the doubled batch and the fold) and tests/script_naive.py, applied to
the host arrays of the engine's own loci and alignments; the chain in between is compared with the one-strand chain (Index.map_reads)
on the oracle's doubled batch."""
import ctypes as C
import functools

import numpy as np
import pytest

from kmer_index_amd import synth
from tests import fold_naive as fn
from tests import script_naive as sn
from tests import chain_data
from tests.chain_checks import MappedStrands as Mapped, StrandWork as Work, check_fold, dev_array, refused, same
from tests.chain_data import ALIGN, CHAIN, COMPLEMENT, FOLD, LOCI, N_READS, READ_WORKLOADS, STRAND_FLOORS as FLOORS, rc4, repeat_text, text_of
from tests.helpers import pack

pytestmark = pytest.mark.gpu

NO = fn.NO_BEST
WORKLOADS = {name: READ_WORKLOADS[name] for name in ("dna4_k10", "aa20_k5")}      # (sigma, k, text length, reads of the generator)
reads_of = functools.partial(chain_data.reads_of, n_reads=N_READS, reverse_odd=True)      # every odd-numbered read reverse-complemented


@pytest.fixture(scope="module")
def work(engine):
    w = Work(engine)
    yield w
    w.close()


# ---- 1. the doubled batch ------------------------------------------------------------------------------------------------------------
LENGTHS = (0, 1, 2, 63, 64, 65, 255, 256, 257, 1024)


def strand_batch(sigma, nr):
    """nr reads of the lengths above in turn, letters >= sigma (sigma and 255) at the first, middle and last letter of some"""
    reads = []
    for i in range(nr):
        m = LENGTHS[(i + nr) % len(LENGTHS)]
        q = synth.ranks(31 * nr + i, m, sigma)
        if m and i % 3 == 0:
            q[(0, m // 2, m - 1)[(i // 3) % 3]] = (sigma, 255)[(i // 9) % 2]
        reads.append(q)
    return pack(reads)


@pytest.fixture(scope="module")
def small_indexes(engine):
    out = {sigma: engine.Index(synth.ranks(90 + sigma, 3000, sigma), sigma, [5], table=2) for sigma in (4, 5, 20)}
    yield out
    for idx in out.values():
        idx.close()


def read_back(reads):
    d_ranks2, d_roff2, nr2, _ = reads.device_ptrs()
    roff2 = dev_array(d_roff2, nr2 + 1, np.uint64)
    return dev_array(d_ranks2, int(roff2[-1]), np.uint8), roff2


@pytest.mark.parametrize("form", ["host", "device"])
@pytest.mark.parametrize("sigma", [4, 5, 20])
def test_doubled_batch_equals_the_oracle(engine, small_indexes, sigma, form):
    import torch

    idx = small_indexes[sigma]
    comp = engine.complement_table(sigma) if sigma != 20 else np.arange(20, dtype=np.uint8)
    assert tuple(comp.tolist()) == COMPLEMENT[sigma]
    stream = torch.cuda.Stream()
    handle = None
    for nr in (257, 0, 1, 255, 256, 10):                      # one handle throughout: it grows and shrinks
        ranks, roff = strand_batch(sigma, nr) if nr != 10 else pack([synth.ranks(5 + m, m, sigma) for m in LENGTHS])
        if nr == 10:
            for at, r in ((0, 3), (127, 6), (256, 8), (1023, 9), (0, 1)):      # first, middle and last letters
                ranks[int(roff[r]) + at] = (sigma, 255)[r % 2]
        if form == "host":
            handle = idx.strand_reads(ranks, roff, comp, reads=handle)
        else:
            d_r = torch.from_numpy(np.array(ranks) if ranks.size else np.zeros(1, np.uint8)).cuda()
            d_o = torch.from_numpy(np.array(roff).view(np.int64)).cuda()
            torch.cuda.synchronize()
            handle = idx.strand_reads_device(d_r.data_ptr(), d_o.data_ptr(), nr, comp, stream=stream.cuda_stream, reads=handle)
            assert handle.device_ptrs()[3] == stream.cuda_stream
            stream.synchronize()
        assert handle.counts() == {"nr": nr, "nr2": 2 * nr}
        want = fn.double_reads(ranks, roff, comp, sigma)
        same(("ranks2", "roff2"), read_back(handle), want)
    handle.close()


# ---- 2. the chain on the device's doubled batch ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["dna4_k10", "aa20_k5"])
def test_chain_on_the_doubled_batch_equals_map_reads_on_the_oracles(work, name):
    sigma, k, _, _ = WORKLOADS[name]
    mp = work.workload(name)
    ranks2, roff2 = fn.double_reads(mp.ranks, mp.roff, COMPLEMENT[sigma], sigma)
    loci, al = work.index(name).map_reads(ranks2, roff2, k, **CHAIN)
    try:
        same(LOCI, mp.h_loci, loci.host())
        same(ALIGN, mp.h_al, al.host())
        assert mp.loci.counts() == loci.counts() and mp.al.counts() == al.counts()
        assert mp.loci.counts()["nr"] == 2 * N_READS
    finally:
        al.close()
        loci.close()


# ---- 3. the fold against the oracle ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,band", sorted(FLOORS))
def test_fold_equals_the_oracle(work, name, band):
    mp = work.workload(name, band)
    want = check_fold(mp.pl, mp.h_loci, mp.h_al)
    n_placed, n_fwd, n_rev, n_dup = FLOORS[(name, band)]
    placed = want["strand"] != 255
    assert want["n_placed"] == n_placed == int(placed.sum())
    assert int((want["strand"] == 0).sum()) >= n_fwd >= n_placed // 4
    assert want["n_reverse"] >= n_rev >= n_placed // 4
    off = mp.h_loci[0].astype(np.int64)
    aligned2 = np.add.reduceat(np.append(mp.h_al[4], 0).astype(np.int64), np.arange(0, 2 * N_READS, 2))      # per public read
    assert int((placed & (aligned2 >= 2) & (want["second"] == 255)).sum()) >= n_dup
    assert n_dup > 0 or band != 0                             # the split diagonals of the reads with a deletion and an insertion
    assert off[-1] == mp.h_al[0].size


# ---- 4. shapes where the fold can go wrong ---------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def repeat_index(engine):
    idx = engine.Index(repeat_text()[0], 4, [10], table=2)
    yield idx
    idx.close()


def test_fold_on_repeats_palindromes_and_one_sided_reads(repeat_index):
    text, unit = repeat_text()
    two = np.concatenate([unit, unit])
    last_only = text[8970:9040].copy()                        # the tail of the last unit and what follows it: 140 loci, the last one is it
    reads = [two, rc4(two), text[11000:11040].copy(), last_only, text[300:380].copy(), rc4(text[500:580]), text[700:705].copy()]
    ranks, roff = pack(reads)
    mp = Mapped(repeat_index, 4, ranks, roff, 10, band=0, min_votes=2, max_edits=8)
    try:
        want = check_fold(mp.pl, mp.h_loci, mp.h_al)
        off = mp.h_loci[0].astype(np.int64)
        n_loci = np.diff(off)
        dist = mp.h_al[0]
        # two units: more than two rounds of the wave on one strand, nothing on the other; ambiguous at distance 0
        for i, s in ((0, 0), (1, 1)):
            assert n_loci[2 * i + s] > 128 and n_loci[2 * i + 1 - s] == 0
            assert (want["strand"][i], want["dist"][i], want["second"][i]) == (s, 0, 0)
            assert text[want["start"][i]:want["end"][i]].tolist() == two.tolist()
        assert want["start"][0] == want["start"][1]           # the leftmost of the 139 places, on either strand
        # the palindrome: one placement, seen on both strands
        assert np.array_equal(rc4(reads[2]), reads[2])
        assert (want["strand"][2], want["dist"][2], want["second"][2], want["start"][2], want["end"][2]) == (0, 0, 0, 11000, 11040)
        assert n_loci[4] >= 1 and n_loci[5] >= 1
        # only the last of 140 loci aligns
        a, b = off[6], off[7]
        assert b - a > 64 and n_loci[7] == 0
        assert np.flatnonzero(dist[a:b] < fn.SKIPPED).tolist() == [b - a - 1]
        assert (want["locus"][3], want["strand"][3], want["dist"][3], want["second"][3], want["start"][3]) == (b - 1, 0, 0, 255, 8970)
        # one strand only, each way
        assert (n_loci[8] > 0, n_loci[9], want["strand"][4], want["start"][4], want["second"][4]) == (True, 0, 0, 300, 255)
        assert (n_loci[10], n_loci[11] > 0, want["strand"][5], want["start"][5], want["second"][5]) == (0, True, 1, 500, 255)
        # no window at all
        assert n_loci[12] == n_loci[13] == 0 and want["strand"][6] == 255 and want["locus"][6] == NO
        assert (want["n_placed"], want["n_reverse"], want["n_ambiguous"]) == (6, 2, 3)
    finally:
        mp.close()


def test_fold_of_skipped_loci_and_of_one_and_no_reads(repeat_index):
    text, _ = repeat_text()
    gapped = np.delete(text[100:171], 35)                     # two diagonals one apart: a locus of span 1 at band 4
    # (min_votes = 8: an 11-letter chance match casts two votes on one diagonal, and such a locus would not be skipped)
    mp = Mapped(repeat_index, 4, *pack([gapped, rc4(gapped)]), 10, band=4, min_votes=8, max_edits=8, max_span=0)
    try:
        want = check_fold(mp.pl, mp.h_loci, mp.h_al)
        assert mp.h_al[0].size >= 2 and (mp.h_al[0] == fn.SKIPPED).all()
        assert want["strand"].tolist() == [255, 255] and want["best2"].tolist() == [NO] * 4 and want["n_placed"] == 0
    finally:
        mp.close()
    mp = Mapped(repeat_index, 4, *pack([text[100:170].copy()]), 10, band=0, min_votes=2, max_edits=8)
    try:
        want = check_fold(mp.pl, mp.h_loci, mp.h_al)
        assert (want["strand"].tolist(), want["start"].tolist(), want["n_placed"]) == ([0], [100], 1)
    finally:
        mp.close()
    mp = Mapped(repeat_index, 4, *pack([]), 10, band=0, min_votes=2, max_edits=8)
    try:
        want = check_fold(mp.pl, mp.h_loci, mp.h_al)
        assert all(want[k].size == 0 for k in FOLD) and mp.pl.counts() == {"nr": 0, "n_placed": 0, "n_reverse": 0, "n_ambiguous": 0}
        assert mp.pl.device_ptrs() == (None,) * 7
    finally:
        mp.close()


# ---- 5. the scripts of the winners -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["dna4_k10", "aa20_k5"])
def test_scripts_of_the_winners(engine, work, name):
    sigma, _, n, _ = WORKLOADS[name]
    mp, idx, text = work.workload(name), work.index(name), text_of(sigma, n)
    ranks2, roff2 = fn.double_reads(mp.ranks, mp.roff, COMPLEMENT[sigma], sigma)
    dist, start, end, best, _ = mp.h_al
    locus, strand, _, p_start, p_end, _, best2 = mp.pl.host()
    placed = strand != 255
    names = ("read_sel_off", "sel", "cig_off", "cigar")
    scr = mp.pl.scripts(idx, mp.reads, mp.loci, mp.al)
    try:
        want = sn.scripts(text, ranks2, roff2, mp.h_loci[0], dist, start, end, best2, sigma, False, False)
        got = scr.host()
        same(names, got, want[:4])
        c = scr.counts()
        assert (c["nr"], c["n_sel"], c["n_mismatched"]) == (2 * N_READS, mp.pl.counts()["n_placed"], want[4]) and want[4] == 0
        assert np.array_equal(got[1], locus[placed])
        assert np.array_equal(np.flatnonzero(np.diff(got[0].astype(np.int64))), 2 * np.flatnonzero(placed) + strand[placed])
        for e, i in enumerate(np.flatnonzero(placed)):        # every script replays: the read, or its reverse complement, against the text
            q = mp.ranks[int(mp.roff[i]):int(mp.roff[i + 1])]
            q = fn.revcomp(q, COMPLEMENT[sigma], sigma) if strand[i] else q
            runs = got[3][int(got[2][e]):int(got[2][e + 1])]
            assert sn.replay(q, text[int(p_start[i]):int(p_end[i])], runs, sigma) == (int(dist[locus[i]]), True), i
        cigars = mp.pl.cigars(scr)
        assert len(cigars) == N_READS and [bool(s) for s in cigars] == placed.tolist()
        assert [s for s in cigars if s] == sn.strings(want[2], want[3])
        # scratch_bytes changes nothing, in the handle of the call before
        same(names, mp.pl.scripts(idx, mp.reads, mp.loci, mp.al, scratch_bytes=1, scripts=scr).host(), want[:4])
        want_m = sn.scripts(text, ranks2, roff2, mp.h_loci[0], dist, start, end, best2, sigma, False, True)
        same(names, mp.pl.scripts(idx, mp.reads, mp.loci, mp.al, m=True, scripts=scr).host(), want_m[:4])
        o = engine.ScriptOptions(C.sizeof(engine.ScriptOptions), engine.SCRIPT_ALL, 0)
        st = engine.lib().kmx_placements_scripts(idx._h, mp.reads._h, mp.loci._h, mp.al._h, mp.pl._h, C.byref(o), C.byref(scr._h))
        assert st == 1 and b"KMX_SCRIPT_ALL" in engine.lib().kmx_last_error()
    finally:
        scr.close()


# ---- 6. plumbing -----------------------------------------------------------------------------------------------------------------------
def test_bad_complement_tables_are_refused_and_leave_an_empty_batch(engine, small_indexes):
    import torch

    idx = small_indexes[4]
    ranks, roff = strand_batch(4, 10)
    h = idx.strand_reads(ranks, roff, COMPLEMENT[4])
    d_r, d_o = torch.from_numpy(np.array(ranks)).cuda(), torch.from_numpy(np.array(roff).view(np.int64)).cuda()
    torch.cuda.synchronize()
    try:
        for table, word in ((None, "NULL complement"), ([1, 2, 0, 3], "involution"), ([0, 1, 2, 4], "outside the alphabet")):
            assert h.counts()["nr"] == 10
            assert word in refused(engine, lambda: idx.strand_reads(ranks, roff, table, reads=h))
            assert h.counts() == {"nr": 0, "nr2": 0}
            assert word in refused(engine, lambda: idx.strand_reads_device(d_r.data_ptr(), d_o.data_ptr(), 10, table, reads=h))
            idx.strand_reads(ranks, roff, COMPLEMENT[4], reads=h)
        bad = np.array(roff)
        bad[0] = 1
        assert "roff[0]" in refused(engine, lambda: idx.strand_reads(ranks, bad, COMPLEMENT[4], reads=h))
        bad = np.array(roff)
        bad[3] = bad[5]
        assert "non-decreasing" in refused(engine, lambda: idx.strand_reads(ranks, bad, COMPLEMENT[4], reads=h))
        assert "NULL read letters" in refused(engine, lambda: idx.strand_reads(np.zeros(0, np.uint8), roff, COMPLEMENT[4], reads=h))
        assert h.counts()["nr2"] == 0
        L, comp = engine.lib(), np.asarray(COMPLEMENT[4], np.uint8)
        assert L.kmx_reads_strands(None, ranks.ctypes.data, roff.ctypes.data, 10, comp.ctypes.data, C.byref(h._h)) == 1
        assert L.kmx_reads_strands(idx._h, ranks.ctypes.data, roff.ctypes.data, 10, comp.ctypes.data, None) == 1
        assert L.kmx_reads_strands(idx._h, ranks.ctypes.data, roff.ctypes.data, 1 << 30, comp.ctypes.data, C.byref(h._h)) == 5
        assert L.kmx_strand_reads_view_device(None, None, None, None, None) == 1
    finally:
        h.close()


def test_fold_refusals_leave_an_empty_result(engine, repeat_index):
    text, _ = repeat_text()
    idx, L = repeat_index, engine.lib()
    four = pack([text[100:170].copy(), text[300:390].copy(), text[2000:2100].copy(), text[500:600].copy()])    # two loci more than `two` doubled
    two = pack([text[100:170].copy(), text[2000:2100].copy()])
    two_b = pack([text[100:170].copy(), text[300:390].copy()])
    kw = dict(band=0, min_votes=8, max_edits=4)                # (no locus of a chance match of 11 letters)
    mp = Mapped(idx, 4, *two, 10, **kw)
    held = []
    try:
        loci3, al3 = idx.map_reads(*pack([text[100:170].copy()] * 3), 10, **kw)
        loci4, al4 = idx.map_reads(*four, 10, **kw)
        loci2, al2 = idx.map_reads(*two_b, 10, **kw)
        held += [loci3, al3, loci4, al4, loci2, al2]
        pl = mp.pl
        assert pl.counts()["n_placed"] == 2
        for call, word in ((lambda: al3.fold_strands(loci3, placements=pl), "odd"),
                           (lambda: al2.fold_strands(loci4, placements=pl), "nr differs"),
                           (lambda: al4.fold_strands(loci2, placements=pl), "nr differs"),
                           (lambda: mp.al.fold_strands(loci4, placements=pl), "n_loci differs")):
            al4.fold_strands(loci4, placements=pl)
            assert pl.counts()["nr"] == 2
            assert word in refused(engine, call)
            assert pl.counts() == {"nr": 0, "n_placed": 0, "n_reverse": 0, "n_ambiguous": 0}
            assert all(x.size == 0 for x in pl.host()) and pl.device_ptrs() == (None,) * 7
        assert loci4.counts()["nr"] == 4 and loci4.counts()["n_loci"] != mp.loci.counts()["n_loci"]
        # before any handle is looked at: the result stays
        al4.fold_strands(loci4, placements=pl)
        good = engine.FoldOptions(C.sizeof(engine.FoldOptions), 0)
        for o in (engine.FoldOptions(C.sizeof(engine.FoldOptions), 1), engine.FoldOptions(C.sizeof(engine.FoldOptions) - 1, 0)):
            assert L.kmx_alignments_fold_strands(loci4._h, al4._h, C.byref(o), None, C.byref(pl._h)) == 1
        assert L.kmx_alignments_fold_strands(None, al4._h, C.byref(good), None, C.byref(pl._h)) == 1
        assert L.kmx_alignments_fold_strands(loci4._h, None, C.byref(good), None, C.byref(pl._h)) == 1
        assert L.kmx_alignments_fold_strands(loci4._h, al4._h, None, None, C.byref(pl._h)) == 1
        assert L.kmx_alignments_fold_strands(loci4._h, al4._h, C.byref(good), None, None) == 1
        assert L.kmx_placements_counts(None, None, None, None, None) == 1
        assert L.kmx_placements_view(None, *[None] * 7) == 1 and L.kmx_placements_view_device(None, *[None] * 7) == 1
        assert pl.counts()["nr"] == 2
        # the scripts call: placements of another batch, NULL handles
        so = engine.ScriptOptions(C.sizeof(engine.ScriptOptions), 0, 0)
        scr = engine.Scripts()
        held.append(scr)
        al2.fold_strands(loci2, placements=pl)                # one public read: not the placements of mp's two
        assert "nr differs" in refused(engine, lambda: pl.scripts(idx, mp.reads, mp.loci, mp.al, scripts=scr))
        assert L.kmx_placements_scripts(idx._h, None, mp.loci._h, mp.al._h, pl._h, C.byref(so), C.byref(scr._h)) == 1
        assert L.kmx_placements_scripts(idx._h, mp.reads._h, mp.loci._h, mp.al._h, None, C.byref(so), C.byref(scr._h)) == 1
        assert L.kmx_placements_scripts(idx._h, mp.reads._h, mp.loci._h, mp.al._h, pl._h, None, C.byref(scr._h)) == 1
    finally:
        for h in held:
            h.close()
        mp.close()


def test_handles_are_reused_views_agree_and_inputs_stay(work):
    name = "dna4_k10"
    sigma, k, n, _ = WORKLOADS[name]
    mp, idx = work.workload(name), work.index(name)
    ptrs = (mp.loci.device_ptrs(), mp.al.device_ptrs())
    # one placements handle for batches of different sizes, on the stream of each
    small = Mapped(idx, sigma, *pack([text_of(sigma, n)[500:650].copy(), fn.revcomp(text_of(sigma, n)[900:1000], COMPLEMENT[4], 4)]), k, **CHAIN)
    try:
        pl = small.pl
        assert pl.counts() == {"nr": 2, "n_placed": 2, "n_reverse": 1, "n_ambiguous": 0}
        mp.al.fold_strands(mp.loci, placements=pl)
        check_fold(pl, mp.h_loci, mp.h_al)
        dv = pl.device_ptrs()
        dts = (np.uint32, np.uint8, np.uint8, np.uint32, np.uint32, np.uint8, np.uint32)
        same(FOLD, [dev_array(p, (2 if x == "best2" else 1) * N_READS, d) for p, d, x in zip(dv, dts, FOLD)], pl.host())
        assert len(pl.host(best2=False)) == 6
        small.al.fold_strands(small.loci, placements=pl)
        check_fold(pl, small.h_loci, small.h_al)
        scr = mp.pl.scripts(idx, mp.reads, mp.loci, mp.al)
        scr.close()
    finally:
        small.close()
    assert ptrs == (mp.loci.device_ptrs(), mp.al.device_ptrs())
    same(LOCI, mp.loci.host(), mp.h_loci)
    same(ALIGN, mp.al.host(), mp.h_al)
    # map_reads is what it was: the two calls it is made of
    ranks, roff = reads_of(name)
    loci, al = idx.map_reads(ranks, roff, k, **CHAIN)
    loci2 = idx.vote_windows(ranks, roff, k, 1, CHAIN["band"], CHAIN["min_votes"], 0)
    al2 = loci2.align(idx, ranks, roff, CHAIN["max_edits"], CHAIN["max_span"])
    try:
        same(LOCI, loci.host(), loci2.host())
        same(ALIGN, al.host(), al2.host())
        assert loci.counts()["nr"] == N_READS
    finally:
        for h in (al2, loci2, al, loci):
            h.close()
