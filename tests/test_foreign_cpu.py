"""Handles of different batches through the oracles alone, without a device: the batches of tests/foreign_data.py through the naive chain
(tests/chain_naive.py), and the mixed combinations of tests/test_foreign_gpu.py through tests/pileup_naive.py, tests/clip_naive.py
and tests/realign_naive.py.  What is asserted are properties of the inputs: every cause that genuine handles can reach occurs in
at least FLOOR entries of the combination meant for it, and in every mixed pileup call at least a quarter of the entries still are
ADDED (a call where everything is MISMATCHED would hide a kernel that adds nothing).  The GPU tests assert the same floors on the
engine's own handles.

Two floors are below FLOOR by construction.  D has exactly two decreasing ranges, so `roff` is reached twice.  The rescue form
has six entries (a batch of 96 internal reads holds six rescued mates): three are ADDED, two reach `bound`, one `text_len`.

The causes that genuine handles cannot reach are shown here on the oracle alone (the last tests): no read r for an entry, an op
other than = X I D S, the letters that end in front of a read, and for the realignment a read above MAX_READ and sel[e] at or past
the number of loci (the call refuses scripts with more entries than the alignments have loci; these batches have a locus per
entry)."""
import functools

import numpy as np

from tests import chain_naive as ch
from tests import clip_naive as cn
from tests import foreign_data as fd
from tests import mapq_naive as mqn
from tests import pileup_naive as pn
from tests import realign_naive as rn
from tests.chain_data import CHAIN as PAIR_CHAIN, COMP4, INSERT, K, LETTERS4, N, PAIR_WORKLOADS, clip_text, text_of
from tests.helpers import pack

FLOOR = 5


@functools.lru_cache(maxsize=None)
def world():
    """the batches through the naive chain, by name: (reads, loci, alignments, placements, scripts, tags)"""
    t = clip_text()
    run = lambda reads, opt: ch.strands(t, 4, *pack(list(reads)), K, COMP4, LETTERS4, **opt)
    return dict(A=run(fd.batch_a()[0], fd.CHAIN), B=run(fd.batch_b(), fd.CHAIN), C=run(fd.batch_c(), fd.CHAIN), S=run(fd.batch_b(), fd.STRICT))


def clips_of(sc, **opt):
    return cn.clip(sc.arrays[2], sc.arrays[3], **dict(cn.DEFAULTS, **opt))[:9]


def pile(sc, cl, al, ranks, roff, n=N, lo=0, hi=None, counts=None, **opt):
    """(planes, counters, tally of the causes, why) of one oracle call"""
    hi = n if hi is None else hi
    why = {}
    counts = pn.planes(lo, hi, 4) if counts is None else counts.copy()
    out = pn.add(counts, lo, hi, 4, sc.arrays, cl, al.arrays[1], al.arrays[2], ranks, roff, n=n, why=why, **opt)
    return counts, out, fd.tally(why), why


def quarter(out, n_entries):
    assert 4 * out["n_added"] >= n_entries and out["n_added"] + out["n_mismatched"] + out["n_filtered"] == n_entries, out


# ---- 1. the batches -------------------------------------------------------------------------------------------------------------------------
def test_the_batches_are_what_the_module_says():
    reads, meta = fd.batch_a()
    t = clip_text()
    m = [q.size for q in reads]
    assert len(reads) == 48 and min(m) >= 40 and max(m) <= 150 and len(set(m)) >= 20                       # lengths varied on purpose
    subs = sum(1 for k in meta if k[0] in (0, 1, 2) and k[3] > 0)
    assert 14 <= subs <= 20 and all(1 <= k[3] <= 3 for k in meta if k[3]) and sum(k[0] == 3 for k in meta) == sum(k[0] == 4 for k in meta) == 2
    for i, (q, (kind, s, mm, edits)) in enumerate(zip(reads, meta)):
        assert q.size == mm and q.max() < 4
        if edits == 0 and i not in fd.RC:
            assert np.array_equal(q, t[s:s + mm])
    assert [q.tobytes() for q in fd.batch_b()] == [q.tobytes() for q in reads[::-1]] and len(fd.batch_c()) == 16
    w = world()
    for name, nr in (("A", 48), ("B", 48), ("S", 48), ("C", 16)):
        _, loci, al, pl, sc, _ = w[name]
        assert loci.totals["n_loci"] == nr and sc.totals["n_sel"] == (al.totals["n_aligned"] if name != "S" else sc.totals["n_sel"])
        assert sc.totals["n_mismatched"] == 0 and (name == "S" or np.array_equal(sc.arrays[1], np.arange(nr)))
    assert w["S"][2].totals["n_aligned"] < 48 and int((w["S"][2].arrays[0] == 255).sum()) >= FLOOR
    # same n_sel, same n_loci, intervals that do not fit
    a, b = w["A"][2].arrays, w["B"][2].arrays
    assert int(((a[2].astype(int) - a[1]) != (b[2].astype(int) - b[1])).sum()) >= FLOOR
    # N_SHORT lies in the middle of A's placements
    assert int((a[2] <= fd.N_SHORT).sum()) == 24 and int((a[1] >= fd.N_SHORT).sum()) == 23 and a[1][12] < fd.N_SHORT < a[2][12]      # read 12 lies across it


def test_the_moved_roff_stays_inside_the_letters_and_has_two_decreasing_ranges():
    ranks2, roff2 = world()["A"][0].arrays
    moved = fd.moved_roff(roff2).astype(np.int64)
    step = np.diff(moved)
    assert moved.size == roff2.size and moved.min() >= 0 and moved.max() <= ranks2.size and not (moved == roff2.astype(np.int64)).any()
    assert int((step < 0).sum()) == 2 and int((step != np.diff(roff2.astype(np.int64))).sum()) >= 2 * len(fd.LONGER)
    read_sel_off = world()["A"][4].arrays[0].astype(np.int64)
    for i in fd.DECREASING:                                    # the decreasing range is that of a read with an entry
        assert step[2 * i] < 0 and read_sel_off[2 * i + 1] - read_sel_off[2 * i] == 1


# ---- 2. the pileup --------------------------------------------------------------------------------------------------------------------------
def test_every_mixed_pileup_combination_reaches_its_cause_and_keeps_a_quarter():
    w = world()
    (_, (ranks2, roff2), _), _, al, _, sc, _ = w["A"]
    harsh, harsh_b = clips_of(sc, **fd.HARSH), clips_of(w["B"][4], **fd.HARSH)
    _, out, seen, _ = pile(sc, None, al, ranks2, roff2)
    assert out["n_added"] == 48 and seen[None] == 48
    _, out, seen, _ = pile(sc, None, w["C"][2], ranks2, roff2)
    quarter(out, 48)
    assert seen["bound"] == 32 and out["n_added"] == 16
    for cl in (None, clips_of(sc)):
        for name in ("B", "S"):
            _, out, seen, _ = pile(sc, cl, w[name][2], ranks2, roff2)
            quarter(out, 48)
            assert seen["text_len"] >= FLOOR and seen["read_len"] == seen["bound"] == 0
        _, out, seen, _ = pile(sc, cl, w["C"][2], ranks2, roff2)
        assert seen["bound"] == 32 and out["n_added"] == 16
        _, out, seen, _ = pile(sc, cl, al, ranks2, roff2, n=fd.N_SHORT)
        assert seen["interval"] == 24 and out["n_added"] == 24
        _, out, seen, _ = pile(sc, cl, al, ranks2, fd.moved_roff(roff2))
        quarter(out, 48)
        assert seen["read_len"] >= FLOOR and seen["roff"] == 2 and seen["text_len"] == 0
    _, out, seen, _ = pile(sc, harsh, w["B"][2], ranks2, roff2)
    quarter(out, 48)
    assert seen["clip"] >= FLOOR and seen["text_len"] >= FLOOR
    _, out, seen, why = pile(sc, harsh_b, al, ranks2, roff2)
    quarter(out, 48)
    assert seen["text_len"] >= FLOOR and seen["read_len"] >= FLOOR
    assert sum(1 for v in why.values() if v == ["text_len"]) >= 2                # the text side alone: the gapped pairs
    _, out, seen, why = pile(sc, None, al, ranks2, roff2, n=fd.N_SHORT)
    quarter(out, 48)
    assert seen["interval"] == 24 and all((not v) == (int(al.arrays[2][e]) <= fd.N_SHORT) for e, v in why.items())
    _, out, seen, _ = pile(sc, None, al, ranks2, fd.moved_roff(roff2))
    quarter(out, 48)
    assert seen["read_len"] >= FLOOR and seen["roff"] == 2 and seen["text_len"] == 0                 # the read side alone
    _, out, seen, _ = pile(sc, None, w["S"][2], ranks2, roff2)
    quarter(out, 48)
    assert seen["text_len"] >= FLOOR


def test_filters_win_over_the_mismatch_and_a_region_cuts_added_entries():
    w = world()
    (_, (ranks2, roff2), _), _, al, _, sc, _ = w["A"]
    pl = w["A"][3].arrays
    mapq = mqn.mapq(pl[1], pl[2], pl[5], fd.CHAIN["max_edits"], per_edit=2)[0]   # 2 (25 - dist): below the cap, so the edits show
    assert sorted(set(mapq.tolist())) == [44, 46, 48, 50]
    score = clips_of(sc)[0]
    cut = int(np.sort(score)[24])
    low = clips_of(sc, min_score=cut)
    assert 0 < int((low[6] & 1).sum()) < 48
    _, _, _, why0 = pile(sc, low, w["B"][2], ranks2, roff2, mapq=mapq)
    bad0 = {e for e, v in why0.items() if v}
    for opt in (dict(min_mapq=47), dict(min_score=cut), dict(skip_low=True), dict(min_mapq=47, min_score=cut, skip_low=True)):
        _, out, _, why = pile(sc, low, w["B"][2], ranks2, roff2, mapq=mapq, **opt)
        filtered = set(range(48)) - set(why)
        assert out["n_filtered"] == len(filtered) and out["n_filtered"] + out["n_mismatched"] + out["n_added"] == 48
        assert len(bad0 & filtered) >= 2 and out["n_mismatched"] == len(bad0 - filtered) and out["n_added"] >= 2, (opt, out)
        assert len(opt) > 1 or out["n_mismatched"] >= 2, (opt, out)          # a single filter leaves some of them MISMATCHED
    # a region that cuts ADDED entries of the mixed call: the slice of the whole
    full, whole_out, _, why = pile(sc, None, w["B"][2], ranks2, roff2)
    start, end = w["B"][2].arrays[1:3]
    e = next(e for e, v in why.items() if not v and end[e] - start[e] >= 100)
    lo, hi = int(start[e]) + 30, int(end[e]) + 2000
    part, out, _, _ = pile(sc, None, w["B"][2], ranks2, roff2, lo=lo, hi=hi)
    assert np.array_equal(part, full[:, lo:hi]) and out["n_added"] == whole_out["n_added"] and 0 < out["n_cells"] < whole_out["n_cells"]
    assert part[:4, 0].sum() >= 1 and any(int(start[x]) < hi < int(end[x]) or int(start[x]) < lo < int(end[x]) for x, v in why.items() if not v)


def test_the_rescue_form_with_the_jobs_of_another_batch():
    sigma, k, n = PAIR_WORKLOADS["dna4_k10"]
    txt = text_of(sigma, n)
    p, q = (ch.pairs(txt, sigma, *b, k, COMP4, LETTERS4, **INSERT, **PAIR_CHAIN) for b in fd.rescue_batches())
    assert p[0].arrays[1].size - 1 == 96 and (p[6].totals["n_jobs"], q[6].totals["n_jobs"]) == (18, 12)
    rsc = p[7].rescue_scripts
    assert rsc.totals["n_sel"] == 6
    for cl in (None, clips_of(rsc)):
        why = {}
        out = pn.add(pn.planes(0, n, 4), 0, n, 4, rsc.arrays, cl, q[6].arrays[5], q[6].arrays[6], *p[0].arrays, n=n, why=why)
        seen = fd.tally(why)
        quarter(out, 6)
        assert seen["bound"] == 2 and seen["text_len"] >= 1


# ---- 3. the clipped MD ------------------------------------------------------------------------------------------------------------------------
def test_the_clipped_md_counts_the_foreign_entries():
    w = world()
    _, _, al, _, sc, _ = w["A"]
    t = clip_text()
    sel = sc.arrays[1]
    harsh, harsh_b = clips_of(sc, **fd.HARSH), clips_of(w["B"][4], **fd.HARSH)
    md = lambda cl, a, txt=t: cn.md(sel, cl[7], cl[8], cl[3], cl[4], a.arrays[1], a.arrays[2], txt, LETTERS4)
    clean = md(harsh, al)
    assert clean[2] == 0
    assert md(harsh, w["C"][2])[2] == 32
    assert FLOOR <= md(harsh, w["B"][2])[2] <= 36 and FLOOR <= md(harsh_b, al)[2] <= 36
    assert md(harsh, al, t[:fd.N_SHORT])[2] == 24
    # tl + tr > end - start alone, among them
    a, b = w["B"][2].arrays[1:3]
    assert int(((harsh[3].astype(int) + harsh[4]) > (b.astype(int) - a)).sum()) >= FLOOR


# ---- 4. the realignment -----------------------------------------------------------------------------------------------------------------------
def real(al, ranks, roff, txt, sc=None):
    sc = world()["A"][4] if sc is None else sc
    why = {}
    out = rn.realign(*sc.arrays, al.arrays[0], al.arrays[1], al.arrays[2], ranks, roff, txt, 4, why=why, **rn.DEFAULTS)
    return out, fd.tally(why), why


def guarded_are_whole(out, why, sc):
    want = clips_of(sc, min_score=2 ** 31 - 1)                 # what kmx_scripts_clip makes of a LOW entry
    for e, v in why.items():
        if v:
            assert out[6][e] == rn.LOW and all(int(out[k][e]) == int(want[k][e]) for k in range(7)), e
            assert np.array_equal(out[8][int(out[7][e]):int(out[7][e + 1])], want[8][int(want[7][e]):int(want[7][e + 1])]), e


def test_every_mixed_realignment_guards_five_entries_and_realigns_five():
    w = world()
    (_, (ranks2, roff2), _), _, al, _, sc, _ = w["A"]
    t = clip_text()
    clean, seen, _ = real(al, ranks2, roff2, t)
    assert seen[None] == 48 and int((clean[6] == rn.REALIGNED).sum()) == 48
    rows = (("B", w["B"][2], ranks2, roff2, t, "gap"), ("S", w["S"][2], ranks2, roff2, t, "dist"), ("D", al, ranks2, fd.moved_roff(roff2), t, "gap"),
            ("short", al, ranks2, roff2, t[:fd.N_SHORT], "interval"))
    for name, a, ranks, roff, txt, cause in rows:
        out, seen, why = real(a, ranks, roff, txt)
        n_guarded = sum(bool(v) for v in why.values())
        passed = [e for e, v in why.items() if not v]
        assert seen[cause] >= FLOOR and n_guarded >= FLOOR and int((out[6][passed] == rn.REALIGNED).sum()) >= FLOOR, (name, seen)
        guarded_are_whole(out, why, sc)
        if name in ("B", "D"):                                 # realigned on other letters: not the clean result
            assert sum(1 for e in passed if out[6][e] == rn.REALIGNED and (out[0][e], out[1][e], out[3][e]) != (clean[0][e], clean[1][e], clean[3][e])) >= FLOOR
        if name == "D":
            assert seen["roff"] == 2
        if name == "short":
            assert all(np.array_equal(out[k][passed], clean[k][passed]) for k in range(7))


# ---- 5. the causes that genuine handles cannot reach ------------------------------------------------------------------------------------------
def test_the_unreachable_guards_of_the_realignment_on_the_oracle():
    w = world()
    (_, (ranks2, roff2), _), _, al, _, sc, _ = w["A"]
    t = clip_text()
    dist, start, end = (a.copy() for a in al.arrays[:3])
    read_sel_off, sel, cig_off, cigar = sc.arrays
    base = dict(read_sel_off=read_sel_off, sel=sel, dist=dist, start=start, end=end, ranks=ranks2, roff=roff2, n_loci=None)

    def causes(**kw):
        a = dict(base, **kw)
        why = {}
        out = rn.realign(a["read_sel_off"], a["sel"], cig_off, cigar, a["dist"], a["start"], a["end"], a["ranks"], a["roff"], t, 4, n_loci=a["n_loci"], why=why,
                         **rn.DEFAULTS)
        guarded_are_whole(out, why, sc)
        return why

    assert not any(causes().values())
    assert causes(read_sel_off=np.zeros_like(read_sel_off))[0] == ["no_read"]
    assert causes(n_loci=3)[3] == ["locus"] and causes(n_loci=3)[2] == []
    d = dist.copy()
    d[4] = rn.MAX_EDITS + 1
    assert causes(dist=d)[4] == ["dist"] and causes(dist=d)[5] == []
    long_roff = np.asarray([0, rn.MAX_READ + 1] + [rn.MAX_READ + 1] * (roff2.size - 2), np.uint64)
    e0 = int(np.flatnonzero(np.diff(read_sel_off.astype(np.int64)))[0])
    assert e0 == 0 and causes(ranks=np.zeros(rn.MAX_READ + 1, np.uint8), roff=long_roff)[0] == ["long_read"]
    s = start.copy()
    s[7] = end[7] + 1
    assert causes(start=s)[7] == ["interval"]
    assert causes(roff=np.asarray([5, 0] + roff2[2:].tolist(), np.uint64))[0] == ["roff"]


def test_the_unreachable_causes_of_the_pileup_on_the_oracle():
    w = world()
    (_, (ranks2, roff2), _), _, al, _, sc, _ = w["A"]
    read_sel_off, sel, cig_off, cigar = sc.arrays
    why = {}
    none = (np.zeros_like(read_sel_off), sel, cig_off, cigar)
    out = pn.add(pn.planes(0, N, 4), 0, N, 4, none, None, al.arrays[1], al.arrays[2], ranks2, roff2, n=N, why=why)
    assert out["n_mismatched"] == 48 and fd.tally(why)["no_read"] == 48
    joined = cigar.copy()
    joined[0] = (joined[0] & ~np.uint32(15)) | 0               # an M run
    why = {}
    out = pn.add(pn.planes(0, N, 4), 0, N, 4, (read_sel_off, sel, cig_off, joined), None, al.arrays[1], al.arrays[2], ranks2, roff2, n=N, why=why)
    assert out["n_mismatched"] == 1 and why[0] == ["op"]
    # the letters that were handed over end in front of the last read: its range is not one
    why = {}
    r = int(np.flatnonzero(np.diff(read_sel_off.astype(np.int64)))[-1])       # the last read with an entry
    out = pn.add(pn.planes(0, N, 4), 0, N, 4, sc.arrays, None, al.arrays[1], al.arrays[2], ranks2[:int(roff2[r + 1]) - 1], roff2, n=N, why=why)
    assert out["n_mismatched"] == 1 and why[47] == ["roff"]
