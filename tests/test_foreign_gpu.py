"""Handles of different batches on the GPU: the guards of kmx_clips_pileup_device / kmx_clips_rescues_pileup (k_pileup_check), of
kmx_clips_md and of kmx_scripts_realign[_device] (entry_of, kmx_script_core.h) with a guard actually firing.  include/kmx.h promises
for every one of them that handles which do not belong together give a defined result (MISMATCHED and counted, or whole and LOW) and
that every access stays inside its array.  The batches are those of tests/foreign_data.py (A, its reversal B, its first 16 reads C,
the moved roff D, the short index, B aligned strictly, and two batches of pairs for the rescue form); no batch has more than 96
internal reads.  The oracle is always applied to the host views of exactly the handles that the call was given (tests/pileup_naive.py,
tests/clip_naive.py, tests/realign_naive.py), and every array, dtype and counter must be identical.  The floors that
tests/test_foreign_cpu.py shows on the naive chain are asserted again here, on the engine's own handles: every cause in at least FLOOR
entries of the combination meant for it (`roff` twice: D has exactly two decreasing ranges; the rescue form has six entries in all),
and at least a quarter of the entries of every mixed pileup call still ADDED.

Every input stays inside its allocations: the moved roff points nowhere past the letters that are handed over, and no test is meant to
make a kernel fault.  A wrong guard shows as a wrong number.

Causes that genuine handles cannot reach stay with the oracle (tests/test_foreign_cpu.py, tests/test_pileup_cpu.py): no read r for an
entry (an nr that differs from the scripts' is refused); an op other than = X I D S or an inner S (scripts made with KMX_SCRIPT_M are
refused, and no call makes the others); the letters bound of the StrandReads form (a StrandReads is consistent with itself); a read
above KMX_ALIGN_MAX_READ (the aligner takes none, so there is no entry); sel[e] >= n_loci in the realignment (scripts with more
entries than the alignments have loci are refused, and these batches have one locus per entry).  Nothing here writes into private
memory to fake them."""
import numpy as np
import pytest

from tests import foreign_data as fd
from tests import realign_naive as rn
from tests.chain_checks import (check_clip_md, check_pileup, check_realign, close_all, doubled, pileup_want, same, snapshot, untouched)
from tests.chain_data import CHAIN as PAIR_CHAIN, CLIPS, COMP4, INSERT, K, LETTERS4, N, PAIR_WORKLOADS, clip_text as text, text_of
from tests.helpers import pack

pytestmark = pytest.mark.gpu

FLOOR = 5


def plus(a, b):
    return {k: a[k] + b[k] for k in a}


@pytest.fixture(scope="module")
def index(engine):
    idx = engine.Index(text(), 4, [K], table=2)
    yield idx
    idx.close()


@pytest.fixture(scope="module")
def short(engine):
    idx = engine.Index(text()[:fd.N_SHORT].copy(), 4, [K], table=2)
    yield idx
    idx.close()


@pytest.fixture(scope="module")
def world(index):
    """A, B, C and S (B aligned strictly) through the chain: name -> (reads, loci, alignments, placements, scripts)"""
    out = {}
    for name, reads, opt in (("A", fd.batch_a()[0], fd.CHAIN), ("B", fd.batch_b(), fd.CHAIN), ("C", fd.batch_c(), fd.CHAIN), ("S", fd.batch_b(), fd.STRICT)):
        out[name] = index.map_reads_strands(*pack(list(reads)), K, COMP4, **opt, scripts=True)
    a = out["A"]
    assert a[0].counts()["nr2"] == 96 and a[4].counts()["n_sel"] == a[2].counts()["n_loci"] == out["B"][2].counts()["n_loci"] == 48
    assert out["B"][4].counts()["n_sel"] == 48 and out["C"][2].counts()["n_loci"] == 16 and out["S"][2].counts()["n_loci"] == 48
    yield out
    for handles in out.values():
        close_all(list(handles))


@pytest.fixture(scope="module")
def clips(world):
    """the clips of A and of B that keep one '=' run (fd.HARSH), and the default clips of A"""
    out = dict(A=world["A"][4].clip(**fd.HARSH), B=world["B"][4].clip(**fd.HARSH), plain=world["A"][4].clip())
    yield out
    close_all(list(out.values()))


def mixed(index, sc, cl, al, reads, pu, n=N, lo=0, hi=None, roff=None, d_roff=None, mapq=None, **flt):
    """One mixed combination through every entry point that serves these handles (Scripts.pileup or Clips.pileup over the StrandReads,
    and the device form; with `roff` / `d_roff`, the moved offsets, the device form alone), each against the oracle on the host views
    of the same handles.  Returns (planes, counters, the tally of the causes, why)."""
    ranks2, roff2 = doubled(reads)
    d_ranks2, d_roff2, nr2, stream = reads.device_ptrs()
    why = {}
    counts, ctr = pileup_want(sc, cl, al, ranks2, roff2 if roff is None else roff, lo, n if hi is None else hi, n, mapq=None if mapq is None else mapq.host(),
                              why=why, **flt)
    held = [h for h in (sc, cl, al) if h is not None]
    before = snapshot(*held)
    calls = [lambda **kw: sc.pileup_device(index, al, d_ranks2, d_roff2 if d_roff is None else d_roff, nr2, clips=cl, stream=stream, **kw)]
    if roff is None:
        calls.append((lambda **kw: sc.pileup(index, al, reads, **kw)) if cl is None else (lambda **kw: cl.pileup(index, sc, al, reads, **kw)))
    for call in calls:
        assert call(lo=lo, hi=hi, mapq=mapq, pileup=pu, **flt) is pu
        check_pileup(pu, counts, ctr, lo, n if hi is None else hi)
    untouched(before, *held)
    cig_off = (sc if cl is None else cl).host()[-2].astype(np.int64)
    n_entries = int((np.diff(cig_off) > 0).sum())              # the entries with runs
    assert ctr["n_added"] + ctr["n_mismatched"] + ctr["n_filtered"] == n_entries == len(why) + ctr["n_filtered"]
    return counts, ctr, fd.tally(why), why


def quarter(ctr, n_entries=48):
    assert 4 * ctr["n_added"] >= n_entries, ctr


# ---- 1. the pileup: one cause per combination ---------------------------------------------------------------------------------------------------
def test_alignments_of_fewer_reads_the_bound_on_sel(engine, index, world, clips):
    reads, _, al, _, sc = world["A"]
    pu = engine.Pileup()
    try:
        clean, k0, seen, _ = mixed(index, sc, None, al, reads, pu)
        assert k0["n_added"] == 48 and seen[None] == 48
        for cl in (None, clips["plain"]):
            counts, ctr, seen, why = mixed(index, sc, cl, world["C"][2], reads, pu)
            quarter(ctr)
            assert seen["bound"] == 32 and ctr["n_added"] == 16 and all((not v) == (e < 16) for e, v in why.items())
    finally:
        pu.close()


def test_alignments_of_the_reversed_batch_the_text_length(engine, index, world, clips):
    reads, _, al, _, sc = world["A"]
    pu = engine.Pileup()
    try:
        for cl in (None, clips["plain"]):
            for name in ("B", "S"):
                _, ctr, seen, _ = mixed(index, sc, cl, world[name][2], reads, pu)
                quarter(ctr)
                assert seen["text_len"] >= FLOOR and seen["read_len"] == seen["bound"] == 0, (name, seen)
    finally:
        pu.close()


def test_clips_that_cut_more_than_the_foreign_interval_holds(engine, index, world, clips):
    reads, _, al, _, sc = world["A"]
    pu = engine.Pileup()
    try:
        _, ctr, seen, _ = mixed(index, sc, clips["A"], world["B"][2], reads, pu)
        quarter(ctr)
        assert seen["clip"] >= FLOOR and seen["text_len"] >= FLOOR
    finally:
        pu.close()


def test_clips_of_another_batch_both_length_tests(engine, index, world, clips):
    reads, _, al, _, sc = world["A"]
    pu = engine.Pileup()
    try:
        assert clips["B"].counts()["n_sel"] == sc.counts()["n_sel"]
        _, ctr, seen, why = mixed(index, sc, clips["B"], al, reads, pu)
        quarter(ctr)
        assert seen["text_len"] >= FLOOR and seen["read_len"] >= FLOOR and sum(1 for v in why.values() if v == ["text_len"]) >= 2
    finally:
        pu.close()


def test_the_short_index_entries_behind_its_end(engine, index, short, world, clips):
    reads, _, al, _, sc = world["A"]
    pu = engine.Pileup()
    try:
        clean, _, _, _ = mixed(index, sc, None, al, reads, pu)
        end = al.host()[2]
        for cl in (None, clips["plain"]):
            counts, ctr, seen, why = mixed(short, sc, cl, al, reads, pu, n=fd.N_SHORT)
            quarter(ctr)
            assert seen["interval"] == 24 >= FLOOR and all((not v) == (int(end[e]) <= fd.N_SHORT) for e, v in why.items())
        below = int(end[end <= fd.N_SHORT].max())              # the entries wholly below the end still are ADDED, as in the clean call
        assert ctr["n_added"] == 24 and np.array_equal(mixed(short, sc, None, al, reads, pu, n=fd.N_SHORT)[0][:, :below], clean[:, :below])
    finally:
        pu.close()


def test_moved_read_offsets_the_read_length_and_the_decreasing_range(engine, index, world, clips):
    import torch
    reads, _, al, _, sc = world["A"]
    ranks2, roff2 = doubled(reads)
    moved = fd.moved_roff(roff2)
    step = np.diff(moved.astype(np.int64))
    assert int(moved.max()) <= ranks2.size and int((step < 0).sum()) == 2          # inside the letters handed over; two decreasing ranges
    d_moved = torch.from_numpy(moved.view(np.int64)).cuda()
    torch.cuda.synchronize()
    pu = engine.Pileup()
    try:
        for cl in (None, clips["plain"]):
            _, ctr, seen, why = mixed(index, sc, cl, al, reads, pu, roff=moved, d_roff=d_moved.data_ptr())
            quarter(ctr)
            assert seen["read_len"] >= FLOOR and seen["roff"] == 2 and seen["text_len"] == 0
            assert sorted(e for e, v in why.items() if v == ["roff"]) == list(fd.DECREASING)
    finally:
        pu.close()


# ---- 2. the pileup: the order of the rules, accumulation, a region ------------------------------------------------------------------------------
def test_filtered_wins_over_mismatched(engine, index, world):
    reads, _, al, pl, sc = world["A"]
    held = []
    try:
        score = sc.clip().host()[0]
        cut = int(np.sort(score)[24])
        low = sc.clip(min_score=cut)
        mq = pl.mapq(fd.CHAIN["max_edits"], per_edit=2)        # 2 (25 - dist): below the cap, so the edits show
        pu = engine.Pileup()
        held += [low, mq, pu]
        assert 0 < low.counts()["n_low"] < 48 and sorted(set(mq.host().tolist())) == [44, 46, 48, 50]
        _, ctr0, _, why0 = mixed(index, sc, low, world["B"][2], reads, pu, mapq=mq)
        bad0 = {e for e, v in why0.items() if v}
        assert ctr0["n_filtered"] == 0 and len(bad0) >= FLOOR
        for opt in (dict(min_mapq=47), dict(min_score=cut), dict(skip_low=True), dict(min_mapq=47, min_score=cut, skip_low=True)):
            _, ctr, _, why = mixed(index, sc, low, world["B"][2], reads, pu, mapq=mq, **opt)
            filtered = set(range(48)) - set(why)
            assert ctr["n_filtered"] == len(filtered) and ctr["n_filtered"] + ctr["n_mismatched"] + ctr["n_added"] == 48
            assert len(bad0 & filtered) >= 2 and ctr["n_mismatched"] == len(bad0 - filtered) and ctr["n_added"] >= 2, (opt, ctr)
            assert len(opt) > 1 or ctr["n_mismatched"] >= 2, (opt, ctr)
    finally:
        close_all(held)


def test_a_mixed_call_added_onto_the_planes_of_a_clean_one(engine, index, world):
    reads, _, al, _, sc = world["A"]
    ranks2, roff2 = doubled(reads)
    d_ranks2, d_roff2, nr2, stream = reads.device_ptrs()
    pu = engine.Pileup()
    try:
        c1, k1 = pileup_want(sc, None, al, ranks2, roff2)
        total, ctr = c1, k1
        sc.pileup(index, al, reads, pileup=pu)
        check_pileup(pu, c1, k1)
        for name, device_form in (("C", False), ("B", True), ("C", True)):
            foreign = world[name][2]
            if device_form:
                sc.pileup_device(index, foreign, d_ranks2, d_roff2, nr2, add=True, stream=stream, pileup=pu)
            else:
                sc.pileup(index, foreign, reads, add=True, pileup=pu)
            total, k = pileup_want(sc, None, foreign, ranks2, roff2, counts=total)
            ctr = plus(ctr, k)
            assert k["n_mismatched"] >= FLOOR and k["n_added"] >= 12
            check_pileup(pu, total, ctr)
        assert ctr["n_added"] == 48 + 16 + 24 + 16 and ctr["n_mismatched"] == 32 + 24 + 32
        # what C adds are the first 16 entries again: behind them the planes are those of the clean call and of B
        first = int(al.host()[2][:16].max())
        only_b, _ = pileup_want(sc, None, world["B"][2], ranks2, roff2, counts=c1)
        assert np.array_equal(total[:, first:], only_b[:, first:]) and not np.array_equal(total[:, :first], only_b[:, :first])
    finally:
        pu.close()


def test_a_region_that_cuts_added_entries_of_a_mixed_call(engine, index, world):
    reads, _, al, _, sc = world["A"]
    foreign = world["B"][2]
    pu = engine.Pileup()
    try:
        full, k, _, why = mixed(index, sc, None, foreign, reads, pu)
        start, end = foreign.host()[1:3]
        e = next(e for e, v in why.items() if not v and end[e] - start[e] >= 100)
        lo, hi = int(start[e]) + 30, int(end[e]) + 2000
        part, ctr, _, _ = mixed(index, sc, None, foreign, reads, pu, lo=lo, hi=hi)
        assert np.array_equal(part, full[:, lo:hi]) and ctr["n_added"] == k["n_added"] and ctr["n_mismatched"] == k["n_mismatched"]
        assert 0 < ctr["n_cells"] < k["n_cells"] and part[:4, 0].sum() >= 1
        lo, hi = int(start[e]) + 64, int(start[e]) + 65        # one position inside an ADDED entry
        part, ctr, _, _ = mixed(index, sc, None, foreign, reads, pu, lo=lo, hi=hi)
        assert np.array_equal(part, full[:, lo:hi]) and ctr["n_cells"] >= 1
    finally:
        pu.close()


# ---- 3. the rescue form ---------------------------------------------------------------------------------------------------------------------
def test_the_rescue_form_with_the_jobs_of_another_batch(engine):
    sigma, k, n = PAIR_WORKLOADS["dna4_k10"]
    idx = engine.Index(text_of(sigma, n), sigma, [k], table=2)
    held = []
    try:
        batch_p, batch_q = fd.rescue_batches()
        kw = dict(PAIR_CHAIN, **INSERT)
        p = idx.map_pairs(*batch_p, k, COMP4, **kw, scripts=True, rescue=True, clip={})
        held += list(p)
        q = idx.map_pairs(*batch_q, k, COMP4, **kw, scripts=True, rescue=True)
        held += list(q)
        reads, res, rcl, foreign = p[0], p[6], p[8], q[6]
        rsc = rcl.scripts
        held.append(rsc)
        assert reads.counts()["nr2"] == 96 and rsc.counts()["n_sel"] == 6 and foreign.host()[5].size == 12 < res.host()[5].size == 18
        ranks2, roff2 = doubled(reads)
        pu = engine.Pileup()
        held.append(pu)
        before = snapshot(rsc, rcl, res, foreign)
        for cl in (None, rcl):
            own, k0 = pileup_want(rsc, cl, res, ranks2, roff2, 0, n, n)
            assert k0["n_added"] == 6
            why = {}
            counts, ctr = pileup_want(rsc, cl, foreign, ranks2, roff2, 0, n, n, why=why)
            seen = fd.tally(why)
            assert 4 * ctr["n_added"] >= 6 and seen["bound"] == 2 and seen["text_len"] >= 1 and ctr["n_mismatched"] == 3
            got = rsc.pileup(idx, foreign, reads, pileup=pu) if cl is None else cl.pileup(idx, rsc, foreign, reads, pileup=pu)
            assert got is pu
            check_pileup(pu, counts, ctr, 0, n)
            (rsc.pileup(idx, res, reads, add=True, pileup=pu) if cl is None else cl.pileup(idx, rsc, res, reads, add=True, pileup=pu))
            both, k1 = pileup_want(rsc, cl, res, ranks2, roff2, 0, n, n, counts=counts)
            check_pileup(pu, both, plus(ctr, k1), 0, n)
        untouched(before, rsc, rcl, res, foreign)
    finally:
        close_all(held)
        idx.close()


# ---- 4. the clipped MD ----------------------------------------------------------------------------------------------------------------------
def test_clipped_md_over_foreign_alignments_foreign_clips_and_the_short_index(engine, index, short, world, clips):
    _, _, al, _, sc = world["A"]
    t = text()
    sel = sc.host()[1]

    def want_of(cl):
        h = cl.host()
        return dict(sel=sel, cig_off=h[7], cigar=h[8], tl=h[3], tr=h[4])

    md = engine.Md()
    try:
        own = want_of(clips["A"])
        start, end = al.host()[1:3]
        clips["A"].md(index, sc, al, LETTERS4, md=md)
        clean = check_clip_md(md, own, start, end, t)
        assert md.counts()["n_mismatched"] == 0 and all(clean)
        before = snapshot(sc, clips["A"], clips["B"], al, world["B"][2], world["C"][2])
        # fewer loci: sel past the bound; the first 16 entries are A's own
        c = world["C"][2].host()
        clips["A"].md(index, sc, world["C"][2], LETTERS4, md=md)
        got = check_clip_md(md, own, c[1], c[2], t)
        assert md.counts()["n_mismatched"] == 32 and got[:16] == clean[:16] and not any(got[16:])
        # the reversed batch: lengths that do not fit, and tl + tr > end - start
        b = world["B"][2].host()
        clips["A"].md(index, sc, world["B"][2], LETTERS4, md=md)
        got = check_clip_md(md, own, b[1], b[2], t)
        over = (own["tl"].astype(np.int64) + own["tr"]) > (b[2].astype(np.int64) - b[1])
        assert FLOOR <= md.counts()["n_mismatched"] <= 36 and int(over.sum()) >= FLOOR and not any(got[e] for e in np.flatnonzero(over))
        assert sum(1 for s in got if s) >= 12
        # the clips of the reversed batch over the scripts of A
        clips["B"].md(index, sc, al, LETTERS4, md=md)
        got = check_clip_md(md, want_of(clips["B"]), start, end, t)
        assert FLOOR <= md.counts()["n_mismatched"] <= 36 and sum(1 for s in got if s) >= 12
        # the short index: not end <= n
        clips["A"].md(short, sc, al, LETTERS4, md=md)
        got = check_clip_md(md, own, start, end, t[:fd.N_SHORT])
        assert md.counts()["n_mismatched"] == 24
        assert all(got[e] == (clean[e] if end[e] <= fd.N_SHORT else "") for e in range(48))
        untouched(before, sc, clips["A"], clips["B"], al, world["B"][2], world["C"][2])
    finally:
        md.close()


# ---- 5. the realignment ---------------------------------------------------------------------------------------------------------------------
def realign_oracle(sc, al, ranks, roff, txt):
    why = {}
    dist, start, end = al.host()[:3]
    return rn.realign(*sc.host(), dist, start, end, ranks, roff, txt, 4, why=why, **rn.DEFAULTS), why


def realign_floors(out, why, sc, cause):
    """the guarded entries are whole and LOW; at least FLOOR of them (and of `cause`), and at least FLOOR of the others are realigned"""
    seen = fd.tally(why)
    guarded = sorted(e for e, v in why.items() if v)
    passed = sorted(e for e, v in why.items() if not v)
    whole = sc.strings()
    assert len(guarded) >= FLOOR and seen[cause] >= FLOOR, seen
    assert all(out["cflags"][e] == rn.LOW and out["strings"][e] == whole[e] and not any(out[k][e] for k in ("sl", "sr", "tl", "tr")) for e in guarded)
    assert int((out["cflags"][passed] == rn.REALIGNED).sum()) >= FLOOR
    return seen, guarded, passed


def test_realign_device_with_foreign_alignments_moved_reads_and_the_short_index(engine, index, short, world):
    import torch
    reads, _, al, _, sc = world["A"]
    ranks2, roff2 = doubled(reads)
    d_ranks2, d_roff2, nr2, stream = reads.device_ptrs()
    moved = fd.moved_roff(roff2)
    assert int(moved.max()) <= ranks2.size
    d_moved = torch.from_numpy(moved.view(np.int64)).cuda()
    torch.cuda.synchronize()
    t = text()
    cl = engine.Clips()
    try:
        sc.realign_device(index, al, d_ranks2, d_roff2, nr2, stream=stream, clips=cl)
        want, why = realign_oracle(sc, al, ranks2, roff2, t)
        clean = check_realign(cl, sc, want)
        assert not any(why.values()) and (clean["cflags"] == rn.REALIGNED).all()
        before = snapshot(sc, al, world["B"][2], world["S"][2])
        rows = (("B", index, world["B"][2], roff2, d_roff2, t, "gap"), ("S", index, world["S"][2], roff2, d_roff2, t, "dist"),
                ("D", index, al, moved, d_moved.data_ptr(), t, "gap"), ("short", short, al, roff2, d_roff2, t[:fd.N_SHORT], "interval"))
        for name, idx, a, roff, d_roff, txt, cause in rows:
            sc.realign_device(idx, a, d_ranks2, d_roff, nr2, stream=stream, clips=cl)
            want, why = realign_oracle(sc, a, ranks2, roff, txt)
            out = check_realign(cl, sc, want)
            seen, guarded, passed = realign_floors(out, why, sc, cause)
            moved_on = [e for e in passed if out["cflags"][e] == rn.REALIGNED and (out["score"][e], out["sl"][e], out["tl"][e]) !=
                        (clean["score"][e], clean["sl"][e], clean["tl"][e])]
            if name in ("B", "D"):                             # realigned on other letters: not the clean result
                assert len(moved_on) >= FLOOR, name
            if name == "D":
                assert seen["roff"] == 2 and sorted(e for e, v in why.items() if v == ["roff"]) == list(fd.DECREASING)
            if name == "short":
                assert seen["interval"] == 24 and not moved_on and all(np.array_equal(out[k][passed], clean[k][passed]) for k in CLIPS[:7])
        untouched(before, sc, al, world["B"][2], world["S"][2])
    finally:
        cl.close()


def test_realign_host_form_with_the_alignments_of_the_reversed_batch(engine, index, world):
    reads, _, al, _, sc = world["A"]
    ranks2, roff2 = doubled(reads)
    d_ranks2, d_roff2, nr2, stream = reads.device_ptrs()
    held = []
    try:
        for name, cause in (("B", "gap"), ("S", "dist")):
            foreign = world[name][2]
            cl = sc.realign(index, foreign, ranks2, roff2)
            held.append(cl)
            want, why = realign_oracle(sc, foreign, ranks2, roff2, text())
            realign_floors(check_realign(cl, sc, want), why, sc, cause)
            apart = sc.realign_device(index, foreign, d_ranks2, d_roff2, nr2, stream=stream)
            held.append(apart)
            same(CLIPS, cl.host(), apart.host())
    finally:
        close_all(held)
