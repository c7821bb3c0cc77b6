"""Mate rescue on the GPU: kmx_pairs_rescue, kmx_rescues_scripts, Pairs.rescue and Index.map_pairs(rescue=True).  The oracle is always
tests/rescue_naive.rescue applied to the engine's own host views from before the call (the loci, the alignments, the placements and
the pairs); every array and every counter must be bit-identical.  The texts, the repeat text, the chain settings and the helpers are
those of tests/chain_data.py and tests/chain_checks.py."""
import ctypes as C
import functools

import numpy as np
import pytest

from kmer_index_amd import synth
from tests import align_naive as an
from tests import fold_naive as fn
from tests import pair_naive as pn
from tests import rescue_naive as rn
from tests import script_naive as sn
from tests import vote_naive as vn
from tests import windows_naive as wn
from tests.chain_checks import MappedPairs, counters_of, dev_array, same
from tests.chain_data import (ALIGN, CHAIN, COMPLEMENT, INSERT, JOBS, LOCI, N_PAIRS, PAIRS, PAIR_WORKLOADS as WORKLOADS, PLACEMENTS, REPEAT_CHAIN,
                              RESCUE_FLOORS as FLOORS, SCRIPTS, copies_text, kill, rc, repeat_text, rescue_pairs_of, text_of)
from tests.helpers import pack

pytestmark = pytest.mark.gpu

NO, NONE16 = pn.NO_BEST, pn.NO_SCORE
ONLY = (pn.MATE1_ONLY, pn.MATE2_ONLY)
E = CHAIN["max_edits"]


def naive_floor(name):
    """How FLOORS was made: the whole chain on the CPU.  Not run by the tests (half a minute per workload)."""
    sigma, k, n = WORKLOADS[name]
    text = text_of(sigma, n)
    ranks2, roff2 = fn.double_reads(*rescue_pairs_of(name), COMPLEMENT[sigma], sigma)
    raw, where = text.tobytes(), {}
    for i in range(n - k + 1):
        where.setdefault(raw[i:i + k], []).append(i)
    qranks, qoff, win_off = wn.expand(ranks2, roff2, k, 1)
    qraw = qranks.tobytes()
    hits = [where.get(qraw[int(a):int(b)], []) for a, b in zip(qoff[:-1], qoff[1:])]
    hit_off = np.zeros(len(hits) + 1, np.uint64)
    hit_off[1:] = np.cumsum([len(h) for h in hits])
    positions = np.asarray([x for h in hits for x in h], np.uint32)
    locus_off, diag, span = vn.vote(hit_off, positions, win_off, 1, CHAIN["band"], CHAIN["min_votes"], 0)[:3]
    dist, start, end, best, _ = an.align(text, ranks2, roff2, locus_off, diag, span, E, CHAIN["max_span"], sigma)
    folded = pn.fold_pairs(locus_off, dist, start, end, best, **INSERT)
    got = rn.rescue(text, sigma, ranks2, roff2, locus_off, dist, start, end, folded[:7], folded[7:11], INSERT["min_insert"], INSERT["max_insert"], E)
    return int((np.isin(folded[7], ONLY) & (got[1][0] == pn.CONCORDANT)).sum())


class Mapped(MappedPairs):
    """map_pairs of a batch, its host loci and alignments, the doubled reads and the text"""

    def __init__(self, idx, text, sigma, ranks, roff, k, **kw):
        super().__init__(idx, sigma, ranks, roff, k, **kw)
        self.text = text
        self.ranks2, self.roff2 = fn.double_reads(ranks, roff, COMPLEMENT[sigma], sigma)

    def oracle(self, min_insert, max_insert, max_edits, orientation=pn.FR, discordant=False, unpaired_penalty=None):
        """rescue_naive on the host views as they are now"""
        penalty = pn.NO_PENALTY if unpaired_penalty is None else unpaired_penalty
        return rn.rescue(self.text, self.sigma, self.ranks2, self.roff2, self.h_loci[0], *self.h_al[:3], self.pl.host(), self.pairs.host(), min_insert,
                         max_insert, max_edits, orientation, discordant, penalty)

    def refold(self, min_insert, max_insert, orientation=pn.FR, unpaired_penalty=None):
        self.al.fold_pairs(self.loci, min_insert, max_insert, orientation, unpaired_penalty, placements=self.pl, pairs=self.pairs)


def check_against(mp, res, want):
    same(PLACEMENTS, mp.pl.host(), want[0])
    same(PAIRS, mp.pairs.host(), want[1])
    same(JOBS, res.host(), want[3])
    assert counters_of(mp.pl, mp.pairs) == want[2]
    assert res.counts() == want[4]


def rescue_checked(mp, min_insert, max_insert, max_edits, orientation=pn.FR, discordant=False, unpaired_penalty=None, segment=0, rescues=None, want=None):
    """The rescue on mp's handles against the oracle on their state before the call; returns (Rescues, the oracle's result by name)."""
    want = want or mp.oracle(min_insert, max_insert, max_edits, orientation, discordant, unpaired_penalty)
    res = mp.pairs.rescue(mp.idx, mp.reads, mp.loci, mp.al, mp.pl, min_insert, max_insert, max_edits, orientation, discordant, unpaired_penalty, segment,
                          rescues)
    check_against(mp, res, want)
    out = dict(zip(PLACEMENTS + PAIRS, want[0] + want[1]))
    out.update(want[2])
    out.update({"job_" + k: v for k, v in zip(JOBS, want[3])})
    out.update({("n_job_concordant" if k == "n_concordant" else k): v for k, v in want[4].items()})
    return res, out


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
            sigma, k, n = WORKLOADS[name]
            self.mapped[name] = Mapped(self.index(name), text_of(sigma, n), sigma, *rescue_pairs_of(name), k, **CHAIN, **INSERT)
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
def test_lost_mates_of_the_workload_are_rescued(work, name):
    mp = work.workload(name)
    mp.refold(**INSERT)
    before = [a.copy() for a in mp.pl.host() + mp.pairs.host()]
    res, want = rescue_checked(mp, **INSERT, max_edits=E)
    try:
        kind, cls0, cls1 = np.arange(N_PAIRS) % 4, before[7], want["cls"]
        assert [int((kind == x).sum()) for x in range(4)] == [75, 75, 75, 75] and want["np"] == N_PAIRS
        rescued = np.isin(cls0, ONLY) & (cls1 == pn.CONCORDANT)
        assert int(rescued.sum()) == FLOORS[name] and not rescued[kind != 0].any()
        assert want["n_taken"] == FLOORS[name] and want["n_jobs"] >= 225
        # which mate and which strand alternate
        i = np.flatnonzero(rescued)
        for lost in (0, 1):
            for s in (0, 1):
                assert int(((cls0[i] == (pn.MATE2_ONLY, pn.MATE1_ONLY)[lost]) & (want["strand"][2 * i + lost] == s)).sum()) >= 10
        assert (np.abs(want["tlen"][rescued]) >= 200).all() and (np.abs(want["tlen"][rescued]) <= 500).all()
        assert (want["score"][rescued] <= E).all() and (want["second_score"][rescued] == NONE16).all()
        # a random mate and a mate 5000 letters away stay where they were; so does every ordinary pair, byte for byte
        stay = kind != 0
        assert np.isin(cls0[(kind == 1) | (kind == 2)], ONLY).sum() >= 140 and np.array_equal(cls1[stay], cls0[stay])
        for name_, b, a in zip(PLACEMENTS + PAIRS, before, [want[k] for k in PLACEMENTS + PAIRS]):
            per = a.size // N_PAIRS
            assert np.array_equal(np.repeat(~rescued, per) * a, np.repeat(~rescued, per) * b), name_
    finally:
        res.close()


# ---- 2. discordant pairs ---------------------------------------------------------------------------------------------------------------
def test_discordant_pairs_are_rescued_only_when_asked(engine):
    t = copies_text()
    idx = engine.Index(t, 4, [10], table=2)
    reads = [t[10_000:10_100].copy(), rc(t[30_000:30_080]), t[15_000:15_080].copy(), rc(t[35_320:35_400])]
    mp = Mapped(idx, t, 4, *pack(reads), 10, **CHAIN, **INSERT)
    res = engine.Rescues()
    try:
        start = mp.pl.host()[3]
        assert mp.pairs.host()[0].tolist() == [pn.DISCORDANT] * 2 and start.tolist() == [10_000, 30_000, 15_000, 35_320]
        # the flag is off: no job, nothing moves
        _, want = rescue_checked(mp, **INSERT, max_edits=E, rescues=res)
        assert want["n_jobs"] == 0 and want["cls"].tolist() == [pn.DISCORDANT] * 2 and want["start"].tolist() == start.tolist()
        # the flag is on: pair 0 by its mate 2, pair 1 by the least (score, b): its mate 1
        _, want = rescue_checked(mp, **INSERT, max_edits=E, discordant=True, rescues=res)
        assert want["job_read"].tolist() == [0, 3, 4, 7] and want["job_status"].tolist() == [0, 3, 3, 2]
        assert want["cls"].tolist() == [pn.CONCORDANT] * 2 and want["start"].tolist() == [10_000, 10_320, 35_000, 35_320]
        assert want["second"][1] == 0 and want["second"][2] == 0          # the old placements, exact and elsewhere
        assert want["dist"][1] == 8 and want["score"].tolist() == [8, 8] and want["tlen"].tolist() == [400, 400]
        assert want["locus"][1] == NO and want["best2"][2:6].tolist() == [NO] * 4 and want["n_discordant"] == 0
        # penalty 0: both stay; penalty 8: both go
        mp.refold(**INSERT)
        _, want = rescue_checked(mp, **INSERT, max_edits=E, discordant=True, unpaired_penalty=0, rescues=res)
        assert want["job_status"].tolist() == [0, 2, 2, 2] and want["cls"].tolist() == [pn.DISCORDANT] * 2 and want["n_taken"] == 0
        _, want = rescue_checked(mp, **INSERT, max_edits=E, discordant=True, unpaired_penalty=7, rescues=res)
        assert want["n_taken"] == 0
        _, want = rescue_checked(mp, **INSERT, max_edits=E, discordant=True, unpaired_penalty=8, rescues=res)
        assert want["job_status"].tolist() == [0, 3, 3, 2]
    finally:
        res.close()
        mp.close()
        idx.close()


# ---- 3. the edges of the window --------------------------------------------------------------------------------------------------------
def test_window_edges(work):
    name = "dna4_k10"
    sigma, k, n = WORKLOADS[name]
    t = text_of(sigma, n)
    junk = synth.ranks(4712, 3, sigma)
    lost = lambda a, b: kill(rc(t[a:b]), k)                    # a broken mate 2 whose source is text[a:b)
    reads = [t[0:100].copy(), lost(320, 400),                                          # 0: the anchor at the very start of the text
             kill(t[n - 400:n - 320], k), rc(t[n - 100:n]),                            # 1: the anchor at its very end, mate 1 lost
             t[n - 400:n - 300].copy(), kill(rc(np.concatenate([t[n - 77:], junk])), k),  # 2: the lost mate overhangs the end of the text
             t[5000:5080].copy(), lost(5020, 5100),                                    # 3: T = min_insert
             t[6000:6100].copy(), lost(6520, 6600),                                    # 4: T = max_insert
             t[7000:7100].copy(), lost(7521, 7601),                                    # 5: T = max_insert + 1: the window ends a letter short
             t[8000:8100].copy(), lost(8020, 8100),                                    # 6: contained, ending flush
             t[9000:9150].copy(), lost(9020, 9100),                                    # 7: inside the anchor's interval
             t[10_000:10_100].copy(), lost(10_041, 10_121)]                            # 8: T = min_insert + 21
    mp = Mapped(work.index(name), t, sigma, *pack(reads), k, **CHAIN, **INSERT)
    res = work.engine.Rescues()
    try:
        M1, M2, CC = pn.MATE1_ONLY, pn.MATE2_ONLY, pn.CONCORDANT
        assert mp.pairs.host()[0].tolist() == [M1, M2, M1, M1, M1, M1, M1, M1, M1]
        _, want = rescue_checked(mp, **INSERT, max_edits=12, rescues=res)
        assert want["job_lo"].tolist()[:3] == [0, n - 600, n - 400] and want["job_hi"].tolist()[:3] == [600, n, n]
        assert want["job_status"].tolist() == [3, 3, 3, 3, 3, 3, 3, 1, 3]
        assert want["cls"].tolist() == [CC, CC, CC, CC, CC, CC, CC, M1, CC]
        assert want["tlen"].tolist() == [400, 400, 400, 100, 600, 600, 100, 0, 121]
        assert want["end"][5] == n and want["dist"][5] == 11                                       # the overhang deleted
        assert want["end"][11] == 7600 and want["dist"][11] == 9                                   # the last letter inserted
        assert (want["job_start"][7], want["job_end"][7], want["job_dist"][7]) == (9020, 9100, 8)
        # within 8 edits the overhanging and the cut mate are none
        mp.refold(**INSERT)
        _, want = rescue_checked(mp, **INSERT, max_edits=8, rescues=res)
        assert want["job_status"].tolist() == [3, 3, 0, 3, 3, 0, 3, 1, 3] and want["job_dist"][2] == rn.NONE
        # a tighter lower bound leaves pairs 3 and 6 found but not concordant
        mp.refold(101, 600)
        _, want = rescue_checked(mp, 101, 600, max_edits=8, rescues=res)
        assert want["job_status"].tolist() == [3, 3, 0, 1, 3, 0, 1, 1, 3]
    finally:
        res.close()
        mp.close()


# ---- 4. the segments -------------------------------------------------------------------------------------------------------------------
def test_the_result_does_not_depend_on_the_segment(work):
    mp = work.workload("dna4_k10")
    mp.refold(**INSERT)
    want = mp.oracle(**INSERT, max_edits=E)
    assert int((want[3][3].astype(np.int64) - want[3][2] == 600).sum()) >= 100        # windows of several segments
    res = work.engine.Rescues()
    try:
        for segment in (0, 7, 64, 1 << 31):
            mp.refold(**INSERT)
            rescue_checked(mp, **INSERT, max_edits=E, segment=segment, rescues=res, want=want)
    finally:
        res.close()


# ---- 5. every class of the passes ------------------------------------------------------------------------------------------------------
def test_mates_of_every_class_and_the_two_that_are_not_served(work):
    name = "dna4_k10"
    sigma, k, n = WORKLOADS[name]
    t = text_of(sigma, n)
    lengths = (64, 65, 128, 129, 257, 513, 1024, 1025, 12, 0)            # 12 <= E: not served; 1025 and the empty mate neither
    reads = []
    for i, m in enumerate(lengths):
        s = 2000 + 4000 * i
        lost = rc(t[s + 200:s + 200 + m])
        if m >= 64:                                            # 12 substitutions, evenly spread: beyond the 8 edits of the chain
            at = ((np.arange(12) + 0.5) * m / 12).astype(np.int64)
            lost[at] = (lost[at] + 1) % sigma
        elif m:
            lost = synth.ranks(4713, m, sigma)
        reads += [t[s:s + 100].copy(), lost]
    insert = dict(min_insert=100, max_insert=1400)
    mp = Mapped(work.index(name), t, sigma, *pack(reads), k, **CHAIN, **insert)
    res = None
    try:
        assert mp.pairs.host()[0].tolist() == [pn.MATE1_ONLY] * len(lengths)
        res, want = rescue_checked(mp, **insert, max_edits=12)
        assert want["job_dist"].tolist() == [12] * 7 + [rn.SKIPPED] * 3 and want["job_status"].tolist() == [3] * 7 + [0] * 3
        assert want["tlen"].tolist() == [200 + m for m in lengths[:7]] + [0] * 3
        assert want["job_hi"].tolist() == [3400 + 4000 * i for i in range(len(lengths))]
    finally:
        if res is not None:
            res.close()
        mp.close()


# ---- 6. the repeat ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def repeat_text_with_a_broken_copy():
    """the repeat text of tests/chain_data.py, 300 random letters, 80 letters of the repeat broken at every 10th, 300 random letters"""
    t0, unit = repeat_text()
    two = np.concatenate([unit, unit])
    t = np.concatenate([t0, synth.ranks(505, 300, 4), kill(two[:80], 10), synth.ranks(506, 300, 4)])
    t.setflags(write=False)
    return t, two, t0.size


def test_a_rescued_read_with_many_loci_and_equal_copies_in_one_window(engine):
    t, two, n0 = repeat_text_with_a_broken_copy()
    idx = engine.Index(t, 4, [10], table=2)
    # pair 0: mate 2 is 80 letters of the repeat, exact at 139 places far from its anchor and broken 200 letters behind it
    # pair 1: mate 2 is the same 80 letters broken: no locus, and every copy in the window of its anchor [1800, 1900) is as good
    reads = [t[n0 + 100:n0 + 200].copy(), rc(two[:80]), t[1800:1900].copy(), kill(rc(two[:80]), 10)]
    mp = Mapped(idx, t, 4, *pack(reads), 10, **REPEAT_CHAIN, **INSERT)
    res = None
    try:
        n_loci = np.diff(mp.h_loci[0].astype(np.int64))
        assert n_loci[3] > 128 and mp.pairs.host()[0].tolist() == [pn.DISCORDANT, pn.MATE1_ONLY]
        res, want = rescue_checked(mp, **INSERT, max_edits=E, discordant=True)
        assert want["job_status"].tolist() == [0, 3, 3] and want["cls"].tolist() == [pn.CONCORDANT] * 2
        assert (want["start"][1], want["end"][1], want["dist"][1], want["second"][1]) == (n0 + 300, n0 + 380, 8, 0)
        assert (want["end"][3], want["dist"][3], want["second"][3]) == (2080, 8, 255)                # the smallest end wins
        assert want["n_ambiguous"] == 0
    finally:
        if res is not None:
            res.close()
        mp.close()
        idx.close()


# ---- 7. shapes -------------------------------------------------------------------------------------------------------------------------
def test_batches_of_every_size_through_one_set_of_handles(work):
    name = "dna4_k10"
    sigma, k, n = WORKLOADS[name]
    idx, t = work.index(name), text_of(sigma, n)
    ranks, roff = rescue_pairs_of(name)
    res = work.engine.Rescues()
    try:
        for n_pairs in (257, 0, 1, 3, 257):
            sub_off = roff[:2 * n_pairs + 1]
            mp = Mapped(idx, t, sigma, ranks[:int(sub_off[-1])], sub_off, k, **CHAIN, **INSERT)
            try:
                _, want = rescue_checked(mp, **INSERT, max_edits=E, rescues=res)
                assert want["np"] == n_pairs and want["nr2"] == 4 * n_pairs
                if n_pairs == 0:
                    assert want["n_jobs"] == 0 and res.device_ptrs()[1:] == (None,) * 7 and res.host()[0].tolist() == [0]
                if n_pairs == 257:
                    assert want["n_taken"] >= 60
                # a second rescue of the same handles takes nothing: both stay byte for byte
                _, again = rescue_checked(mp, **INSERT, max_edits=E, rescues=res)
                assert again["n_taken"] == 0 and again["n_jobs"] == want["n_jobs"] - want["n_taken"]
                for x in PLACEMENTS + PAIRS:
                    assert np.array_equal(again[x], want[x]), x
            finally:
                mp.close()
        # a batch without an eligible pair: zero jobs
        sub = [np.asarray(ranks[int(roff[i]):int(roff[i + 1])]) for p in range(3, 40, 4) for i in (2 * p, 2 * p + 1)]
        mp = Mapped(idx, t, sigma, *pack(sub), k, **CHAIN, **INSERT)
        try:
            assert mp.pairs.host()[0].tolist() == [pn.CONCORDANT] * 10
            before = mp.pl.host() + mp.pairs.host()
            _, want = rescue_checked(mp, **INSERT, max_edits=E, rescues=res)
            assert want["n_jobs"] == 0 and not want["job_job_off"].any() and want["job_job_off"].size == 41
            same(PLACEMENTS + PAIRS, mp.pl.host() + mp.pairs.host(), before)
        finally:
            mp.close()
    finally:
        res.close()


# ---- 8. the scripts of the rescued mates -----------------------------------------------------------------------------------------------
def test_scripts_of_the_rescued_mates(work):
    name = "dna4_k10"
    sigma, _, _ = WORKLOADS[name]
    mp, engine = work.workload(name), work.engine
    mp.refold(**INSERT)
    res, _ = rescue_checked(mp, **INSERT, max_edits=E)
    held = [res]
    try:
        job_off, read, _, _, dist, start, end, status = res.host()
        best = np.full(mp.roff2.size - 1, NO, np.uint32)
        best[read[status == 3]] = 0
        assert set((read[status == 3] & 1).tolist()) == {0, 1}                     # forward and reverse placements
        for m in (False, True):
            scr = res.scripts(mp.idx, mp.reads, m=m)
            held.append(scr)
            want = sn.scripts(mp.text, mp.ranks2, mp.roff2, job_off, dist, start, end, best, sigma, False, m)
            got = scr.host()
            same(SCRIPTS, got, want[:4])
            c = scr.counts()
            assert (c["nr"], c["n_sel"], c["n_mismatched"]) == (best.size, int((status == 3).sum()), 0) and want[4] == 0
            assert np.array_equal(got[1], np.flatnonzero(status == 3))             # sel = the job
            for e, j in enumerate(got[1]):                                         # every script replays against the text
                q = mp.ranks2[int(mp.roff2[read[j]]):int(mp.roff2[read[j] + 1])]
                runs = got[3][int(got[2][e]):int(got[2][e + 1])]
                assert sn.replay(q, mp.text[int(start[j]):int(end[j])], runs, sigma) == (int(dist[j]), True), j
        cigars = res.cigars(held[1])
        strand = mp.pl.host(best2=False)[1]
        assert len(cigars) == 2 * N_PAIRS and sum(bool(s) for s in cigars) == int((status == 3).sum())
        assert all(bool(cigars[int(r) // 2]) and strand[int(r) // 2] == int(r) % 2 for r in read[status == 3])
        # KMX_SCRIPT_ALL is refused
        o = engine.ScriptOptions(C.sizeof(engine.ScriptOptions), engine.SCRIPT_ALL, 0)
        assert engine.lib().kmx_rescues_scripts(mp.idx._h, mp.reads._h, res._h, C.byref(o), C.byref(held[1]._h)) == 1
        assert b"KMX_SCRIPT_ALL" in engine.lib().kmx_last_error()
    finally:
        for h in reversed(held):
            h.close()


# ---- 9. plumbing -----------------------------------------------------------------------------------------------------------------------
def test_refusals_and_the_state_of_the_three_handles(work):
    name = "dna4_k10"
    sigma, k, n = WORKLOADS[name]
    engine, idx, t = work.engine, work.index(name), text_of(sigma, n)
    L = engine.lib()
    ranks, roff = rescue_pairs_of(name)
    mp = Mapped(idx, t, sigma, ranks[:int(roff[16])], roff[:17], k, **CHAIN, **INSERT)
    other = Mapped(idx, t, sigma, ranks[:int(roff[24])], roff[:25], k, **CHAIN, **INSERT)
    held = []
    try:
        res, want = rescue_checked(mp, **INSERT, max_edits=E)
        held.append(res)
        assert want["n_taken"] == 2
        state = lambda: ([a.tobytes() for a in mp.pl.host() + mp.pairs.host() + res.host()], counters_of(mp.pl, mp.pairs), res.counts())
        full = state()
        size = C.sizeof(engine.RescueOptions)
        assert size == 32
        opt = lambda **kw: engine.RescueOptions(**dict(dict(struct_size=size, min_insert=100, max_insert=600, orientation=0, max_edits=E,
                                                           unpaired_penalty=0, segment=0, flags=0), **kw))
        call = lambda o, index=idx, reads=mp.reads, loci=mp.loci, al=mp.al, pl=mp.pl, pr=mp.pairs, out=res: L.kmx_pairs_rescue(
            index and index._h, reads and reads._h, loci and loci._h, al and al._h, o and C.byref(o), pl and pl._h, pr and pr._h, out and C.byref(out._h))
        # before any handle is looked at: all three stay as they are
        for o, word in ((opt(struct_size=size - 1), "struct_size"), (opt(flags=2), "flags"), (opt(orientation=3), "orientation"),
                        (opt(min_insert=601), "min_insert"), (opt(max_insert=65537), "KMX_RESCUE_MAX_INSERT"), (opt(max_edits=251), "max_edits")):
            assert call(o) == 1 and word.encode() in L.kmx_last_error(), word
        good = opt()
        for kw in (dict(index=None), dict(reads=None), dict(loci=None), dict(al=None), dict(pl=None), dict(pr=None), dict(out=None)):
            assert call(good, **kw) == 1
        assert call(None) == 1
        assert L.kmx_rescues_counts(None, *[None] * 5) == 1 and L.kmx_rescues_view(None, *[None] * 8) == 1
        assert L.kmx_rescues_view_device(None, *[None] * 8) == 1
        assert L.kmx_rescues_scripts(idx._h, mp.reads._h, None, None, None) == 1 and L.kmx_rescues_scripts(idx._h, None, res._h, None, None) == 1
        L.kmx_rescues_free(None)
        assert state() == full
        # after looking: the placements and the pairs stay, the rescues hold an empty result
        pl_pr = (full[0][:11], full[1])
        for kw, word in ((dict(loci=other.loci), "differs"), (dict(al=other.al), "differs"), (dict(reads=other.reads), "nr2 differs"),
                         (dict(pl=other.pl), "nr differs"), (dict(pr=other.pairs), "np differs")):
            mp.pairs.rescue(idx, mp.reads, mp.loci, mp.al, mp.pl, **INSERT, max_edits=E, rescues=res)
            assert res.counts()["nr2"] == 32
            assert call(good, **kw) == 1 and word.encode() in L.kmx_last_error(), word
            assert res.counts() == dict(nr2=0, n_jobs=0, n_found=0, n_concordant=0, n_taken=0)
            assert res.device_ptrs() == (None,) * 8 and res.host()[0].tolist() == [0] and all(x.size == 0 for x in res.host()[1:])
            now = state()
            assert (now[0][:11], now[1]) == pl_pr
        # the greatest max_edits (every mate is too short for it), then the greatest max_insert (windows of 128 segments, clipped by
        # the text) and a handle allocated by the call
        mp.refold(**INSERT)
        _, want = rescue_checked(mp, **INSERT, max_edits=250, rescues=res)
        assert want["job_dist"].tolist() == [rn.SKIPPED] * want["n_jobs"] and want["n_jobs"] >= 6
        res2, want = rescue_checked(mp, 0, 65536, max_edits=60)
        held.append(res2)
        assert int((want["job_hi"].astype(np.int64) - want["job_lo"] > 20_000).sum()) >= 3 and want["n_found"] >= 3
    finally:
        for h in reversed(held):
            h.close()
        other.close()
        mp.close()


def test_views_agree_inputs_stay_and_map_pairs_is_the_calls_it_is_made_of(work):
    name = "dna4_k10"
    sigma, k, _ = WORKLOADS[name]
    mp, idx, engine = work.workload(name), work.index(name), work.engine
    ptrs = (mp.loci.device_ptrs(), mp.al.device_ptrs(), mp.reads.device_ptrs())
    d_ranks2, nr2 = mp.reads.device_ptrs()[0], mp.reads.device_ptrs()[2]
    mp.refold(**INSERT)
    res, want = rescue_checked(mp, **INSERT, max_edits=E)
    held = [res]
    try:
        # device views against host views
        nj = want["n_jobs"]
        dts = (np.uint64, np.uint32, np.uint32, np.uint32, np.uint8, np.uint32, np.uint32, np.uint8)
        same(JOBS, [dev_array(p, nr2 + 1 if x == "job_off" else nj, d) for p, d, x in zip(res.device_ptrs(), dts, JOBS)], res.host())
        dts = (np.uint32, np.uint8, np.uint8, np.uint32, np.uint32, np.uint8, np.uint32)
        same(PLACEMENTS, [dev_array(p, (4 if x == "best2" else 2) * N_PAIRS, d) for p, d, x in zip(mp.pl.device_ptrs(), dts, PLACEMENTS)], mp.pl.host())
        same(PAIRS, [dev_array(p, N_PAIRS, d) for p, d in zip(mp.pairs.device_ptrs(), (np.uint8, np.int32, np.uint16, np.uint16))], mp.pairs.host())
        # the loci, the alignments and the reads are untouched
        assert ptrs == (mp.loci.device_ptrs(), mp.al.device_ptrs(), mp.reads.device_ptrs())
        same(LOCI, mp.loci.host(), mp.h_loci)
        same(ALIGN, mp.al.host(), mp.h_al)
        assert np.array_equal(dev_array(d_ranks2, mp.ranks2.size, np.uint8), mp.ranks2)
        # map_pairs(rescue=True) is the calls it is made of, and map_pairs() is what it was
        ranks, roff = rescue_pairs_of(name)
        comp = np.asarray(COMPLEMENT[sigma], np.uint8)
        out = idx.map_pairs(ranks, roff, k, comp, **INSERT, **CHAIN, rescue=True, scripts=True)
        held += list(out)
        assert len(out) == 7 and isinstance(out[6], engine.Rescues) and isinstance(out[5], engine.Scripts)
        same(PLACEMENTS, out[3].host(), mp.pl.host())
        same(PAIRS, out[4].host(), mp.pairs.host())
        same(JOBS, out[6].host(), res.host())
        assert (out[3].counts(), out[4].counts(), out[6].counts()) == (mp.pl.counts(), mp.pairs.counts(), res.counts())
        assert out[5].counts()["n_sel"] == mp.pl.counts()["n_placed"] - want["n_taken"]      # a rescued placement is no locus
        plain = idx.map_pairs(ranks, roff, k, comp, **INSERT, **CHAIN)
        held += list(plain)
        assert len(plain) == 5
        mp.refold(**INSERT)
        same(PLACEMENTS, plain[3].host(), mp.pl.host())
        same(PAIRS, plain[4].host(), mp.pairs.host())
        with_edits = idx.map_pairs(ranks, roff, k, comp, **INSERT, **CHAIN, rescue=True, rescue_edits=3, rescue_discordant=True)
        held += list(with_edits)
        _, w3 = rescue_checked(mp, **INSERT, max_edits=3, discordant=True)
        same(PAIRS, with_edits[4].host(), mp.pairs.host())
        assert len(with_edits) == 6 and with_edits[5].counts()["n_taken"] == w3["n_taken"] < want["n_taken"]
        # the SAM fields of a rescued pair: a proper pair with both mates mapped
        strand, start = out[3].host(best2=False)[1], out[3].host(best2=False)[3]
        cls, tlen = out[4].host()[:2]
        flag, pos, pnext, tl = engine.sam_pair_fields(strand, start, cls, tlen)
        p = int(out[6].host()[1][out[6].host()[7] == 3][0]) // 4
        for i in (2 * p, 2 * p + 1):
            assert flag[i] & 0x2 and not flag[i] & 0xC and pos[i] == int(start[i]) + 1 and pnext[i] == int(start[i ^ 1]) + 1
        assert tl[2 * p] == tlen[p] == -tl[2 * p + 1] and tlen[p] != 0
    finally:
        for h in reversed(held):
            h.close()
