"""kmx_scripts_realign and kmx_scripts_clip where tests/test_realign_gpu.py and tests/test_clip_gpu.py do not reach: gaps that are
opened, extended across lanes and walked back in every class of the band (NPL = 1, 2, 4, 8 diagonals per lane), the contract's tie
rules on texts of low complexity in every class, the scorings at the bounds of the header, and seeded batches through the whole chain
into MD and the pileup.  The inputs and what they are made for: tests/realign_band.py and tests/test_realign_bands_cpu.py.

The oracle is tests/realign_naive.py (tests/clip_naive.py for the trimmer) on the host views of the engine's own handles and on the
reads as the device holds them; every array, its dtype and every counter must be identical.  Behind it every realigned entry is
checked a second time without the oracle's tables or its walk: best_v() gives the score and the end cell, replay_score() the score
of the device's own runs.  A mismatch prints the entry (q, t, d, the scoring, both CIGARs, both (V, i1, j1)) for a replay on the CPU.
No batch holds more than 64 public reads."""
import numpy as np
import pytest

from tests import realign_band as rb
from tests import realign_naive as rn
from tests.chain_checks import check_clip_md, check_clips, check_pileup, check_realign, close_all, doubled, pileup_want, refused, same
from tests.chain_data import CLIPS, COMP4, LETTERS4 as LETTERS
from tests.helpers import pack

pytestmark = pytest.mark.gpu

K = rb.K
R, LOW = rn.REALIGNED, rn.LOW
DEL, INS = 5, 6                                                # the planes of a pileup over four letters


def opts(s, **more):
    return dict(rn.DEFAULTS, **s, **more)


def oracle(sc, al, ranks, roff, txt, sigma, **opt):
    dist, start, end = al.host()[:3]
    return rn.realign(*sc.host(), dist, start, end, ranks, roff, txt, sigma, **opt)


def report(cl, sc, al, ranks, roff, txt, sigma, want, opt):
    """every entry at which the handle and the oracle differ, in a form that replays on the CPU"""
    got = cl.host()
    g_str, w_str = cl.strings(), rn.strings(want[7], want[8])
    for e, (q, t, d) in enumerate(rb.entries_of(sc.host(), al.host(), ranks, roff, txt)):
        g = (g_str[e],) + tuple(int(a[e]) for a in got[:7])
        w = (w_str[e],) + tuple(int(a[e]) for a in want[:7])
        if g != w:
            ends = lambda x: (x[1], len(q) - x[3], len(t) - x[5])
            print(f"entry {e}: q = {q.tolist()}\nt = {t.tolist()}\nd = {d}, sigma = {sigma}, scoring = {opt}\n"
                  f"device {g[0]} (V, i1, j1) = {ends(g)} flags {g[7]}\noracle {w[0]} (V, i1, j1) = {ends(w)} flags {w[7]}\n"
                  f"best_v = {rb.best_v(q, t, d, sigma, **opt)}")


def second_opinion(cl, sc, al, ranks, roff, txt, sigma, opt):
    """Every entry of the handle against best_v() and replay_score(): a REALIGNED entry has the greatest V, its end cell and runs that
    are worth that V; an entry with a script is LOW exactly when the best path is empty (it ends in row 0) or below the floor."""
    score, sl, sr, tl, tr, nm, cflags, cig_off, cigar = cl.host()
    scripts = np.diff(sc.host()[2].astype(np.int64))
    for e, (q, t, d) in enumerate(rb.entries_of(sc.host(), al.host(), ranks, roff, txt)):
        if not scripts[e]:
            assert cflags[e] == LOW
            continue
        v, i1, j1 = rb.best_v(q, t, d, sigma, **opt)
        assert (cflags[e] == LOW) == (i1 == 0 or v < opt["min_score"]), (e, v, i1, j1)
        if cflags[e] == R:
            assert (int(score[e]), len(q) - int(sr[e]), len(t) - int(tr[e])) == (v, i1, j1), e
            worth = rb.replay_score(cigar[int(cig_off[e]):int(cig_off[e + 1])], q, t, int(tl[e]), sigma, **opt)
            assert worth == (v, len(q) - int(sl[e]) - int(sr[e]), len(t) - int(tl[e]) - int(tr[e])), e


def checked(cl, sc, al, ranks, roff, txt, sigma, want=None, **opt):
    """chain_checks.check_realign against the oracle (`want`: its tuple, where it is known already), with the report
    of a mismatch, and the second opinion"""
    want = oracle(sc, al, ranks, roff, txt, sigma, **opt) if want is None else want
    try:
        out = check_realign(cl, sc, want)
    except AssertionError:
        report(cl, sc, al, ranks, roff, txt, sigma, want, opt)
        raise
    second_opinion(cl, sc, al, ranks, roff, txt, sigma, opt)
    out["want"] = want
    return out


def aligned_at_voters(index, batch, max_edits, held):
    """(alignments, scripts, ranks, roff) of the aligned reads of a batch at the loci of its voters"""
    ranks, roff = pack(batch.aligned)
    loci = index.vote_windows(*pack(batch.voters), K, *rb.VOTE)
    held.append(loci)
    al = loci.align(index, ranks, roff, max_edits, 64)
    held.append(al)
    sc = al.scripts(index, loci, ranks, roff)
    held.append(sc)
    return al, sc, ranks, roff


def dist_of(al, sc):
    return al.host()[0][sc.host()[1]].astype(np.int64)


@pytest.fixture(scope="module")
def index(engine):
    idx = engine.Index(rb.plain_text(), 4, [K], table=2)
    yield idx
    idx.close()


# ---- 1. gaps in every class ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("s", (rb.DEFAULT, rb.ZERO, rb.SCORINGS[3], rb.ALL_255), ids=rb.name_of)
def test_gaps_in_every_class(engine, index, s):
    import torch
    b = rb.class_gaps()
    txt, opt = b.text, opts(s)
    held = []
    try:
        al, sc, ranks, roff = aligned_at_voters(index, b, 250, held)
        d = dist_of(al, sc)
        assert d.size == len(b.aligned) and sc.counts()["n_mismatched"] == 0
        assert [rb.class_of(x) for x in d.tolist()] == b.klass and [x for x, w in zip(d.tolist(), b.exact) if w is not None] == list(rb.BOUNDARIES)
        per_entry = sc.realign(index, al, ranks, roff, **s, scratch_bytes=1)    # clamped up to the largest entry: a chunk per entry
        held.append(per_entry)
        out = checked(per_entry, sc, al, ranks, roff, txt, 4, **opt)
        cl = sc.realign(index, al, ranks, roff, **s)
        held.append(cl)
        same(CLIPS, cl.host(), per_entry.host())
        assert cl.counts() == per_entry.counts()
        trimmed = sc.clip(**s)
        held.append(trimmed)
        check_clips(trimmed, sc, **s)
        assert (out["score"] >= trimmed.host()[0]).all()       # (min_score = 0: the trimmed part is one of the paths of the band)
        if s != rb.DEFAULT:
            return
        assert (out["cflags"] == R).all()
        for string, kind, g in zip(out["strings"], b.kind, b.g):
            assert all(f"={g}{op}" in string for op in kind), (string, kind, g)
        assert (out["score"] > trimmed.host()[0])[:12].all()   # a gap of 12 letters and more is in pieces in the unit-cost script
        # the pileup of these clips: the deletion of 72 letters is 72 positions of DEL, the insertion of 72 one INS
        d_ranks, d_roff = torch.from_numpy(ranks).cuda(), torch.from_numpy(roff.view(np.int64)).cuda()
        torch.cuda.synchronize()
        n = txt.size
        counts, ctr = pileup_want(sc, cl, al, ranks, roff, hi=n, n=n)
        pu = cl.pileup_device(index, sc, al, d_ranks.data_ptr(), d_roff.data_ptr(), roff.size - 1)
        held.append(pu)
        check_pileup(pu, counts, ctr, hi=n)
        assert ctr["n_added"] == len(b.aligned) and ctr["n_mismatched"] == 0
        planes = pu.planes()
        deleted, inserted = b.at[9], b.at[10]                  # the reads of the widest class with one gap
        assert (b.kind[9], b.kind[10], b.g[9]) == ("D", "I", 72)
        where = np.flatnonzero(planes[DEL, deleted:deleted + len(b.aligned[9]) + 72]) + deleted
        assert where.size == 72 and where[-1] - where[0] == 71 and (planes[DEL, where] == 1).all()
        assert int(planes[INS, inserted:inserted + len(b.aligned[10])].sum()) == 1
        md = cl.md(index, sc, al, LETTERS)
        held.append(md)
        _, start, end = al.host()[:3]
        strings = check_clip_md(md, out, start, end, txt)
        assert md.counts()["n_mismatched"] == 0 and strings[9].count("^") == 1 and len(strings[9]) > 72
    finally:
        close_all(held)


# ---- 2. ties ------------------------------------------------------------------------------------------------------------------------------------
TIE_SCORINGS = (rb.ZERO, rb.SCORINGS[2], rb.SCORINGS[5], rb.DEFAULT)
TIE_CASES = [(name, 0, rb.TIE_EDITS) for name in rb.TIE_NAMES] + [("tandem", target, max_edits) for max_edits, target in rb.RAISED]


@pytest.mark.parametrize("name,raised,max_edits", TIE_CASES, ids=[f"{n}_{r}" for n, r, _ in TIE_CASES])
def test_ties_on_low_complexity_texts(engine, name, raised, max_edits):
    import torch
    assert [rb.name_of(s) for s in TIE_SCORINGS] == ["a1_b0_o0_x0_p0", "a1_b1_o0_x1_p0", "a2_b1_o0_x1_p1", "a1_b4_o6_x1_p5"]
    b = rb.tandem_reads(raised) if raised else rb.tie_texts()[rb.TIE_NAMES.index(name)]
    txt, sigma = b.text, b.sigma
    idx = engine.Index(txt, sigma, [K], table=2)
    held = []
    try:
        al, sc, ranks, roff = aligned_at_voters(idx, b, max_edits, held)
        d = dist_of(al, sc)
        assert d.size == len(b.aligned) and sc.counts()["n_mismatched"] == 0
        if raised:                                             # the same ties at NPL = 2, 4 and 8
            assert d.tolist() == [raised] * 4 and rb.class_of(raised) == {36: 1, 67: 2, 129: 3}[raised]
        d_ranks, d_roff = torch.from_numpy(ranks).cuda(), torch.from_numpy(roff.view(np.int64)).cuda()
        torch.cuda.synchronize()
        cl = None
        for s in TIE_SCORINGS:
            opt = opts(s)
            cl = sc.realign(idx, al, ranks, roff, **s, clips=cl)
            if cl not in held:
                held.append(cl)
            out = checked(cl, sc, al, ranks, roff, txt, sigma, **opt)
            by_device = sc.realign_device(idx, al, d_ranks.data_ptr(), d_roff.data_ptr(), roff.size - 1, **s)
            held.append(by_device)
            checked(by_device, sc, al, ranks, roff, txt, sigma, want=out["want"], **opt)
    finally:
        close_all(held)
        idx.close()


# ---- 3. the bounds of the scoring -----------------------------------------------------------------------------------------------------------------
def bound_reads():
    """(voters, aligned): the read of 1024 letters of tests/test_clip_gpu.py at 250 edits, 1024 letters without an edit, the read of
    the widest class with a deletion of 72 letters, one letter, and 40 letters outside the alphabet (its script is 40I)"""
    t = rb.plain_text()
    long = t[6000:6000 + 1024].copy()
    long[0:250:2] = rb.other(long[0:250:2])
    long[1024 - 250::2] = rb.other(long[1024 - 250::2])
    long[300:701:100] = rb.other(long[300:701:100])
    gaps = rb.class_gaps()
    at = (6000, 13_000, gaps.at[9], 15_000, 16_000)
    aligned = [long, t[13_000:13_000 + 1024].copy(), gaps.aligned[9], t[15_000:15_001].copy(), np.full(40, 255, np.uint8)]
    return rb.Batch(t, [t[a:a + 150].copy() for a in at], aligned, at=at, sigma=4)


@pytest.fixture(scope="module")
def bounds(index):
    held = []
    out = aligned_at_voters(index, bound_reads(), 250, held)
    yield out
    close_all(held)


@pytest.mark.parametrize("s", rb.SCORINGS, ids=rb.name_of)
def test_scoring_bounds(engine, index, bounds, s):
    al, sc, ranks, roff = bounds
    txt, opt = rb.plain_text(), opts(s)
    assert dist_of(al, sc).tolist() == [250, 0, 142, 0, 40] and sc.strings()[1:] == ["1024=", sc.strings()[2], "1=", "40I"]
    held = []
    try:
        cl = sc.realign(index, al, ranks, roff, **s)
        held.append(cl)
        out = checked(cl, sc, al, ranks, roff, txt, 4, **opt)
        a, p = s["match"], s["clip_penalty"]
        assert (out["strings"][1], int(out["score"][1]), int(out["cflags"][1])) == ("1024=", 1024 * a, R)
        assert a != 255 or int(out["score"][1]) == 261_120     # above 65535: the score is not a 16-bit value anywhere
        assert (out["strings"][3], int(out["score"][3])) == ("1=", a)
        assert (out["strings"][4], int(out["cflags"][4]), int(out["score"][4])) == ("40I", LOW, -(s["gap_open"] + 40 * s["gap_extend"]))
        got = cl.host()
        if p == 65535:                                         # nothing is clipped unless the oracle clips it
            want = out["want"]
            assert np.array_equal((got[1].astype(np.int64) + got[2]) > 0, (want[1].astype(np.int64) + want[2]) > 0)
            assert not (got[1][1] or got[2][1] or got[1][3] or got[2][3])                     # the two reads without an edit
        trimmed = sc.clip(**s)
        held.append(trimmed)
        cut = check_clips(trimmed, sc, **s)
        assert (int(cut["score"][1]), cut["strings"][1], cut["strings"][4]) == (1024 * a, "1024=", "40I")
        assert (out["score"] >= cut["score"]).all()
    finally:
        close_all(held)


def test_min_score_at_either_end_of_int32_and_the_refusals(engine, index, bounds):
    al, sc, ranks, roff = bounds
    txt = rb.plain_text()
    held = []
    try:
        # 2^31 - 1: nothing meets it, and both calls leave the same whole entries
        cl = sc.realign(index, al, ranks, roff, min_score=rb.INT_MAX)
        trimmed = sc.clip(min_score=rb.INT_MAX)
        held += [cl, trimmed]
        for name, g, w in zip(CLIPS, cl.host(), trimmed.host()):
            assert g.dtype == w.dtype and g.tobytes() == w.tobytes(), name
        n_sel = sc.counts()["n_sel"]
        assert cl.counts() == trimmed.counts() == dict(n_sel=n_sel, n_ops=sc.counts()["n_ops"], n_clipped=0, n_low=n_sel)
        check_clips(trimmed, sc, min_score=rb.INT_MAX)
        assert cl.strings() == sc.strings() and (cl.host()[6] == LOW).all()
        # -2^31: every entry is realigned, under a scoring that makes the best path of an edited read worth less than nothing
        s = rb.SCORINGS[8]
        assert s == rb.scoring(1, 255, 255, 255, 65535)
        for floor in (rb.INT_MIN, rb.INT_MAX):
            sc.realign(index, al, ranks, roff, **s, min_score=floor, clips=cl)
            sc.clip(**s, min_score=floor, clips=trimmed)
            check_clips(trimmed, sc, **s, min_score=floor)
            out = checked(cl, sc, al, ranks, roff, txt, 4, **opts(s, min_score=floor))
            assert (out["cflags"] == LOW).tolist() == [floor == rb.INT_MAX] * 5
            # (40 insertions cost 255 + 40 * 255, less than the clip of a read that keeps nothing: even 40I is a path here)
            assert floor == rb.INT_MAX or (out["strings"][4], int(out["score"][4]), int(out["nm"][4])) == ("40I", -10_455, 40)
        # the default scoring over the floor of -2^31: what the default floor gives, which every path here meets
        sc.realign(index, al, ranks, roff, min_score=rb.INT_MIN, clips=cl)
        second_opinion(cl, sc, al, ranks, roff, txt, 4, opts(rb.DEFAULT, min_score=rb.INT_MIN))
        at_zero = sc.realign(index, al, ranks, roff)
        held.append(at_zero)
        same(CLIPS, cl.host(), at_zero.host())
        assert cl.counts() == at_zero.counts() and (cl.host()[6] == R).tolist() == [True] * 4 + [False]
        # the four refusals: nothing is looked at, and a handle that was empty stays empty
        for kw in (dict(match=0), dict(match=256), dict(gap_extend=256), dict(clip_penalty=65536)):
            for call, fn in ((lambda c: sc.realign(index, al, ranks, roff, **kw, clips=c), "kmx_scripts_realign"), (lambda c: sc.clip(**kw, clips=c), "kmx_scripts_clip")):
                fresh = engine.Clips()
                refused(engine, lambda: call(fresh), fn)
                assert not fresh._h, kw
    finally:
        close_all(held)


# ---- 4. seeded batches through the whole chain ------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def fuzz(engine):
    """the index of the text of the seeded batches, and the two handles that every seed reuses"""
    idx = engine.Index(rb.fuzz_text(), 4, [K], table=2)
    cl, pu = engine.Clips(), engine.Pileup()
    yield idx, cl, pu
    close_all([cl, pu])
    idx.close()


def n_reads_of(seed):
    return (4, 32, 7)[seed % 3] if seed < 3 else 32            # small, large, small through the two handles; then whole batches


@pytest.mark.parametrize("seed", range(12))
def test_seeded_batches(engine, fuzz, seed):
    idx, cl, pu = fuzz
    b = rb.fuzz_batch(seed)
    txt, n, s = b.text, b.text.size, b.scoring
    opt = opts(s, min_score=b.min_score)
    public = b.aligned[:n_reads_of(seed)]
    held = list(idx.map_reads_strands(*pack(public), K, COMP4, **rb.FUZZ_CHAIN, scripts=True))
    try:
        reads, loci, al, pl, sc = held
        ranks2, roff2 = doubled(reads)
        d_ranks2, d_roff2, nr2, stream = reads.device_ptrs()
        assert nr2 == 2 * len(public) <= 64 and sc.counts()["n_mismatched"] == 0
        assert sc.counts()["n_sel"] >= len(public) // 2        # (tests/chain_naive.py places 26 or 27 of the 32 reads of seeds 0 .. 2)
        assert sc.realign_device(idx, al, d_ranks2, d_roff2, nr2, **s, min_score=b.min_score, stream=stream, clips=cl) is cl
        out = checked(cl, sc, al, ranks2, roff2, txt, 4, **opt)
        _, start, end = al.host()[:3]
        md = cl.md(idx, sc, al, LETTERS)
        held.append(md)
        check_clip_md(md, out, start, end, txt)
        assert md.counts()["n_mismatched"] == 0
        counts, ctr = pileup_want(sc, cl, al, ranks2, roff2, hi=n, n=n)
        assert cl.pileup(idx, sc, al, reads, pileup=pu) is pu
        check_pileup(pu, counts, ctr, hi=n)
        assert ctr["n_mismatched"] == 0 and ctr["n_added"] == sc.counts()["n_sel"]
        # the trimmer under the same scoring and floor, through the same clips handle
        assert sc.clip(**s, min_score=b.min_score, stream=stream, clips=cl) is cl
        cut = check_clips(cl, sc, **s, min_score=b.min_score)
        if b.min_score >= 0:
            assert (out["score"] >= cut["score"]).all()
    finally:
        close_all(held)
