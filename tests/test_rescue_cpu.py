"""tests/rescue_naive.py against itself: the two statements of the mate rescue agree on seeded inputs, the hand-made cases of the
contract (include/kmx.h, KMX_PAIR_RESCUE) come out as it says, and the segmented forward pass of the kernels equals the serial one
wherever the distance is within the bound.  No device is needed."""
import numpy as np
import pytest

from tests import fold_naive as fn
from tests import pair_naive as pn
from tests import rescue_naive as rn
from tests.chain_data import rc
from tests.helpers import pack

SIGMA = 4
COMP = (3, 2, 1, 0)
NO = rn.NO_BEST
FR, RF, FF = pn.FR, pn.RF, pn.FF


def best_of(locus_off, dist):
    best = np.full(len(locus_off) - 1, NO, np.uint32)
    for r in range(len(locus_off) - 1):
        a, b = int(locus_off[r]), int(locus_off[r + 1])
        keys = [(int(dist[l]), l - a) for l in range(a, b) if int(dist[l]) < fn.SKIPPED]
        if keys:
            best[r] = min(keys)[1]
    return best


class Chain:
    """The host arrays of a chain from the mates and, for every internal read, a list of (dist, start, end); the pair fold is
    pair_naive's."""

    def __init__(self, text, mates, per_strand, min_insert, max_insert, orientation=FR, penalty=pn.NO_PENALTY):
        assert len(per_strand) == 2 * len(mates) and len(mates) % 2 == 0
        self.text = np.asarray(text, np.uint8)
        ranks, roff = pack([np.asarray(m, np.uint8) for m in mates])
        self.ranks2, self.roff2 = fn.double_reads(ranks, roff, COMP, SIGMA)
        self.off = np.zeros(len(per_strand) + 1, np.uint64)
        self.off[1:] = np.cumsum([len(x) for x in per_strand])
        flat = [t for x in per_strand for t in x]
        self.dist = np.asarray([t[0] for t in flat], np.uint8)
        self.start = np.asarray([t[1] for t in flat], np.uint32)
        self.end = np.asarray([t[2] for t in flat], np.uint32)
        folded = pn.fold_pairs(self.off, self.dist, self.start, self.end, best_of(self.off, self.dist), min_insert, max_insert, orientation, penalty)
        self.placements, self.pairs, self.counters = folded[:7], folded[7:11], folded[11]
        self.insert, self.orientation = (min_insert, max_insert), orientation

    def args(self):
        return (self.text, SIGMA, self.ranks2, self.roff2, self.off, self.dist, self.start, self.end, self.placements, self.pairs)

    def rescue(self, E, discordant=False, penalty=pn.NO_PENALTY, insert=None, loop=True):
        lo, hi = insert or self.insert
        got = rn.rescue(*self.args(), lo, hi, E, self.orientation, discordant, penalty)
        if loop:
            same_result(got, rn.rescue_loop(*self.args(), lo, hi, E, self.orientation, discordant, penalty))
        out = dict(zip(pn.PLACEMENTS, got[0]))
        out.update(zip(pn.PAIRS, got[1]))
        out.update(got[2])
        out.update({"job_" + k: v for k, v in zip(rn.JOBS, got[3])})
        out.update({("n_job_concordant" if k == "n_concordant" else k): v for k, v in got[4].items()})
        return out


def same_result(got, want):
    for names, g, w in ((pn.PLACEMENTS, got[0], want[0]), (pn.PAIRS, got[1], want[1]), (rn.JOBS, got[3], want[3])):
        for name, x, y in zip(names, g, w):
            assert x.dtype == y.dtype, name
            assert np.array_equal(x, y), name
    assert got[2] == want[2] and got[4] == want[4]


def make_pair(text, s, f, m1, m2, orientation, rev):
    """The mates of a fragment text[s:s + f) read from the forward (rev = 0) or the reverse strand, and where each lies:
    ((mate 1, strand, start, end), (mate 2, ...))."""
    frag = np.asarray(text[s:s + f])
    g = rc(frag) if rev else frag
    head, tail = g[:m1], g[f - m2:]
    hp, tp = ((s, s + m1), (s + f - m2, s + f)) if not rev else ((s + f - m1, s + f), (s, s + m2))
    if orientation == FR:
        return (head.copy(), rev, *hp), (rc(tail), 1 - rev, *tp)
    if orientation == RF:
        return (rc(head), 1 - rev, *hp), (tail.copy(), rev, *tp)
    return (head.copy(), rev, *hp), (tail.copy(), rev, *tp)


def mutate(q, every, first=3):
    q = np.array(q, np.uint8)
    q[first::every] = (q[first::every] + 1) % SIGMA
    return q


def random_text(seed, n):
    return np.random.default_rng(seed).integers(0, SIGMA, n).astype(np.uint8)


# ---- 1. the two statements agree -------------------------------------------------------------------------------------------------------
def random_chain(seed, orientation):
    rng = np.random.default_rng(seed)
    text = random_text(seed + 1000, 260)
    mates, per = [], []
    for _ in range(int(rng.integers(1, 6))):
        f, m1, m2 = int(rng.integers(24, 70)), int(rng.integers(7, 12)), int(rng.integers(7, 12))
        s = int(rng.integers(0, text.size - f))
        placed = make_pair(text, s, f, m1, m2, orientation, int(rng.integers(0, 2)))
        kind = int(rng.integers(0, 6))         # 0: both placed; 1, 2: one mate lost; 3: one mate misplaced; 4: both lost; 5: lost and random
        lost = int(rng.integers(0, 2))
        for mate, (q, strand, a, b) in enumerate(placed):
            loci = [[], []]
            if mate == lost and kind in (1, 2, 3, 5):
                q = mutate(q, int(rng.integers(3, 9)), int(rng.integers(0, 3)))
                if kind == 5:
                    q = rng.integers(0, SIGMA, q.size).astype(np.uint8)
                if kind == 3:
                    w = int(rng.integers(0, text.size - 12))
                    loci[int(rng.integers(0, 2))].append((int(rng.integers(0, 3)), w, w + int(rng.integers(6, 12))))
            elif kind != 4:
                loci[strand].append((int(rng.integers(0, 2)), a, b))
            if rng.random() < 0.3:               # a locus that is not aligned, and one that may lie anywhere
                loci[int(rng.integers(0, 2))].append((int(rng.choice([fn.SKIPPED, fn.NONE])), 0, 0))
                if loci[0] or loci[1]:
                    w = int(rng.integers(0, text.size - 12))
                    loci[int(rng.integers(0, 2))].append((int(rng.integers(1, 4)), w, w + 9))
            mates.append(q)
            per += loci
    lo = int(rng.integers(0, 30))
    return Chain(text, mates, per, lo, lo + int(rng.integers(10, 70)), orientation, int(rng.choice([0, 2, pn.NO_PENALTY])))


@pytest.mark.parametrize("orientation", [FR, RF, FF])
@pytest.mark.parametrize("discordant", [False, True])
def test_the_two_statements_agree(orientation, discordant):
    taken = jobs = 0
    for seed in range(24):
        ch = random_chain(100 * orientation + seed, orientation)
        for penalty in (0, 1, 5, pn.NO_PENALTY):
            got = ch.rescue(int(np.random.default_rng(seed).integers(0, 4)), discordant, penalty)
            taken += got["n_taken"]
            jobs += got["n_jobs"]
    assert jobs >= 40 and taken >= 10


# ---- 2. the clauses by hand ------------------------------------------------------------------------------------------------------------
TEXT = random_text(7, 700)


def lost_pair(orientation, rev, lost, s=100, f=120, m=20, every=9, **kw):
    """one pair whose mate `lost` has no locus and a substitution at every `every`-th letter; the other lies where it was cut"""
    placed = make_pair(TEXT, s, f, m, m, orientation, rev)
    mates, per = [], []
    for mate, (q, strand, a, b) in enumerate(placed):
        loci = [[], []]
        if mate == lost:
            q = mutate(q, every)
        else:
            loci[strand].append((0, a, b))
        mates.append(q)
        per += loci
    return Chain(TEXT, mates, per, kw.pop("min_insert", 50), kw.pop("max_insert", 300), orientation), placed


@pytest.mark.parametrize("orientation", [FR, RF, FF])
@pytest.mark.parametrize("rev", [0, 1])
@pytest.mark.parametrize("lost", [0, 1])
def test_every_orientation_anchor_strand_and_mate(orientation, rev, lost):
    ch, placed = lost_pair(orientation, rev, lost)
    assert ch.pairs[0].tolist() == [pn.MATE2_ONLY if lost == 0 else pn.MATE1_ONLY]
    got = ch.rescue(2)
    _, strand, a, b = placed[lost]
    i = lost
    assert got["cls"].tolist() == [pn.CONCORDANT] and got["job_status"].tolist() == [3] and got["n_taken"] == 1
    assert (got["strand"][i], got["dist"][i], got["start"][i], got["end"][i]) == (strand, 2, a, b)
    assert got["locus"][i] == NO and got["best2"][2 * i:2 * i + 2].tolist() == [NO, NO] and got["second"][i] == 255
    assert got["job_read"].tolist() == [2 * lost + strand]
    upstream_is_mate1 = placed[0][2] < placed[1][2]
    assert got["tlen"].tolist() == [120 if upstream_is_mate1 else -120]
    assert got["score"].tolist() == [2] and got["second_score"].tolist() == [pn.NO_SCORE]
    assert got["n_placed"] == 2 and got["n_concordant"] == 1 and got["n_single"] == 0 and got["n_reverse"] == (2 if orientation == FF and rev else 0 if orientation == FF else 1)
    # the anchor stays byte for byte
    j = 1 - lost
    for name in pn.PLACEMENTS[:6]:
        assert got[name][j] == ch.placements[pn.PLACEMENTS.index(name)][j], name
    # an edit too many: none
    assert ch.rescue(1)["job_dist"].tolist() == [rn.NONE] and ch.rescue(1)["cls"].tolist() == ch.pairs[0].tolist()


def test_the_window_is_clipped_at_both_ends_of_the_text():
    ch, _ = lost_pair(FR, 0, 0, s=0, f=100)                   # the lost mate at [0, 20), the anchor downstream: lo = max(0, 100 - 300)
    got = ch.rescue(2)
    assert (got["job_lo"].tolist(), got["job_hi"].tolist()) == ([0], [100]) and got["start"][0] == 0 and got["job_status"].tolist() == [3]
    n = TEXT.size
    ch, _ = lost_pair(FR, 0, 1, s=n - 100, f=100)             # the lost mate at [n - 20, n), the anchor upstream: hi = min(n, n - 100 + 300)
    got = ch.rescue(2)
    assert (got["job_lo"].tolist(), got["job_hi"].tolist()) == ([n - 100], [n]) and got["end"][1] == n and got["job_status"].tolist() == [3]
    # a mate that overhangs the end of the text comes out with the overhang deleted
    placed = make_pair(TEXT, n - 100, 100, 20, 20, FR, 0)
    over = np.concatenate([TEXT[n - 18:], [0, 1]]).astype(np.uint8)
    ch = Chain(TEXT, [placed[0][0], rc(over)], [[(0, n - 100, n - 80)], [], [], []], 50, 300)
    got = ch.rescue(2)
    assert got["job_status"].tolist() == [3] and (got["dist"][1], got["start"][1], got["end"][1]) == (2, n - 18, n) and got["tlen"].tolist() == [100]


def test_the_template_length_at_its_bounds():
    for lo, hi, status in ((120, 300, 3), (50, 120, 3), (121, 300, 1)):
        ch, _ = lost_pair(FR, 0, 1, min_insert=lo, max_insert=hi)
        got = ch.rescue(2)
        assert got["job_status"].tolist() == [status] and (got["tlen"].tolist() == [120]) == (status == 3)
    # T = max_insert + 1: the window ends one letter short, and the alignment the window has is the mate with its last letter
    # inserted: one edit more, T = max_insert
    ch, _ = lost_pair(FR, 0, 1, min_insert=50, max_insert=119)
    assert ch.rescue(2)["job_dist"].tolist() == [rn.NONE]
    got = ch.rescue(3)
    assert got["job_status"].tolist() == [3] and got["dist"][1] == 3 and got["end"][1] == 219 and got["tlen"].tolist() == [119]


def test_found_but_not_concordant():
    # the mate inside the anchor's interval: the anchor [100, 160) forward, the mate the reverse complement of [110, 130)
    anchor = TEXT[100:160].copy()
    inside = mutate(rc(TEXT[110:130]), 9)
    ch = Chain(TEXT, [anchor, inside], [[(0, 100, 160)], [], [], []], 0, 300)
    got = ch.rescue(2)
    assert got["job_status"].tolist() == [1] and got["job_start"].tolist() == [110] and got["job_end"].tolist() == [130]
    assert got["cls"].tolist() == [pn.MATE1_ONLY] and got["n_found"] == 1 and got["n_job_concordant"] == 0 and got["n_taken"] == 0
    for g, w in zip(got_arrays(got), ch.placements + ch.pairs):
        assert np.array_equal(g, w)
    # a dovetail: the anchor [200, 260) on the reverse strand, the forward mate starts behind the anchor's start
    anchor = rc(TEXT[200:260])
    tail = mutate(TEXT[230:250], 9)
    ch = Chain(TEXT, [tail, anchor], [[], [], [], [(0, 200, 260)]], 0, 300)
    got = ch.rescue(2)
    assert got["job_status"].tolist() == [1] and got["job_start"].tolist() == [230] and got["cls"].tolist() == [pn.MATE2_ONLY]


def got_arrays(got):
    return [got[k] for k in pn.PLACEMENTS + pn.PAIRS]


def two_copies():
    """Region 1 holds mate 1's source and a copy of mate 2's with one substitution, region 2 the other way round; the loci name the
    exact sources, 400 letters apart: a discordant pair that both mates can be rescued from, at the same score."""
    text = TEXT.copy()
    text[400:420] = mutate(text[100:120], 50, 5)
    text[200:220] = mutate(text[500:520], 50, 5)
    mate1, mate2 = text[100:120].copy(), rc(text[500:520])
    return text, [mate1, mate2], [[(0, 100, 120)], [], [], [(0, 500, 520)]]


def test_a_discordant_pair_the_tie_and_the_penalty():
    text, mates, per = two_copies()
    ch = Chain(text, mates, per, 50, 300)
    assert ch.pairs[0].tolist() == [pn.DISCORDANT]
    off = ch.rescue(2)                                         # the flag is off: no job
    assert off["n_jobs"] == 0 and off["cls"].tolist() == [pn.DISCORDANT]
    got = ch.rescue(2, True)
    assert got["job_status"].tolist() == [3, 2] and got["job_dist"].tolist() == [1, 1] and got["job_read"].tolist() == [0, 3]
    assert got["cls"].tolist() == [pn.CONCORDANT] and got["score"].tolist() == [1] and got["tlen"].tolist() == [120]
    assert (got["start"].tolist(), got["end"].tolist()) == ([400, 500], [420, 520])
    assert got["second"][0] == 0                               # the old placement lies elsewhere
    assert got["n_discordant"] == 0 and got["n_concordant"] == 1 and got["n_job_concordant"] == 2
    # rejected by the penalty, accepted one higher
    rejected = ch.rescue(2, True, 0)
    assert rejected["job_status"].tolist() == [2, 2] and rejected["cls"].tolist() == [pn.DISCORDANT]
    for g, w in zip(got_arrays(rejected), ch.placements + ch.pairs):
        assert np.array_equal(g, w)
    assert ch.rescue(2, True, 1)["job_status"].tolist() == [3, 2]
    # only the second mate's job is concordant: it is taken
    per[0] = [(0, 100, 120)]
    text2 = text.copy()
    text2[400:420] = (text2[400:420] + 1) % SIGMA
    got = Chain(text2, mates, per, 50, 300).rescue(2, True)
    assert got["job_status"].tolist() == [0, 3] and got["start"].tolist() == [100, 200]


def test_second_ignores_an_old_placement_that_overlaps():
    # mate 2's old locus ends two letters late: T = 122 > max_insert; the window [100, 221) yields the placement at [200, 220)
    placed = make_pair(TEXT, 100, 120, 20, 20, FR, 0)
    per = [[(0, 100, 120)], [], [], [(2, 200, 222), (rn.NONE, 0, 0)]]
    ch = Chain(TEXT, [placed[0][0], placed[1][0]], per, 50, 121)
    assert ch.pairs[0].tolist() == [pn.DISCORDANT]
    got = ch.rescue(2, True)
    assert got["cls"].tolist() == [pn.CONCORDANT] and (got["start"][1], got["end"][1], got["dist"][1]) == (200, 220, 0)
    assert got["second"][1] == 255 and got["score"].tolist() == [0]
    # the same old locus on the other strand lies elsewhere
    per[2], per[3] = [(2, 200, 222)], []
    got = Chain(TEXT, [placed[0][0], placed[1][0]], per, 50, 121).rescue(2, True)
    assert got["cls"].tolist() == [pn.CONCORDANT] and got["second"][1] == 2


@pytest.mark.parametrize("m,E", [(0, 0), (0, 2), (2, 2), (1, 2), (1025, 8)])
def test_reads_that_are_not_served(m, E):
    lost = np.random.default_rng(m).integers(0, SIGMA, m).astype(np.uint8)
    ch = Chain(TEXT, [TEXT[100:120].copy(), lost], [[(0, 100, 120)], [], [], []], 0, 300)
    got = ch.rescue(E)
    assert got["job_dist"].tolist() == [rn.SKIPPED] and got["job_status"].tolist() == [0] and got["n_jobs"] == 1 and got["n_found"] == 0
    assert got["job_start"].tolist() == [0] and got["job_end"].tolist() == [0] and got["cls"].tolist() == [pn.MATE1_ONLY]


def test_a_read_of_one_letter_more_than_the_bound_is_served():
    ch = Chain(TEXT, [TEXT[100:120].copy(), rc(TEXT[200:203])], [[(0, 100, 120)], [], [], []], 0, 300)
    got = ch.rescue(2)
    assert got["job_status"].tolist() == [3] and got["job_dist"].tolist()[0] <= 2


def test_no_pair_and_no_eligible_pair():
    empty = Chain(TEXT, [], [], 0, 300).rescue(2)
    assert empty["n_jobs"] == 0 and empty["job_job_off"].tolist() == [0] and empty["nr2"] == 0
    ch, _ = lost_pair(FR, 0, 1)
    once = rn.rescue(*ch.args(), 50, 300, 2)
    again = rn.rescue(*ch.args()[:8], once[0], once[1], 50, 300, 2)     # a second rescue finds nothing
    assert again[4]["n_jobs"] == 0 and again[2] == once[2]
    for g, w in zip(again[0] + again[1], once[0] + once[1]):
        assert np.array_equal(g, w)


# ---- 3. the segments of the forward pass -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("G", [1, 7, 64, None])
def test_the_segmented_forward_pass_equals_the_serial_one(G):
    rng = np.random.default_rng(11)
    text = random_text(12, 500)
    within = 0
    for _ in range(60):
        m, E = int(rng.integers(5, 40)), int(rng.integers(0, 5))
        if m <= E:
            continue
        s = int(rng.integers(0, text.size - m))
        q = text[s:s + m].copy()
        for _ in range(int(rng.integers(0, 7))):                # substitutions, insertions and deletions
            k, at = int(rng.integers(0, 3)), int(rng.integers(0, q.size))
            q = np.concatenate([q[:at], [rng.integers(0, SIGMA)], q[at + (k == 0):]]).astype(np.uint8) if k < 2 else np.delete(q, at)
        if q.size <= E:
            continue
        lo = int(rng.integers(0, text.size - 10))
        hi = min(text.size, lo + int(rng.integers(1, 220)))
        d, _, end = rn.align_window(text, q, lo, hi, E, SIGMA)
        seg = rn.forward_segmented(text, q, lo, hi, E, SIGMA, G)
        if d <= E:
            within += 1
            assert seg == (d, end)
        else:
            assert seg is None                                 # never a smaller score than the serial pass has
    assert within >= 10
