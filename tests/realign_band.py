"""A second implementation of the best value of kmx_scripts_realign, a replay of its runs, and the seeded inputs of
tests/test_realign_bands_cpu.py and tests/test_realign_bands_gpu.py: gaps in every class of the band, texts of low complexity on
which the contract's tie rules decide, the scorings at the bounds of the header, and seeded batches.  No device; never imported by
the package.  tests/realign_naive.py, the contract cell by cell, is not imported here: best_v() is what it is checked against on
inputs larger than an enumeration of paths reaches.

A generator returns a Batch: the tuple (text, voters, aligned) in the style of boundary_reads of tests/test_realign_gpu.py (voter r
fixes the locus at which aligned read r is aligned), with what the tests need to know about the reads as attributes.  `at[r]` is the
text position the read was cut from: the CPU tests align there with tests/align_naive.py, the GPU tests let the voters find it.

An index of sigma = 2 is built at k = 10 like every other one here: the engine asks for 0 < k < 64 / log2(sigma) alone."""
import functools

import numpy as np

from kmer_index_amd import synth
from tests import align_naive as an
from tests import clip_naive as cn
from tests import script_naive as sn

OP_I, OP_D, OP_S, OP_EQ, OP_X = cn.OP_I, cn.OP_D, cn.OP_S, cn.OP_EQ, cn.OP_X
FIELDS = ("match", "mismatch", "gap_open", "gap_extend", "clip_penalty")
INT_MIN, INT_MAX = -2 ** 31, 2 ** 31 - 1
K, VOTE = 10, (1, 8, 2, 0)                                     # the window of every index here; stride, band, min_votes, max_occ of the voters
PAD = 4                                                        # a letter outside every alphabet here: no window holds it
NEG = -(1 << 50)


def scoring(a, b, o, x, p):
    return dict(zip(FIELDS, (a, b, o, x, p)))


DEFAULT, ZERO, ALL_255 = scoring(1, 4, 6, 1, 5), scoring(1, 0, 0, 0, 0), scoring(255, 255, 255, 255, 65535)
SCORINGS = [DEFAULT, ZERO, scoring(1, 1, 0, 1, 0), scoring(1, 4, 6, 0, 5), scoring(1, 4, 0, 1, 5), scoring(2, 1, 0, 1, 1), ALL_255,
            scoring(255, 0, 0, 0, 0), scoring(1, 255, 255, 255, 65535), scoring(1, 0, 255, 0, 0), scoring(1, 0, 0, 255, 0)]


def name_of(s):
    return "a{}_b{}_o{}_x{}_p{}".format(*(s[f] for f in FIELDS))


def class_of(d):
    return 0 if d < 32 else 1 if d < 64 else 2 if d < 128 else 3


# ---- the best value, by rows of whole diagonals ------------------------------------------------------------------------------------------
def best_v(q, t, d, sigma, match=1, mismatch=4, gap_open=6, gap_extend=1, clip_penalty=5, **_):
    """(V, i1, j1) of the contract of tests/realign_naive.py: the greatest V over the cells |j - i| <= d of the rectangle, the least i
    among equals, then the least j.  A row is an array over the diagonals x = j - i + d.  Along a row E(x) = max over x' < x of
    H(x') - o - (x - x') gap_extend; H(x') may be replaced by Ht(x') = max(Z, diagonal, F), because a gap opened right behind one that
    closed costs gap_open >= 0 more than the longer gap, and so E is a running maximum of Ht(x') + x' gap_extend."""
    q, t = np.asarray(q).astype(np.int64), np.asarray(t).astype(np.int64)
    m, L, W = q.size, t.size, 2 * d + 1
    a, b, o, x, p = match, mismatch, gap_open, gap_extend, clip_penalty
    xs = np.arange(W, dtype=np.int64)
    gx = xs * x
    # tp[i + x] = t[j - 1] with j = i + x - d, -1 where there is no such letter
    tp = np.concatenate([np.full(d + 1, -1, np.int64), t, np.full(max(0, m + d - L) + 1, -1, np.int64)])
    j = xs - d
    H = np.where((j >= 0) & (j <= L), 0, NEG)                  # row 0: Z(0) = 0, and no gap run from a 0 is worth more
    F = np.full(W, NEG, np.int64)
    best = (-p if m else 0, 0, 0)
    edge = np.full(1, NEG, np.int64)
    for i in range(1, m + 1):
        j = i + xs - d
        exist = (j >= 0) & (j <= L)
        c = int(q[i - 1])
        diag = H + np.where((tp[i:i + W] == c) & (c < sigma), a, -b)
        F = np.maximum(np.concatenate([F[1:], edge]) - x, np.concatenate([H[1:], edge]) - o - x)
        Ht = np.where(exist, np.maximum(np.maximum(diag, F), -p), NEG)
        E = np.concatenate([edge, np.maximum.accumulate(Ht + gx)[:-1]]) - o - gx
        H = np.where(exist, np.maximum(Ht, E), NEG)
        F = np.where(exist, F, NEG)
        V = np.where(exist, H - (p if i < m else 0), 2 * NEG)
        k = int(np.argmax(V))                                  # (the first of equals: the least j of the row)
        if int(V[k]) > best[0]:                                # (rows ascend: the least i stays)
            best = (int(V[k]), i, i + k - d)
    return best


def replay_score(runs, q, t, tl=0, sigma=4, match=1, mismatch=4, gap_open=6, gap_extend=1, clip_penalty=5, **_):
    """(score, read letters, text letters) of a run list as the realignment writes one: S runs at either end, which cost clip_penalty
    each, and = X I D runs between them, replayed on the read behind the left clip and on the text from t[tl] on.  None when a run
    lies: an '=' over different letters, an X over equal ones, a run past either end, an S run inside."""
    runs = [int(v) for v in runs]
    sl = runs[0] >> 4 if runs and runs[0] & 15 == OP_S else 0
    sr = runs[-1] >> 4 if len(runs) > 1 and runs[-1] & 15 == OP_S else 0
    kept = runs[(sl > 0):len(runs) - (sr > 0)]
    if any(v & 15 == OP_S for v in kept) or sl + sr > len(q):
        return None
    n_read, n_text = cn.letters_of(kept, (OP_EQ, OP_X, OP_I)), cn.letters_of(kept, (OP_EQ, OP_X, OP_D))
    if sl + n_read + sr != len(q) or tl + n_text > len(t) or not sn.replay(q[sl:sl + n_read], t[tl:tl + n_text], kept, sigma)[1]:
        return None
    score = sum(cn.weight(v, match, mismatch, gap_open, gap_extend) for v in kept) - clip_penalty * ((sl > 0) + (sr > 0))
    return score, n_read, n_text


def entries_of(scripts, alignments, ranks, roff, text):
    """(q, t, d) of every entry of the host view of a scripts handle (read_sel_off, sel, cig_off, cigar) over the host view of its
    alignments (dist, start, end, ...)"""
    read_sel_off, sel = scripts[0], scripts[1]
    dist, start, end = alignments[:3]
    read_of = np.repeat(np.arange(len(read_sel_off) - 1), np.diff(np.asarray(read_sel_off, np.int64)))
    return [(ranks[int(roff[r]):int(roff[r + 1])], text[int(start[l]):int(end[l])], int(dist[l])) for r, l in zip(read_of.tolist(), sel.tolist())]


# ---- the inputs ------------------------------------------------------------------------------------------------------------------------------
class Batch(tuple):
    """(text, voters, aligned), and the rest by name"""

    def __new__(cls, text, voters, aligned, **more):
        self = super().__new__(cls, (text, voters, aligned))
        self.__dict__.update(text=text, voters=voters, aligned=aligned, **more)
        return self


def other(q):
    """every letter replaced by another one of the four"""
    return (np.asarray(q, np.uint8) + 2) % 4


def substituted_ends(q, n_left, n_right):
    """q with every other letter of either end replaced, n_left of them from the first letter on and n_right from the last one back:
    what boundary_reads of tests/test_realign_gpu.py does to raise the distance"""
    q = np.array(q, np.uint8)
    assert 2 * (n_left + n_right) <= q.size
    left, right = np.arange(n_left) * 2, q.size - 1 - np.arange(n_right) * 2
    q[left], q[right] = other(q[left]), other(q[right])
    return q


def located(batch, max_edits, sigma=4):
    """(q, t, d, the runs of the script) of every aligned read of a batch at its place `at`, through tests/align_naive.py and
    tests/script_naive.py; a read beyond max_edits has no entry and is left out"""
    out = []
    for q, at in zip(batch.forward if hasattr(batch, "forward") else batch.aligned, batch.at):
        d, s, e = an.align_one(batch.text, q, at, 0, max_edits, sigma)
        if d > max_edits:
            continue
        runs, bad = sn.script_one(q, batch.text[s:e], d, sigma)
        assert not bad
        out.append((q, batch.text[s:e], d, runs))
    return out


@functools.lru_cache(maxsize=None)
def plain_text():
    t = synth.ranks(911, 20_000, 4)                            # the text of tests/test_clip_gpu.py
    t.setflags(write=False)
    return t


def to_distance(text, make, at, target):
    """make(n_left, n_right) with the two counts chosen so that tests/align_naive.py finds exactly `target` edits at `at`: a
    substitution at every other letter of an end is one edit each, give or take what the free ends of the aligner make of the last"""
    n_left = n_right = max(target, 0) // 2
    n_left += target - n_left - n_right
    for _ in range(16):
        q = make(n_left, n_right)
        d = an.align_one(text, q, at, 0, an.MAX_EDITS, 4)[0]
        if d == target:
            return q
        n_left += target - d
    raise AssertionError(f"no read at distance {target}")


# Gaps in every class.  g = 12, 24, 48, 72 letters: at NPL = 1, 2, 4, 8 diagonals per lane a gap run crosses g / NPL >= 9 lanes.  Under
# the default scoring a clip in place of the gap costs p = 5 and loses a flank, the gap o + g x = 6 + g: a clean flank of more than
# 11 + g letters on either side keeps the gap.  The unit-cost aligner in front asks for more: it takes the gap (g edits) only where
# aligning the far flank at the wrong place costs more, and random text of four letters aligns to itself at about half an edit per
# letter, so a flank holds 2 g + 24 clean letters.  n_ends substitutions at every other letter of both ends put the distance
# n_ends + g (+ g) inside the class; the read is those 2 n_ends letters, its flanks and its insertion.
GAPS = (12, 24, 48, 72)
ENDS = ((8, 4), (20, 8), (30, 12), (70, 16))                   # the substitutions of a read with one gap, with both: d = 20 / 28, 44 / 56, 78 / 108, 142 / 160
BOUNDARIES = (31, 32, 63, 64, 127, 128, 250)


@functools.lru_cache(maxsize=None)
def class_gaps():
    """Three reads per class of the band (an interior deletion of g text letters, an interior insertion of g random letters, both)
    and one read with a deletion of 12 letters per distance of BOUNDARIES.  kind[r], g[r], klass[r]: what was planted and the class
    the distance is meant to fall into; exact[r]: the distance itself for the boundary reads, else None."""
    t = plain_text()
    rng = np.random.default_rng(7301)
    at, aligned, kind, gs, cls, exact = [], [], [], [], [], []
    s = 600
    for c, (g, ends) in enumerate(zip(GAPS, ENDS)):
        flank = 2 * g + 24
        for what, n in (("D", ends[0]), ("I", ends[0]), ("DI", ends[1])):
            edge = flank + n                                   # an outer flank carries n / 2 substitutions at every other letter: n letters
            parts, pos = [t[s:s + edge]], s + edge
            for op in what:
                inner = flank if op != what[-1] else edge
                if op == "D":
                    pos += g
                else:
                    parts.append(rng.integers(0, 4, g).astype(np.uint8))
                parts.append(t[pos:pos + inner])
                pos += inner
            q = np.concatenate(parts)
            aligned.append(substituted_ends(q, n - n // 2, n // 2))
            at.append(s); kind.append(what); gs.append(g); cls.append(c); exact.append(None)
            s = pos + 300
    for target in BOUNDARIES:
        n = target - 12
        m = 2 * n + 2 * 48 + 8                                 # 48 clean letters on either side of the deletion, and room for the search
        cut = s + m // 2

        def make(n_left, n_right, s=s, m=m, cut=cut):
            return substituted_ends(np.concatenate([t[s:cut], t[cut + 12:s + m + 12]]), n_left, n_right)

        aligned.append(to_distance(t, make, s, target))
        at.append(s); kind.append("D"); gs.append(12); cls.append(class_of(target)); exact.append(target)
        s += m + 12 + 300
    assert s < t.size
    voters = [t[a:a + 150].copy() for a in at]
    return Batch(t, voters, aligned, at=at, kind=kind, g=gs, klass=cls, exact=exact, sigma=4)


# ---- texts on which the tie rules decide ---------------------------------------------------------------------------------------------------
UNITS = (1, 2, 3, 7, 1, 2, 3, 7)
SEP = 200                                                      # random letters in front of every repeat
REPS = (300, 300, 300, 300, 60, 60, 60, 60)                    # the letters of the repeats: four that no read spans, four that a read does
REP_AT = tuple(SEP * (b + 1) + sum(REPS[:b]) for b in range(len(REPS)))


@functools.lru_cache(maxsize=None)
def tandem_text():
    """200 random letters and a tandem repeat, for units of 1, 2, 3, 7 letters over 300 letters each and again over 60 letters each,
    and 200 random letters: 3240.  A gap inside a repeat of 300 letters cannot be told from a shorter read by a read of 200 that ends
    inside the repeat, so the short repeats are there for reads that cross one with a gap that can sit anywhere in it."""
    parts = []
    for b, (u, rep) in enumerate(zip(UNITS, REPS)):
        unit = synth.ranks(940 + b, u, 4)
        if u > 1 and (unit == unit[0]).all():
            unit[-1] = (unit[0] + 1) % 4
        parts += [synth.ranks(950 + b, SEP, 4), np.tile(unit, rep // u + 1)[:rep]]
    t = np.concatenate(parts + [synth.ranks(960, SEP, 4)])
    assert all((t[at:at + u] == t[at + u:at + 2 * u]).all() for at, u in zip(REP_AT, UNITS))
    t.setflags(write=False)
    return t


@functools.lru_cache(maxsize=None)
def repeat_text():
    """2000 random letters, a 50-letter unit 140 times, 2000 random letters, a reverse palindrome x + rc(x) of 40 letters: the text of
    tests/test_secondaries_gpu.repeat_text, restated"""
    unit, x = synth.ranks(501, 50, 4), synth.ranks(502, 20, 4)
    t = np.concatenate([synth.ranks(503, 2000, 4), np.tile(unit, 140), synth.ranks(504, 2000, 4), x, (3 - x[::-1]).astype(np.uint8)])
    t.setflags(write=False)
    return t


@functools.lru_cache(maxsize=None)
def binary_text():
    t = synth.ranks(921, 4000, 2)
    t.setflags(write=False)
    return t


def edit(region, edits, sigma):
    """region with (pos, 'D' / 'I', n) applied from the last to the first; an insertion repeats the n letters in front of pos, so
    that inside a repeat it is a copy of the repeat; the letter in front of every gap is substituted"""
    q = np.array(region, np.uint8)
    for pos, op, n in sorted(edits, reverse=True):
        sub = pos - 1 if op == "D" else pos - 1 - n            # (in front of the letters an insertion copies)
        q[sub] = (q[sub] + 1) % sigma
        q = np.concatenate([q[:pos], q[pos + n:]]) if op == "D" else np.concatenate([q[:pos], q[pos - n:pos], q[pos:]])
    return q


def voter_of(text, at, unique):
    """A read whose windows vote for the diagonal `at` alone: PAD letters up to the first stretch of `unique` text at or behind `at`,
    then up to 60 letters of it"""
    for lo, hi in unique:
        u0 = max(at, lo)
        u1 = min(hi, u0 + 60)
        if u1 - u0 >= 30:
            assert u1 - at <= an.MAX_READ
            return np.concatenate([np.full(u0 - at, PAD, np.uint8), text[u0:u1]])
    raise AssertionError(f"no unique text behind {at}")


def tandem_specs():
    """(at, letters, edits) of the reads of the tandem text.  Blocks 0 .. 3: an even one starts 50 letters in front of its repeat and
    ends inside it, an odd one starts inside and ends 50 letters behind it.  Blocks 4 .. 7: 60 letters in front of the repeat, the
    repeat, 60 letters behind it.  The gaps are whole units inside the repeat, so they can sit anywhere in it; blocks 2, 3 and 6
    carry a deletion and an insertion."""
    out = []
    for b, (u, rep) in enumerate(zip(UNITS, REP_AT)):
        n = {1: 4, 2: 4, 3: 6, 7: 7}[u]
        if b >= 4:
            at, m = rep - 60, 180
            edits = [(60 + 30, "DI"[b % 2], n)] + ([(60 + 50, "I", n)] if b == 6 else [])
        elif b % 2 == 0:
            at, m = rep - 50, 140 + 10 * b
            edits = [(50 + 40, "D", n)] + ([(50 + 70, "I", n)] if b == 2 else [])
        else:
            m = 60 + 20 * b
            at = rep + REPS[b] + 50 - m
            edits = [(m - 50 - 30, "I", n)] + ([(m - 50 - 60, "D", n)] if b == 3 else [])
        out.append((at, m, edits))
    return out


def cut_reads(text, specs, sigma, unique, raised=0):
    """The Batch of the (at, letters, edits) of `specs`.  raised > 0: every read is cut with room for substituted ends in front
    and behind, and these are chosen so that the distance at `at` is exactly `raised`."""
    at, aligned = [], []
    for r, (a, m, edits) in enumerate(specs):
        if not raised:
            q = edit(text[a:a + m + sum(n for _, op, n in edits if op == "D")], edits, sigma)
            if r % 3:                                          # the last letter, or the one in front of it: '=X' and '=X=' at the end
                q[-(r % 3)] = (q[-(r % 3)] + 1) % sigma
            at.append(a)
            aligned.append(q)
            continue
        room = raised + 4
        full = m + sum(n for _, op, n in edits if op == "D")
        a0 = a - room
        shifted = [(pos + room, op, n) for pos, op, n in edits]
        q = edit(text[a0:a0 + full + 2 * room], shifted, sigma)
        at.append(a0)
        aligned.append(to_distance(text, lambda n_left, n_right, q=q: substituted_ends(q, max(n_left, 0), n_right), a0, raised))
    voters = [text[a:a + 150].copy() if unique is None else voter_of(text, a, unique) for a in at]
    return Batch(text, voters, aligned, at=at, sigma=sigma)


TANDEM_UNIQUE = tuple((at - SEP, at) for at in REP_AT) + ((REP_AT[-1] + REPS[-1], REP_AT[-1] + REPS[-1] + SEP),)
RAISED = ((40, 36), (70, 67), (130, 129))                      # max_edits and the distance of the raised reads: NPL = 2, 4, 8


@functools.lru_cache(maxsize=None)
def tandem_reads(raised=0):
    """the eight reads of the tandem text; raised: the four that cross a repeat (a unit of every length, a deletion, an insertion
    and both), which is what the oracle of a band of 259 diagonals has the time for"""
    return cut_reads(tandem_text(), tandem_specs()[4:] if raised else tandem_specs(), 4, TANDEM_UNIQUE, raised)


@functools.lru_cache(maxsize=None)
def tie_texts():
    """Three batches.  binary: random text of two letters, eight reads of 60 .. 200 letters with a deletion of three letters, every
    other one with an insertion as well.  tandem: tandem_reads().  repeat: the 50-letter unit, two reads that start in front of the
    repeat and end inside and two that start inside, one with a whole unit deleted (50 letters: NPL = 2)."""
    b = binary_text()
    specs = [(300 + 400 * i, 60 + 20 * i, [(30, "D", 3)] + ([(45, "I", 2)] if i % 2 else [])) for i in range(8)]
    r = repeat_text()
    rspecs = [(1950, 150, [(100, "D", 5)]), (8900, 160, [(50, "I", 4)]), (1940, 200, [(110, "D", 50)]), (8880, 180, [(40, "D", 3), (80, "I", 3)])]
    return (cut_reads(b, specs, 2, None), tandem_reads(), cut_reads(r, rspecs, 4, ((0, 2000), (9000, 11_000))))


TIE_NAMES = ("binary", "tandem", "repeat")
TIE_EDITS = 64                                                 # max_edits of the tie batches as they are


# ---- seeded batches ---------------------------------------------------------------------------------------------------------------------------
FUZZ_CHAIN = dict(band=8, min_votes=2, max_edits=64, max_span=64)
COMP4 = np.asarray([3, 2, 1, 0], np.uint8)


@functools.lru_cache(maxsize=None)
def fuzz_text():
    t = np.concatenate([synth.ranks(931, 4000, 4), tandem_text()])
    t.setflags(write=False)
    return t


def revcomp(q):
    """the reverse complement as the chain makes it: a letter outside the alphabet stays"""
    q = np.asarray(q, np.uint8)[::-1]
    return np.where(q < 4, COMP4[np.minimum(q, 3)], q).astype(np.uint8)


def fuzz_batch(seed):
    """32 reads of 20 .. 160 letters, two in three from the random part of fuzz_text() and the rest from its tandem part, with
    0 .. 10 edits each: substitutions (one in eight by a letter outside the alphabet), insertions and deletions of 1 .. 12 letters
    anywhere, the ends included.  Every third read is reverse-complemented: `aligned` (= `voters`) are the public reads, `forward`
    what the chain aligns at `at`.  scoring, min_score: what the batch is realigned and clipped under."""
    rng = np.random.default_rng(88_000 + seed)
    t = fuzz_text()
    forward, at = [], []
    for i in range(32):
        m = int(rng.integers(20, 161))
        s = int(rng.integers(100, 3700)) if i % 3 != 2 else 4000 + int(rng.integers(100, tandem_text().size - 300))
        q = t[s:s + m].copy()
        for _ in range(int(rng.integers(0, 11))):
            op, n, pos = int(rng.integers(0, 3)), int(rng.integers(1, 13)), int(rng.integers(0, q.size + 1))
            if op == 0:
                pos = min(pos, q.size - 1)
                q[pos] = PAD if rng.integers(0, 8) == 0 else (q[pos] + 1 + rng.integers(0, 3)) % 4
            elif op == 1 and q.size + n <= 160:
                q = np.concatenate([q[:pos], rng.integers(0, 5, n).astype(np.uint8), q[pos:]])
            elif op == 2 and q.size - n >= 20:
                pos = min(pos, q.size - n)
                q = np.concatenate([q[:pos], q[pos + n:]])
        forward.append(q)
        at.append(s)
    reads = [revcomp(q) if i % 3 == 0 else q for i, q in enumerate(forward)]
    pick = lambda values: int(values[int(rng.integers(0, len(values)))])
    few = (0, 1, 2, 6, 255)
    sc = scoring(pick((1, 2, 255)), pick(few), pick(few), pick(few), pick((0, 5, 65535)))
    return Batch(t, reads, reads, forward=forward, at=at, sigma=4, scoring=sc, min_score=pick((INT_MIN, 0, 40, INT_MAX)))
