"""The batches of the foreign-handle tests (tests/test_foreign_cpu.py, tests/test_foreign_gpu.py): small batches over the text of the
clip tests whose handles are then mixed on purpose, so that the guards of the pileup, of the clipped MD and of the realignment fire.
Pure numpy plus kmer_index_amd.synth: importable without the library and without torch.

A (batch_a): 48 public reads of 40 .. 150 letters cut from the text, as 24 pairs (p, 47 - p) of three kinds, by p % 3:
  0  two reads of ONE length from places 400 letters apart.  At p = 6, 18 the first has one insertion, at p = 12, 21 one deletion
     (m = L + 1 and m = L - 1); in the other four pairs the second carries 1 .. 3 substitutions when it has 80 letters or more.
  1  twins: the first is text[s, s + m), the second text[s + c, s + c + m) with c = 1 or 2 and c or c + 1 substitutions, so its
     distance is at least c: the first read lies inside the band of the second's locus, one diagonal off.
  2  a long read (120 .. 150 letters, substitutions at its quarters) and a short one (40 .. 60), in turn first and second.
  Reads RC of them are reverse-complemented.  Every read has one locus and is placed, so entry e is read e and locus e.
B (batch_b): the reads of A in reverse order: as many reads, loci and entries, and sel[e] = e is the locus of read 47 - e.  Kind 0
  and kind 1 give an interval of the same length (ADDED on the wrong letters, realigned where the band reaches), kind 2 one of
  another length, and the gapped reads of kind 0 one that is a letter off.
C (batch_c): the first 16 reads of A: 16 loci, so sel >= bound for the other 32 entries, and the first 16 are A's own.
D (moved_roff): the roff of A's doubled batch with every entry moved, for the device forms: every offset one further on (the same
  length, the letters of the neighbour at the end), the last one two back; for the public reads LONGER the offset between the two
  strands 30 further on (the forward read 30 letters longer, the reverse one 30 shorter); for the forward-placed public reads
  DECREASING that offset 5 in front of the forward read's start, so the forward read's range decreases.  Every offset stays inside
  [0, the letters of the batch].
N_SHORT: the length of the short index, text[:N_SHORT]: the pairs 0 .. 11 lie below it, read 12 across it, the others behind it.
STRICT: B aligned with max_edits = 2: the loci of its reads with three edits are not aligned (dist 255, start = end = 0).
P, Q (rescue_batches): the pairs 0 .. 23 and 24 .. 39 of chain_data.rescue_pairs_of("dna4_k10"): 18 and 12 rescue jobs, 6 and 4 taken.

CHAIN is CLIP_CHAIN with min_votes = 6.  At min_votes = 2 about forty stray loci of two or three votes, none of them aligned, sit
between the 48 real ones (the CPU chain showed 89 loci), so locus e would no longer be read e and the pairing above would be lost;
the least real locus has more than thirty votes."""
import collections
import functools

import numpy as np

from kmer_index_amd import synth
from tests.chain_data import CLIP_CHAIN, clip_text, other, rc4, rescue_pairs_of

CHAIN = dict(CLIP_CHAIN, min_votes=6)
STRICT = dict(CHAIN, max_edits=2)
N_READS = 48
N_FIRST = 16
N_SHORT = 10_000
RC = (5, 13, 22, 30, 41)
INSERTION, DELETION = (6, 18), (12, 21)
LONGER = (2, 7, 11, 19, 26, 33)
DECREASING = (9, 37)
HARSH = dict(mismatch=255, clip_penalty=0)                     # the clips that keep one '=' run: tl + tr is most of a long read


def _subs(q, places):
    q = q.copy()
    q[list(places)] = other(q[list(places)])
    return q


@functools.lru_cache(maxsize=None)
def batch_a():
    """(the 48 reads, per read (kind, start in the text, m, edits) with kind as above and 3 / 4 for an insertion / a deletion)"""
    t = clip_text()
    z = synth.u64_stream(941, 8 * 24).astype(np.int64) & 0x7FFFFFFF
    reads, meta = [None] * N_READS, [None] * N_READS
    for p in range(24):
        zz = z[8 * p:8 * p + 8]
        s = 300 + 800 * p + int(zz[0] % 100)
        i, j = p, N_READS - 1 - p
        if p % 3 == 2:
            m_long, m_short = 120 + int(zz[1] % 31), 40 + int(zz[2] % 21)
            n_sub = 2 + int(zz[3] % 2)
            big = _subs(t[s:s + m_long], (m_long // 4, m_long // 2, 3 * m_long // 4)[:n_sub])
            small = t[s + 400:s + 400 + m_short].copy()
            a, b = (big, small) if p % 2 else (small, big)
            meta[i], meta[j] = ((2, s, m_long, n_sub), (2, s + 400, m_short, 0)) if p % 2 else ((2, s + 400, m_short, 0), (2, s, m_long, n_sub))
        elif p % 3 == 1:
            m, c = 80 + int(zz[1] % 71), 1 + int(zz[3] % 2)
            n_sub = c + int(zz[4] % 2)
            a = t[s:s + m].copy()
            b = _subs(t[s + c:s + c + m], (m // 4, m // 2, 3 * m // 4)[:n_sub])
            meta[i], meta[j] = (1, s, m, 0), (1, s + c, m, n_sub)
        else:
            m = 40 + int(zz[1] % 111)
            gapped = p in INSERTION + DELETION
            if gapped:
                m = max(m, 70)
            b = t[s + 400:s + 400 + m].copy()
            n_sub = 0
            if p in INSERTION:                                 # m letters over m - 1 of the text
                a = np.insert(t[s:s + m - 1], m // 2, other(t[s + m // 2]))
                meta[i] = (3, s, m, 1)
            elif p in DELETION:                                # m letters over m + 1 of the text
                a = np.delete(t[s:s + m + 1], m // 2)
                meta[i] = (4, s, m, 1)
            else:
                a = t[s:s + m].copy()
                meta[i] = (0, s, m, 0)
                if m >= 80:
                    n_sub = 1 + int(zz[3] % 3)
                    b = _subs(b, (m // 4, m // 2, 3 * m // 4)[:n_sub])
            meta[j] = (0, s + 400, m, n_sub)
        reads[i], reads[j] = np.asarray(a, np.uint8), np.asarray(b, np.uint8)
    for i in RC:
        reads[i] = rc4(reads[i])
    for q in reads:
        q.setflags(write=False)
    return tuple(reads), tuple(meta)


def batch_b():
    return tuple(reversed(batch_a()[0]))


def batch_c():
    return batch_a()[0][:N_FIRST]


def moved_roff(roff2):
    """D: the roff of A's doubled batch (internal read 2i is public read i, 2i + 1 its reverse complement) with every entry moved"""
    roff2 = np.asarray(roff2, np.uint64).astype(np.int64)
    assert roff2.size == 2 * N_READS + 1
    out = roff2 + 1
    out[-1] = roff2[-1] - 2
    for i in LONGER:
        out[2 * i + 1] += 30
    for i in DECREASING:
        out[2 * i + 1] = out[2 * i] - 5
    assert out.min() >= 0 and out.max() <= roff2[-1] and not (out == roff2).any()
    return out.astype(np.uint64)


def rescue_batches():
    """((ranks, roff) of P, (ranks, roff) of Q): interleaved mates"""
    ranks, roff = rescue_pairs_of("dna4_k10")
    cut = lambda a, b: (ranks[int(roff[2 * a]):int(roff[2 * b])].copy(), (roff[2 * a:2 * b + 1] - roff[2 * a]).astype(np.uint64))
    return cut(0, 24), cut(24, 40)


def tally(why):
    """{cause: entries} of the `why` dict that pileup_naive.add or realign_naive.realign filled, and the entries without a cause
    under None"""
    out = collections.Counter(c for causes in why.values() for c in causes)
    out[None] = sum(not causes for causes in why.values())
    return out
