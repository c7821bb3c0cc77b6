"""What the tests of the mapping chain share as data: the texts, the read and pair workloads, the constants that travel with them
and the field names of the handles.  Pure numpy plus kmer_index_amd.synth and the naive models: importable without the library and
without torch.  The floors that the GPU tests assert were confirmed once, on the CPU, for the exact bytes these generators give;
tests/test_chain_data_cpu.py pins those bytes.  The layouts and batches of the chain's front: tests/front_data.py."""
import functools

import numpy as np

from kmer_index_amd import synth
from tests import fold_naive as fn
from tests import pair_naive as pn
from tests import rescue_naive as rn
from tests.helpers import pack

# ---- the field names of the handles -------------------------------------------------------------------------------------------------------
HITS = ("win_off", "hit_off", "positions", "status")
LOCI = ("locus_off", "diag", "span", "votes", "skipped")
ALIGN = ("dist", "start", "end", "best", "aligned")
FOLD = ("locus", "strand", "dist", "start", "end", "second", "best2")
PLACEMENTS, PAIRS, JOBS = pn.PLACEMENTS, pn.PAIRS, rn.JOBS
SCRIPTS = ("read_sel_off", "sel", "cig_off", "cigar")
MD = ("md_off", "md")
CLIPS = ("score", "sl", "sr", "tl", "tr", "nm", "cflags", "cig_off", "cigar")

# ---- alphabets and strands ----------------------------------------------------------------------------------------------------------------
COMPLEMENT = {4: (3, 2, 1, 0), 5: (4, 2, 1, 3, 0), 20: tuple(range(20))}      # dna4, dna5 (N is its own complement), the plain reversal
COMP4 = np.asarray([3, 2, 1, 0], np.uint8)
LETTERS = {4: "ACGT", 20: "ACDEFGHIKLMNPQRSTVWY"}
LETTERS4 = LETTERS[4]


@functools.lru_cache(maxsize=None)
def text_of(sigma, n=50_000):
    t = synth.ranks(7 + sigma, n, sigma)
    t.setflags(write=False)
    return t


def rc(q, sigma=4):
    return fn.revcomp(q, COMPLEMENT[sigma], sigma)


def rc4(q):
    return fn.revcomp(q, COMP4, 4)


def frozen(ranks, roff):
    ranks.setflags(write=False)
    roff.setflags(write=False)
    return ranks, roff


def kill(q, k):
    """a substitution at every k-th letter from letter k - 2 on: no window of k letters survives, the first and the last letter do"""
    q = np.array(q, np.uint8)
    q[k - 2::k] = (q[k - 2::k] + 1) % (4 if k == 10 else 20)
    return q


def other(q):
    """every letter replaced by another one"""
    return (np.asarray(q, np.uint8) + 2) % 4


def edited(z, q, n_edits):
    """q with n_edits random edits (substitutions, insertions, deletions) at random places, from the numbers z"""
    q = list(int(x) for x in q)
    for k in range(n_edits):
        kind, at, letter = int(z[3 * k] % 3), int(z[3 * k + 1] % max(len(q), 1)), int(z[3 * k + 2] % 4)
        if kind == 0 and q:
            q[at] = (q[at] + 1 + letter % 3) % 4
        elif kind == 1:
            q.insert(at, letter)
        elif q:
            del q[at]
    return np.asarray(q, np.uint8)


# ---- the single reads of the vote, align, script and strand-fold tests ----------------------------------------------------------------------
# name: (sigma, k, text length, reads of the generator)
READ_WORKLOADS = {"dna4_k10": (4, 10, 50_000, 3000), "aa20_k5": (20, 5, 50_000, 3000), "dna4_k5": (4, 5, 100_000, 300)}
N_READS = 600                     # the align, script and strand-fold tests take the first so many
# Floors on what the strand fold is given, from tests/align_naive.py and tests/fold_naive.py on the CPU (a dictionary of the text's
# k-mers, vote_naive.vote, align_naive.align, fold_naive.fold; never from the engine): (workload, band) -> (n_placed exactly, placed
# on the forward strand at least, placed on the reverse strand at least, placed reads with two or more aligned loci and second == 255
# at least), for reads_of(name, N_READS, reverse_odd=True).  The even reads (kinds 0 and 2) are cut from the forward strand, the odd
# reads of kind 1 from the reverse one.  Kind 1 carries a substitution every 25 letters, so only its reads of up to about 212 letters
# stay within 8 edits, which is why the reverse strand holds somewhat under a third of the placed reads and not half.  At band 8 a
# read's split diagonals join into one locus, so the last figure is the business of the band 0 case.
STRAND_FLOORS = {
    ("dna4_k10", 8): (370, 268, 102, 1),
    ("aa20_k5", 8): (374, 268, 106, 0),
    ("dna4_k10", 0): (370, 268, 102, 118),
}


@functools.lru_cache(maxsize=None)
def reads_of(name, n_reads=None, meta=None, reverse_odd=False):
    """The first n_reads reads of a workload (all of them by default).  Read i has m = z % 301 letters and kind i % 4: 3 is random
    letters, the others are cut from the text (at 0 when i % 40 == 0, flush with its end when i % 40 == 4, else anywhere); kind 1 with
    m > 40 gets a substitution at letters 12, 37, 62, ...; kind 2 with m > 60 loses the letter at m / 3 and has the one at 2m / 3
    twice.  i % 40 == 8 / 12 with m >= 40: 20 random letters in front of text[:m - 20] / behind text[n - (m - 20):], reads that
    overhang the text.  Every 50th read carries one letter >= sigma, at its first, last and middle letter in turn.  reverse_odd: every
    odd-numbered read is reverse-complemented afterwards.  Returns (ranks, roff), and with meta a third item, per read
    (kind, s, m, plain) for meta="plain" and (kind, s, m, plain, bad) for meta="bad": plain = cut from the text at s and left as it
    was, bad = carries a letter >= sigma."""
    sigma, _, n, n_all = READ_WORKLOADS[name]
    text = text_of(sigma, n)
    z = synth.u64_stream(4241 + sigma + n_all, 2 * n_all).astype(np.int64) & 0x7FFFFFFF
    reads, side = [], []
    n_bad = 0
    for i in range(n_all if n_reads is None else n_reads):
        m, kind = int(z[2 * i] % 301), i % 4
        s, plain = -1, False
        if kind == 3:
            q = synth.ranks(900_001 + i, m, sigma)
        elif i % 40 == 8 and m >= 40:
            q = np.concatenate([synth.ranks(700_001 + i, 20, sigma), text[:m - 20]])
        elif i % 40 == 12 and m >= 40:
            q = np.concatenate([text[n - (m - 20):], synth.ranks(800_001 + i, 20, sigma)])
        else:
            s = 0 if i % 40 == 0 else n - m if i % 40 == 4 else int(z[2 * i + 1] % (n - m - 1 + 1))
            if kind == 2 and m > 60:
                q = text[s:s + m + 1].copy()
                q = np.delete(q, m // 3)[:m]                               # one letter gone ...
                q = np.insert(q, 2 * m // 3, q[2 * m // 3])[:m]            # ... and one twice
            else:
                q = text[s:s + m].copy()
                if kind == 1 and m > 40:
                    q[12::25] = (q[12::25] + 1) % sigma
            plain = kind == 0
        bad = i % 50 == 7 and m > 0
        if bad:
            q[(0, m - 1, m // 2)[n_bad % 3]] = (sigma, 255)[(n_bad // 3) % 2]
            n_bad += 1
            plain = False
        q = np.asarray(q, np.uint8)
        reads.append(fn.revcomp(q, COMPLEMENT[sigma], sigma) if reverse_odd and i % 2 else q)
        side.append((kind, s, m, plain, bad) if meta == "bad" else (kind, s, m, plain))
    ranks, roff = frozen(*pack(reads))
    return (ranks, roff, side) if meta else (ranks, roff)


# ---- the pairs of the pair, rescue, tag, contig, secondary and clip tests -----------------------------------------------------------------
# (sigma, k, text length)
PAIR_WORKLOADS = {"dna4_k10": (4, 10, 50_000), "aa20_k5": (20, 5, 50_000)}
N_PAIRS = 300
CHAIN = dict(band=8, min_votes=2, max_edits=8, max_span=64)
INSERT = dict(min_insert=100, max_insert=600)
# Floors on (n_concordant, n_discordant, n_single) of pairs_of, from the naive chain on the CPU (a dictionary of the text's k-mers,
# vote_naive.vote, align_naive.align on fold_naive.double_reads of the mates, pair_naive.fold_pairs; never from the engine).  Of the
# 300 pairs the 30 with p % 10 == 0 (mates 5000 apart) and the 30 with p % 10 == 3 (both mates on one strand) are discordant, the 30
# with p % 10 == 5 keep one mate, the 30 with p % 10 == 7 none, and the other 180 are concordant.
PAIR_FLOORS = {"dna4_k10": (180, 60, 30), "aa20_k5": (180, 60, 30)}
# Pairs of rescue_pairs_of that are MATE1_ONLY / MATE2_ONLY after the pair fold and CONCORDANT after the rescue, from the naive chain
# on the CPU (naive_floor of tests/test_rescue_gpu.py: a dictionary of the text's k-mers, vote_naive.vote, align_naive.align,
# pair_naive.fold_pairs, rescue_naive.rescue; never from the engine).  75 pairs are planted, and every one of them comes out ONLY and
# is rescued.
RESCUE_FLOORS = {"dna4_k10": 75, "aa20_k5": 75}


@functools.lru_cache(maxsize=None)
def pairs_of(name):
    """N_PAIRS pairs as interleaved mates.  Pair p comes from a fragment of 200 .. 500 letters, taken from the reverse strand when p is
    odd (then mate 2 is the upstream one); mate 1 is its first 80 .. 150 letters, mate 2 the reverse complement of its last 80 .. 150.
    p % 4 == 0: mate 1 carries a substitution at letters 10, 40, 70, ... and mate 2 loses its middle letter.  p % 10 == 0: mate 2 is
    cut 5000 letters downstream instead; == 3: mate 2 is not reverse-complemented (both on one strand); == 5: one mate is random
    letters (mate 1 and mate 2 in turn); == 7: both are."""
    sigma, _, n = PAIR_WORKLOADS[name]
    text = text_of(sigma, n)
    z = synth.u64_stream(977 + sigma, 4 * N_PAIRS).astype(np.int64) & 0x7FFFFFFF
    reads = []
    for p in range(N_PAIRS):
        f, m1, m2 = 200 + int(z[4 * p] % 301), 80 + int(z[4 * p + 1] % 71), 80 + int(z[4 * p + 2] % 71)
        s = int(z[4 * p + 3] % (n - 6000))
        frag = rc(text[s:s + f], sigma) if p % 2 else text[s:s + f]      # odd: the fragment as the reverse strand has it
        mate1 = frag[:m1].copy()
        mate2 = rc(text[s + 5000:s + 5000 + m2] if p % 10 == 0 else frag[f - m2:], sigma)
        if p % 10 == 3:
            mate2 = rc(mate2, sigma)
        if p % 4 == 0:
            mate1[10::30] = (mate1[10::30] + 1) % sigma
            mate2 = np.delete(mate2, m2 // 2)
        if p % 10 == 7 or p % 20 == 5:
            mate1 = synth.ranks(600_001 + p, m1, sigma)
        if p % 10 == 7 or p % 20 == 15:
            mate2 = synth.ranks(610_001 + p, m2, sigma)
        reads += [np.asarray(mate1, np.uint8), np.asarray(mate2, np.uint8)]
    return frozen(*pack(reads))


@functools.lru_cache(maxsize=None)
def rescue_pairs_of(name):
    """N_PAIRS pairs as interleaved mates, cut as pairs_of cuts them: from a fragment of 200 .. 500 letters, taken from the reverse
    strand when (p // 8) is odd.  By p % 4, with `lost` = (p // 4) % 2 the mate it is done to, of 8 k letters: 0: the lost mate has a
    substitution at every k-th letter (8 edits, no intact window); 1: it is random letters; 2: it is cut 5000 letters downstream and
    broken as in 0; 3: an ordinary pair."""
    sigma, k, n = PAIR_WORKLOADS[name]
    text = text_of(sigma, n)
    z = synth.u64_stream(1977 + sigma, 4 * N_PAIRS).astype(np.int64) & 0x7FFFFFFF
    reads = []
    for p in range(N_PAIRS):
        kind, lost, rev = p % 4, (p // 4) % 2, (p // 8) % 2
        f, m = 200 + int(z[4 * p] % 301), [80 + int(z[4 * p + 1] % 71), 80 + int(z[4 * p + 2] % 71)]
        s = int(z[4 * p + 3] % (n - 6000))
        if kind != 3:
            m[lost] = 8 * k
        g = rc(text[s:s + f], sigma) if rev else text[s:s + f]
        mates = [g[:m[0]].copy(), rc(g[f - m[1]:], sigma)]
        if kind == 0:
            mates[lost] = kill(mates[lost], k)
        elif kind == 1:
            mates[lost] = synth.ranks(700_001 + p, m[lost], sigma)
        elif kind == 2:
            far = text[s + 5000:s + 5000 + m[lost]]
            mates[lost] = kill(far if (lost == 0) != bool(rev) else rc(far, sigma), k)
        reads += [np.asarray(x, np.uint8) for x in mates]
    return frozen(*pack(reads))


# ---- the repeat text ------------------------------------------------------------------------------------------------------------------------
REPEAT_CHAIN = dict(band=0, min_votes=2, max_edits=8)


@functools.lru_cache(maxsize=None)
def repeat_text():
    """2000 random letters, a 50-letter unit 140 times, 2000 random letters, a reverse palindrome x + rc(x) of 40 letters"""
    unit = synth.ranks(501, 50, 4)
    x = synth.ranks(502, 20, 4)
    t = np.concatenate([synth.ranks(503, 2000, 4), np.tile(unit, 140), synth.ranks(504, 2000, 4), x, rc(x)])
    t.setflags(write=False)
    return t, unit


def repeat_pair():
    text, _ = repeat_text()
    return pack([text[8800:8900].copy(), rc(text[9200:9300])])


# ---- texts with planted copies ------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def copies_text():
    """The dna4 text with, for pair 0, an exact second copy of mate 2's source at 30000 and the true copy near the anchor broken; for
    pair 1, region 15000 with mate 1's source and a broken copy of mate 2's, region 35000 the other way round."""
    t = text_of(4, 50_000).copy()
    t[30_000:30_080] = t[10_320:10_400]
    t[10_320:10_400] = kill(t[10_320:10_400], 10)
    t[35_000:35_080] = kill(t[15_000:15_080], 10)
    t[15_320:15_400] = kill(t[35_320:35_400], 10)
    t.setflags(write=False)
    return t


PLANT_AT = (500, 1500, 2600, 3700, 4900)      # exact, exact, 1 substitution, 3 substitutions, exact but reverse-complemented


@functools.lru_cache(maxsize=None)
def planted_text():
    t = synth.ranks(811, 6000, 4).copy()
    seg = synth.ranks(812, 120, 4)
    one, three = seg.copy(), seg.copy()
    one[60] = (one[60] + 1) % 4
    three[[25, 60, 95]] = (three[[25, 60, 95]] + 2) % 4
    for at, copy in zip(PLANT_AT, (seg, seg, one, three, rc4(seg))):
        t[at:at + 120] = copy
    t.setflags(write=False)
    return t, seg


# ---- the text with contigs 12 and 13 alike------------------------------------------------------------------------------------------------
PAIR_SIZES = (1500,) * 12 + (300, 300) + (1500,) * 12          # contigs 12 and 13 hold the same 300 letters


def table_of(sizes):
    return np.concatenate([[0], np.cumsum(sizes)]).astype(np.uint64)


@functools.lru_cache(maxsize=None)
def pair_text():
    t = synth.ranks(91, sum(PAIR_SIZES), 4).copy()
    off = table_of(PAIR_SIZES).astype(np.int64)
    t[off[13]:off[14]] = t[off[12]:off[13]]
    t.setflags(write=False)
    return t


# ---- the planted reads of the clip, realign and pileup tests ----------------------------------------------------------------------------------
N, K, M = 20_000, 10, 150
CLIP_E = 24
CLIP_CHAIN = dict(band=8, min_votes=2, max_edits=CLIP_E, max_span=64)
CLIP_SIZES = (7000, 5000, 8000)                                # the contigs of the junction tests: junctions at 7000 and 12 000


@functools.lru_cache(maxsize=None)
def clip_text():
    t = synth.ranks(911, N, 4)
    t.setflags(write=False)
    return t


# the planted reads by name, then fillers: 150 letters from random places with 0 .. 3 edits
CLIP_PLANTED = ("unedited", "three_subs", "tail", "tail_reverse", "over_end", "over_start", "outside")


@functools.lru_cache(maxsize=None)
def clip_planted_reads():
    t = clip_text()
    subs = t[2000:2000 + M].copy()
    subs[[0, 2, 4]] = other(subs[[0, 2, 4]])
    reads = [t[1000:1000 + M].copy(), subs, np.concatenate([t[3000:3138], other(t[3138:3150])]),
             rc4(np.concatenate([t[4000:4138], other(t[4138:4150])])), np.concatenate([t[N - 140:], np.full(10, (int(t[N - 1]) + 2) % 4, np.uint8)]),
             np.concatenate([other(t[N - 10:]), t[:140]]), np.full(M, 4, np.uint8)]
    z = synth.u64_stream(912, 16 * 40).astype(np.int64) & 0x7FFFFFFF
    for p in range(40):
        zz = z[16 * p:16 * p + 16]
        s = 5000 + int(zz[0] % 10_000)
        q = edited(zz[2:], t[s:s + M], int(zz[1] % 4))
        reads.append(rc4(q) if p % 2 else q)
    return reads


def table_reads():
    """the two reads of the realignment's table and a chimera: a deletion of 12 letters, an insertion of 4, and 120 + 30 letters of
    two places"""
    t = clip_text()
    return [np.concatenate([t[8000:8070], t[8082:8162]]), np.concatenate([t[6000:6070], other(t[6070:6074]), t[6070:6146]]),
            np.concatenate([t[7000:7120], t[12_000:12_030]])]


def realign_batch():
    return clip_planted_reads() + table_reads()


def boundary_reads():
    """(the reads that vote, the reads that are aligned at their loci): substitutions at every other letter of both ends, so that the
    distance falls into each class of the band (< 32, 32 .. 63, 64 .. 127, >= 128), the read of 1024 letters of tests/test_clip_gpu.py
    among them, and reads of 1, 63, 64, 65, 128 and 129 letters"""
    t = clip_text()
    voters, aligned = [], []
    for s, m, w in ((9000, 200, 16), (9500, 300, 50), (10_000, 400, 100), (10_500, 600, 170), (6000, 1024, 250), (11_200, 1, 0), (11_400, 63, 6),
                    (11_600, 64, 6), (11_800, 65, 6), (12_000, 128, 6), (12_200, 129, 6)):
        q = t[s:s + m].copy()
        if w:
            q[0:w:2] = other(q[0:w:2])
            q[m - w::2] = other(q[m - w::2])
        if m == 1024:
            q[300:701:100] = other(q[300:701:100])
        voters.append(t[s:s + M].copy())
        aligned.append(q)
    return voters, aligned


# ---- the planted reads of the supplementary tests -------------------------------------------------------------------------------------------
# the shapes of the clip tests.  SUPP_E: a planted part of L >= 40 letters leaves at most M - L <= 110 letters of the read to be
# edits, so every such part is aligned at its locus whatever the rest of the read does there
SUPP_E = 110
SUPP_CHAIN = dict(band=8, min_votes=2, max_edits=SUPP_E, max_span=64)
COPIES = 66                                                    # of either unit: 132 entries for the read made of the two


@functools.lru_cache(maxsize=None)
def units():
    return synth.ranks(932, 40, 4), synth.ranks(933, 40, 4)


@functools.lru_cache(maxsize=None)
def supp_text():
    """20 000 random letters; text[9000:9050] occurs again at 11 000; either unit of 40 letters occurs 66 times, 50 letters apart"""
    t = synth.ranks(931, N, 4).copy()
    t[11_000:11_050] = t[9000:9050]
    for c in range(COPIES):
        t[12_000 + 50 * c:12_040 + 50 * c] = units()[0]
        t[16_000 + 50 * c:16_040 + 50 * c] = units()[1]
    t.setflags(write=False)
    return t


# the planted reads by name, then 40 fillers: 150 letters from random places with 0 .. 3 edits, every other one reverse-complemented
SUPP_PLANTED = ("plain", "split", "split_rc", "split_rc_whole", "three", "dup", "adapter", "short", "tandem", "inverted", "many", "outside")


@functools.lru_cache(maxsize=None)
def supp_planted_reads():
    t, cat = supp_text(), np.concatenate
    split_rc = cat([t[2500:2600], rc4(t[5500:5550])])
    reads = [t[1000:1150].copy(),                              # plain
             cat([t[2000:2100], t[5000:5050]]),                # split: 100 + 50 on one strand
             split_rc,                                         # the second part reverse-complemented
             rc4(split_rc),                                    # the whole of it reverse-complemented: the primary lies on strand 1
             cat([t[3000:3060], t[6000:6050], t[7500:7540]]),  # three parts
             cat([t[3500:3600], t[9000:9050]]),                # the second part is the segment that occurs twice
             cat([t[4000:4120], synth.ranks(934, 30, 4)]),     # an adapter tail
             cat([t[4500:4635], t[8000:8015]]),                # a second part below min_len
             cat([t[6500:6600], t[6530:6580]]),                # a tandem duplication on one strand
             cat([t[7000:7100], rc4(t[7030:7080])]),           # the same with the second part inverted
             cat(units()),                                     # 66 loci for either half
             np.full(M, 4, np.uint8)]                          # no letter of the alphabet
    z = synth.u64_stream(935, 16 * 40).astype(np.int64) & 0x7FFFFFFF
    for p in range(40):
        zz = z[16 * p:16 * p + 16]
        s = 200 + int(zz[0] % 10_000)
        q = edited(zz[2:], t[s:s + M], int(zz[1] % 4))
        reads.append(rc4(q) if p % 2 else q)
    return reads


# ---- the scorings of the realignment small enough for an enumeration of every path ---------------------------------------------------------
SMALL_SCORINGS = {
    "default": dict(),
    "free_clips": dict(clip_penalty=0),
    "all_zero": dict(mismatch=0, gap_open=0, gap_extend=0, clip_penalty=0),
    "zeros_p3": dict(mismatch=0, gap_open=0, gap_extend=0, clip_penalty=3),
    "a2_b1_o0_x1_p1": dict(match=2, mismatch=1, gap_open=0, gap_extend=1, clip_penalty=1),
}


# ---- the tiny chain of tests/test_handle_views_gpu.py -------------------------------------------------------------------------------------------
TINY_N = 6000
TINY_E = 110                                                   # as SUPP_E: any locus with three votes is aligned, whatever the rest of the read does there
TINY_CHAIN = dict(band=8, min_votes=3, max_edits=TINY_E, max_span=64)
TINY_INSERT = dict(min_insert=100, max_insert=600)
TINY_CONTIGS = (2500, 3500)


@functools.lru_cache(maxsize=None)
def tiny_text():
    """6000 random letters; text[3000:3050] occurs again at 4400"""
    t = synth.ranks(951, TINY_N, 4).copy()
    t[4400:4450] = t[3000:3050]
    t.setflags(write=False)
    return t


def tiny_pairs():
    """Eight pairs as interleaved mates of about M letters, one entry at least for every handle of the chain: a split mate (a
    supplementary part), a mate without an intact window (rescued), a mate over the segment that occurs twice (a secondary place), a
    mate with a broken tail (clipped), one with a substitution and a deletion (MD, a site), a pair of random letters (unplaced) and
    two ordinary pairs, one of them from the reverse strand.  The first two pairs are the quarter batch."""
    t, cat = tiny_text(), np.concatenate
    edits = t[3600:3751].copy()
    edits[40] = (edits[40] + 1) % 4
    return [cat([t[500:600], t[2000:2050]]), rc4(t[800:950]),
            t[1000:1150].copy(), kill(rc4(t[1300:1450]), K),
            t[2950:3100].copy(), rc4(t[3250:3400]),
            cat([t[5000:5138], other(t[5138:5150])]), rc4(t[5300:5450]),
            np.delete(edits, 90), rc4(t[3900:4050]),
            synth.ranks(952, M, 4), synth.ranks(953, M, 4),
            t[1600:1750].copy(), rc4(t[1900:2050]),
            rc4(t[5700:5850]), t[5450:5600].copy()]
