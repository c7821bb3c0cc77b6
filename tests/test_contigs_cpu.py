"""The contig table without a GPU: tests/contig_naive.py (the contract of KMX_MAP_CONTIGS in executable form) against the brute-force
definitions of the stages on the contig's letters alone, the midpoint rule, engine.concat_sequences / sam_header / sam_lines with
located_host on hand-made arrays, the ABI of the new calls and their refusals that need no device."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from tests import align_naive as an
from tests import contig_naive as cn
from tests import rescue_naive as rn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LETTERS = "ACGT"


def random_table(rng, lo, hi, nc):
    sizes = rng.integers(lo, hi + 1, nc)
    return np.concatenate([[0], np.cumsum(sizes)]).astype(np.uint64)


def mutate(rng, q, edits, sigma):
    q = list(int(x) for x in q)
    for _ in range(edits):
        k = int(rng.integers(0, 3))
        i = int(rng.integers(0, max(len(q), 1)))
        if k == 0 and q:
            q[i] = (q[i] + 1 + int(rng.integers(0, sigma - 1))) % sigma
        elif k == 1 and len(q) > 1:
            del q[i]
        else:
            q.insert(i, int(rng.integers(0, sigma)))
    return np.asarray(q, np.uint8)


# ---- 1. align against the definition on the contig's letters ---------------------------------------------------------------------------------
def test_align_equals_brute_force_on_the_sub_text_and_differs_from_the_whole_text():
    rng = np.random.default_rng(20260)
    sigma = 4
    n_cases = n_aligned = n_differs = 0
    for case in range(60):
        ctg_off = random_table(rng, 1, 40, int(rng.integers(1, 5)))
        n = int(ctg_off[-1])
        text = rng.integers(0, sigma, n).astype(np.uint8)
        E = int(rng.integers(0, 5))
        reads, diag, span, locus_off = [], [], [], [0]
        for r in range(4):
            m = int(rng.integers(6, 15))
            at = int(rng.integers(-3, n))                      # near and across junctions: the contigs are short
            piece = text[max(at, 0):max(at, 0) + m]
            q = mutate(rng, piece, int(rng.integers(0, 3)), sigma) if piece.size else rng.integers(0, sigma, m).astype(np.uint8)
            reads.append(q)
            for _ in range(2):
                diag.append(min(at + int(rng.integers(-2, 3)), n - 1))     # (the diagonals of a vote lie below n)
                span.append(int(rng.integers(0, 4)))
            locus_off.append(len(diag))
        ranks = np.concatenate(reads)
        roff = np.concatenate([[0], np.cumsum([q.size for q in reads])]).astype(np.uint64)
        got = cn.align(text, ctg_off, ranks, roff, locus_off, diag, span, E, 2, sigma)
        whole = an.align(text, ranks, roff, locus_off, diag, span, E, 2, sigma)
        for r in range(4):
            q = reads[r]
            for l in range(locus_off[r], locus_off[r + 1]):
                if span[l] > 2:
                    assert got[0][l] == an.SKIPPED and got[5][l] == cn.NO_CONTIG
                    continue
                c = cn.contig_of(ctg_off, n, diag[l], span[l], q.size)
                b0, b1 = int(ctg_off[c]), int(ctg_off[c + 1])
                assert got[5][l] == c
                d, s, e = an.brute_one(text[b0:b1], q, diag[l] - b0, span[l], E, sigma)
                lo, hi = cn.window(ctg_off, c, q.size, diag[l], span[l], E)
                assert (lo - b0, hi - b0) == an.window(b1 - b0, q.size, diag[l] - b0, span[l], E)   # the two forms of the window
                n_cases += 1
                if d > E:
                    assert got[0][l] == an.NONE and got[1][l] == 0 and got[2][l] == 0
                    continue
                n_aligned += 1
                assert (int(got[0][l]), int(got[1][l]), int(got[2][l])) == (d, s + b0, e + b0)
                assert b0 <= got[1][l] <= got[2][l] <= b1
                n_differs += (int(whole[0][l]), int(whole[1][l]), int(whole[2][l])) != (d, s + b0, e + b0)
    assert n_cases >= 300 and n_aligned >= 100 and n_differs >= 10, (n_cases, n_aligned, n_differs)


def test_midpoint_ties_for_even_and_odd_sums():
    off = [0, 10, 20, 30]
    # mid = D + (S + m) // 2: an even and an odd S + m on either side of the junction at 10
    assert cn.contig_of(off, 30, 4, 0, 12) == 1 and cn.contig_of(off, 30, 3, 0, 12) == 0        # mid 10, 9
    assert cn.contig_of(off, 30, 4, 0, 13) == 1 and cn.contig_of(off, 30, 3, 0, 13) == 0        # 13 // 2 == 6 (floor)
    assert cn.contig_of(off, 30, 3, 1, 12) == 0 and cn.contig_of(off, 30, 3, 2, 12) == 1        # the span counts
    # the clamp: a diagonal before the text and one that points past it
    assert cn.contig_of(off, 30, -50, 0, 8) == 0 and cn.contig_of(off, 30, 29, 3, 40) == 2 and cn.contig_of(off, 30, 10 ** 12, 0, 1) == 2
    assert cn.contig_of([0, 30], 30, 17, 0, 5) == 0
    # a negative diagonal: the floor is taken of (S + m) / 2 alone, then D is added
    assert cn.contig_of(off, 30, -3, 0, 25) == 0 and cn.contig_of(off, 30, -2, 0, 25) == 1      # mid 9, 10


# ---- 2. the spread rescue against the definition on clamped windows ---------------------------------------------------------------------------
def test_spread_window_equals_brute_force_on_the_clamped_window():
    rng = np.random.default_rng(777)
    sigma = 4
    n_cases = n_found = n_differs = 0
    while n_cases < 300:
        ctg_off = random_table(rng, 1, 120, 3)
        n = int(ctg_off[-1])
        text = rng.integers(0, sigma, n).astype(np.uint8)
        E = int(rng.integers(0, 5))
        max_insert = int(rng.integers(20, 200))
        wide, add = cn.spread(text, ctg_off, max_insert + 1, sigma)
        c = int(rng.integers(0, 3))
        b0, b1 = int(ctg_off[c]), int(ctg_off[c + 1])
        m = int(rng.integers(6, 41))
        # a mate cut near the end of the contig or across the junction, with a few edits
        at = int(rng.integers(max(b0 - 8, 0), b1 + 4))
        piece = text[at:at + m]
        if piece.size < 6:
            continue
        q = mutate(rng, piece, int(rng.integers(0, E + 1)), sigma)
        if not 6 <= q.size <= 40:
            continue
        Sa = int(rng.integers(b0, b1))
        Ea = min(b1, Sa + int(rng.integers(1, 30)))
        for up in (True, False):
            lo, hi = cn.rescue_window(ctg_off, c, up, Sa, Ea, max_insert)
            assert b0 <= lo <= hi <= b1
            want = rn.brute_window(text, q, lo, hi, E, sigma)
            # what rescue_naive sees on the spread text: its plain window, from the shifted anchor
            a = int(add[c])
            wlo, whi = (Sa + a, min(wide.size, Sa + a + max_insert)) if up else (max(0, Ea + a - max_insert), Ea + a)
            d, s, e = rn.align_window(wide, q, wlo, whi, E, sigma)
            got = (d, s - a, e - a) if d <= E else (d, 0, 0)
            assert got == want, (ctg_off, c, up, Sa, Ea, max_insert, E, q)
            plain = rn.align_window(text, q, *((Sa, min(n, Sa + max_insert)) if up else (max(0, Ea - max_insert), Ea)), E, sigma)
            n_cases += 1
            n_found += want[0] <= E
            n_differs += plain != want
    assert n_found >= 40 and n_differs >= 15, (n_cases, n_found, n_differs)


# ---- 3. locate ----------------------------------------------------------------------------------------------------------------------------------
def test_locate_naive_on_hand_made_placements():
    off = [0, 10, 25]
    lctg = [0, 1, 1, cn.NO_CONTIG, 7]
    U, NB = 255, an.NO_BEST
    #                placed c0  unplaced  rescued   its mate   skipped locus  bad contig  locus out  start outside
    locus = np.asarray([0,       NB,       NB,       2,         3,             4,          9,         1], np.uint32)
    strand = np.asarray([0,      U,        1,        0,         0,             0,          1,         0], np.uint8)
    start = np.asarray([10,      0,        12,       25,        1,             1,          1,         9], np.uint32)
    ctg, pos, ok, bad = cn.locate(off, lctg, locus, strand, start, mates=True)
    assert ctg.tolist() == [0, cn.NO_CONTIG, 1, 1] + [cn.NO_CONTIG] * 4 and pos.tolist() == [10, 0, 2, 15, 0, 0, 0, 0]
    assert (ok, bad) == (3, 4)
    ctg, pos, ok, bad = cn.locate(off, lctg, locus, strand, start, mates=False)                  # the rescued read comes without the flag
    assert ctg[2] == cn.NO_CONTIG and (ok, bad) == (2, 5)
    # an empty alignment on a junction belongs to the contig of its locus, on either side
    ctg, pos, _, _ = cn.locate(off, [0, 1], [0, 1], [0, 0], [10, 10])
    assert ctg.tolist() == [0, 1] and pos.tolist() == [10, 0]


# ---- 4. the Python helpers ----------------------------------------------------------------------------------------------------------------------
def test_concat_sequences(engine):
    seqs = [np.asarray([0, 1, 2], np.uint8), [3], np.asarray([2, 2], np.int64)]
    ranks, ctg_off = engine.concat_sequences(seqs)
    assert ranks.dtype == np.uint8 and ranks.tolist() == [0, 1, 2, 3, 2, 2]
    assert ctg_off.dtype == np.uint64 and ctg_off.tolist() == [0, 3, 4, 6]
    r0, o0 = engine.concat_sequences([])
    assert r0.size == 0 and o0.tolist() == [0]
    with pytest.raises(ValueError):
        engine.concat_sequences([[1], []])


def test_sam_header(engine):
    assert engine.sam_header(["chr1", "chrM"], [0, 1000, 1016]) == ["@HD\tVN:1.6\tSO:unsorted", "@SQ\tSN:chr1\tLN:1000", "@SQ\tSN:chrM\tLN:16"]
    assert engine.sam_header([], [0]) == ["@HD\tVN:1.6\tSO:unsorted"]
    with pytest.raises(ValueError):
        engine.sam_header(["a"], [0, 1, 2])


def test_sam_lines_with_contigs_on_hand_made_pairs_of_all_five_classes(engine):
    from kmer_index_amd import synth

    U, NC = 255, engine.NO_CONTIG
    reads = [synth.ranks(300 + i, 6 + i, 4) for i in range(10)]
    ranks, roff = np.concatenate(reads), np.concatenate([[0], np.cumsum([r.size for r in reads])]).astype(np.uint64)
    ctg_off = [0, 400, 1000, 9500]
    names3 = ["cA", "cB", "cC"]
    #                    unplaced  concordant  discordant (split)  mate 1 only  mate 2 only
    strand = np.asarray([U, U,     0, 1,       0, 0,               1, U,        U, 0], np.uint8)
    start = np.asarray([0, 0,      100, 300,   500, 9000,          700, 0,      0, 1000], np.uint32)
    ctg = np.asarray([NC, NC,      0, 0,       1, 2,               1, NC,       NC, 2], np.uint32)
    pos = np.where(strand != U, start - np.asarray(ctg_off)[np.where(ctg == NC, 0, ctg)], 0).astype(np.uint32)
    dist = np.asarray([255, 255,   0, 2,       1, 0,               3, 255,      255, 0], np.uint8)
    placements = (np.zeros(10, np.uint32), strand, dist, start, start + 10, np.full(10, 255, np.uint8))
    cls = np.asarray([engine.PAIR_UNPLACED, engine.PAIR_CONCORDANT, engine.PAIR_DISCORDANT, engine.PAIR_MATE1_ONLY, engine.PAIR_MATE2_ONLY], np.uint8)
    tlen = np.asarray([0, 210, 0, 0, 0], np.int32)
    pairs = (cls, tlen, np.zeros(5, np.uint16), np.zeros(5, np.uint16))
    cigars = ["" if s == U else f"{6 + i}=" for i, s in enumerate(strand)]
    mds = ["" if s == U else str(6 + i) for i, s in enumerate(strand)]
    mapq = np.asarray([0, 0, 60, 60, 10, 10, 30, 0, 0, 30], np.uint8)
    qn = [f"r{i // 2}" for i in range(10)]
    args = (qn, ranks, roff, LETTERS, [3, 2, 1, 0], 4)
    lines = engine.sam_lines(*args, names3, placements, cigars, mds, mapq, pairs, located_host=(ctg, pos))
    old = engine.sam_lines(*args, "chr", placements, cigars, mds, mapq, pairs)
    f = [ln.split("\t") for ln in lines]
    g = [ln.split("\t") for ln in old]
    for i in range(10):
        assert f[i][:2] == g[i][:2] and f[i][4:6] == g[i][4:6] and f[i][8:] == g[i][8:]          # only RNAME POS RNEXT PNEXT change
    assert [x[2:4] + x[6:8] for x in f] == [
        ["*", "0", "*", "0"], ["*", "0", "*", "0"],
        ["cA", "101", "=", "301"], ["cA", "301", "=", "101"],
        ["cB", "101", "cC", "8001"], ["cC", "8001", "cB", "101"],                                 # mates on different contigs
        ["cB", "301", "=", "301"], ["cB", "301", "=", "301"],                                     # the unplaced mate sits with its partner
        ["cC", "1", "=", "1"], ["cC", "1", "=", "1"]]
    # single reads: no mate fields
    single = engine.sam_lines(*args, names3, placements, cigars, mds, mapq, None, located_host=(ctg, pos))
    assert single[5].split("\t")[2:4] == ["cC", "8001"] and single[5].split("\t")[6:8] == ["*", "0"] and single[1].split("\t")[2:4] == ["*", "0"]
    # with None the output is what it was
    assert engine.sam_lines(*args, "chr", placements, cigars, mds, mapq, pairs, located_host=None) == old
    # a placed read without a contig, and a contig without a name
    bad = ctg.copy(); bad[2] = NC
    with pytest.raises(ValueError):
        engine.sam_lines(*args, names3, placements, cigars, mds, mapq, pairs, located_host=(bad, pos))
    with pytest.raises(ValueError):
        engine.sam_lines(*args, names3[:2], placements, cigars, mds, mapq, pairs, located_host=(ctg, pos))


# ---- 5. the ABI ---------------------------------------------------------------------------------------------------------------------------------
def test_struct_size_and_the_capability_macro(engine):
    assert C.sizeof(engine.LocateOptions) == 8 and engine.LOCATE_MATES == 1
    hdr = open(os.path.join(ROOT, "include", "kmx.h")).read()
    assert re.search(r"^#define KMX_MAP_CONTIGS 1$", hdr, re.M) and re.search(r"^#define KMX_VERSION 5$", hdr, re.M)
    assert re.search(r"^#define KMX_LOCATE_MATES 1u", hdr, re.M)
    assert "struct_size;  /* = sizeof(kmx_locate_options): 8 */" in hdr
    for name in ("kmx_index_set_contigs", "kmx_index_contigs", "kmx_alignments_contigs_view", "kmx_alignments_contigs_view_device",
                 "kmx_placements_locate", "kmx_located_counts", "kmx_located_view", "kmx_located_view_device", "kmx_located_free"):
        assert name in engine.EXPORTS and re.search(r"\b" + name + r"\(", hdr) and hasattr(engine.lib(), name)


def test_refusals_that_need_no_device(engine):
    L = engine.lib()
    off = np.asarray([0, 4], np.uint64)
    assert L.kmx_index_set_contigs(None, off.ctypes.data, 1) == 1 and b"kmx_index_set_contigs" in L.kmx_last_error() and b"index is NULL" in L.kmx_last_error()
    assert L.kmx_index_contigs(None, None, None, 0) == 1 and b"kmx_index_contigs" in L.kmx_last_error()
    assert L.kmx_alignments_contigs_view(None, None, None) == 1 and L.kmx_alignments_contigs_view_device(None, None, None) == 1
    out = C.c_void_p()
    opt = lambda **kw: engine.LocateOptions(**dict(dict(struct_size=8, flags=0), **kw))
    one = C.c_void_p(1)                                        # never dereferenced: the refusal comes first
    for ix, al, pl, o, inout, word in ((None, one, one, opt(), out, b"index is NULL"), (one, None, one, opt(), out, b"alignments handle is NULL"),
                                       (one, one, None, opt(), out, b"placements handle is NULL"), (one, one, one, None, out, b"options is NULL"),
                                       (one, one, one, opt(), None, b"inout is NULL"), (one, one, one, opt(struct_size=7), out, b"struct_size"),
                                       (one, one, one, opt(flags=2), out, b"unknown flags"), (one, one, one, opt(flags=3), out, b"unknown flags")):
        st = L.kmx_placements_locate(ix, al, pl, C.byref(o) if o is not None else None, None, C.byref(inout) if inout is not None else None)
        assert st == 1 and word in L.kmx_last_error() and b"kmx_placements_locate" in L.kmx_last_error(), word
        assert not out.value                                   # no handle was made
    assert L.kmx_located_counts(None, None, None, None) == 1 and L.kmx_located_view(None, None, None) == 1 and L.kmx_located_view_device(None, None, None) == 1
    L.kmx_located_free(None)
