"""SAM tags without a GPU: tests/md_naive.py and tests/mapq_naive.py (the contracts of kmx_scripts_md / kmx_rescues_md and
kmx_placements_mapq in executable form) against a second implementation, literal cases and a hand-written table; engine.sam_lines
on hand-made arrays; the ABI of the new calls and their refusals that need no device."""
import ctypes as C
import os
import re

import numpy as np

from kmer_index_amd import synth
from tests import mapq_naive as qn
from tests import md_naive as mn
from tests import script_naive as sn
from tests.chain_data import edited

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LETTERS = "ACGT"
EQ, X, I, D = sn.OP_EQ, sn.OP_X, sn.OP_I, sn.OP_D


def run(n, op):
    return (n << 4) | op


def ranks_of(s):
    return np.asarray([LETTERS.index(c) for c in s], np.uint8)


def one(runs, text, s=0, t=None):
    """the MD string of one entry over text[s:t] through md_naive.md, which must count it as served"""
    text = ranks_of(text) if isinstance(text, str) else text
    t = len(text) if t is None else t
    md_off, md, bad = mn.md([0], [0, len(runs)], np.asarray(runs, np.uint32), [s], [t], text, LETTERS)
    assert bad == 0 and md_off.tolist() == [0, md.size]
    return md.tobytes().decode()


# ---- 1. md_naive against a second implementation ------------------------------------------------------------------------------------------
def by_columns(runs, q, t):
    """The alignment column by column ((read letter or None, text letter or None)), then formatted."""
    cols, i, j = [], 0, 0
    for v in runs:
        for _ in range(int(v) >> 4):
            op = int(v) & 15
            if op == I:
                cols.append((int(q[i]), None))
                i += 1
            elif op == D:
                cols.append((None, int(t[j])))
                j += 1
            else:
                cols.append((int(q[i]), int(t[j])))
                i += 1
                j += 1
    assert i == len(q) and j == len(t)
    out, c, in_del = "", 0, False
    for a, b in cols:
        if b is None:                                          # an insertion: not in the MD, but it ends a deletion
            in_del = False
        elif a is None:
            if not in_del:
                out += f"{c}^"
                c = 0
            out += LETTERS[b]
            in_del = True
        elif a == b:
            c += 1
            in_del = False
        else:
            out += f"{c}{LETTERS[b]}"
            c = 0
            in_del = False
    return out + str(c)


def test_md_naive_equals_the_column_formatter_and_rebuilds_the_text():
    n_pairs = 2000
    text = synth.ranks(4242, 20_000, 4)
    z = synth.u64_stream(4243, 24 * n_pairs).astype(np.int64) & 0x7FFFFFFF
    seen = {"X": 0, "^": 0, "I": 0, "plain": 0}
    sel, cig_off, cigar, start, end = [], [0], [], [], []
    want_strings, seqs = [], []
    for p in range(n_pairs):
        zz = z[24 * p:24 * p + 24]
        s, m, n_edits = int(zz[0] % 19_000), 20 + int(zz[1] % 60), int(zz[2] % 7)
        t = text[s:s + m]
        q = edited(zz[3:], t, n_edits)
        h = sn.full_h(q, t, 4)
        runs = sn.rle(sn.walk(q, t, 4, h))
        assert sn.replay(q, t, runs, 4) == (int(h[len(q)][len(t)]), True)
        want = by_columns(runs, q, t)
        assert mn.GRAMMAR.match(want), want
        assert mn.byte_count(runs) == len(want)
        assert mn.md_one(runs, text, s, LETTERS.encode()).decode() == want
        seq = "".join(LETTERS[int(x)] for x in q)
        assert mn.rebuild(seq, runs, want) == "".join(LETTERS[int(x)] for x in t)
        ops = {int(v) & 15 for v in runs}
        seen["X"] += X in ops
        seen["^"] += D in ops
        seen["I"] += I in ops
        seen["plain"] += ops == {EQ}
        sel.append(p)
        cigar += runs
        cig_off.append(len(cigar))
        start.append(s)
        end.append(s + m)
        want_strings.append(want)
        seqs.append(seq)
    assert min(seen.values()) >= 100, seen
    # the batch form: offsets, bytes and the counter
    md_off, md, bad = mn.md(sel, cig_off, np.asarray(cigar, np.uint32), start, end, text, LETTERS)
    assert bad == 0 and mn.strings(md_off, md) == want_strings and md_off.dtype == np.uint64 and md.dtype == np.uint8
    assert md_off[-1] == md.size == sum(len(w) for w in want_strings)


# ---- 2. literal cases ---------------------------------------------------------------------------------------------------------------------
def test_literal_md_strings():
    t = "ACGTACGTAC"
    assert one([run(1, X), run(9, EQ)], t) == "0A9"                                   # X at the first letter
    assert one([run(9, EQ), run(1, X)], t) == "9C0"                                   # ... and at the last
    assert one([run(3, EQ), run(2, X), run(5, EQ)], t) == "3T0A5"                     # two adjacent X
    assert one([run(2, EQ), run(2, D), run(1, X), run(2, EQ)], "GGACTGG") == "2^AC0T2"  # D followed directly by X
    assert one([run(1, X), run(2, D), run(7, EQ)], t) == "0A0^CG7"                    # X followed directly by D
    assert one([run(4, EQ), run(2, I), run(6, EQ)], t) == "10"                        # I between matches: the counts add up
    assert one([run(2, I), run(10, EQ), run(3, I)], t) == "10"
    assert one([run(10, D)], t) == "0^ACGTACGTAC0"
    assert one([run(10, X)], t) == "0A0C0G0T0A0C0G0T0A0C0"
    assert one([run(3, I)], t, 4, 4) == "0"                                           # the empty substring
    assert one([run(3, EQ), run(1, D), run(2, EQ)], t, 2, 8) == "3^C2"                # a substring inside the text
    long_text = np.tile(ranks_of("ACGT"), 600)
    for n in (9, 10, 99, 100, 999, 1000, 1024):
        assert one([run(n, EQ)], long_text, 0, n) == str(n) and mn.byte_count([run(n, EQ)]) == len(str(n))
        got = one([run(n, EQ), run(1, X), run(n, EQ)], long_text, 3, 3 + 2 * n + 1)
        assert got == f"{n}{LETTERS[(3 + n) % 4]}{n}" and mn.byte_count([run(n, EQ), run(1, X), run(n, EQ)]) == len(got)
        assert mn.GRAMMAR.match(got)


def test_entries_without_runs_and_every_mismatched_clause():
    text = ranks_of("ACGTACGTAC")
    good = [run(4, EQ), run(1, X), run(5, EQ)]
    cigar = np.asarray(good * 7 + [run(10, sn.OP_M)] + [run(4, EQ), run(1, I), run(5, EQ)], np.uint32)
    #        served  no runs  l out of bound  s > t  t > n  sum != t - s  served  op M   sum (I does not count)
    sel = [0,       0,       5,              1,     2,     3,            4,      0,     0]
    cig_off = [0, 3, 3, 6, 9, 12, 15, 18, 19, 22]
    start = [0, 6, 5, 0, 0]
    end = [10, 5, 15, 9, 10]
    md_off, md, bad = mn.md(sel, cig_off, cigar, start, end, text, LETTERS)
    assert mn.strings(md_off, md) == ["4A5", "", "", "", "", "", "4A5", "", ""] and bad == 6
    # the bound on sel may be tighter than the arrays
    assert mn.md(sel, cig_off, cigar, start, end, text, LETTERS, bound=4)[2] == 7
    # no entries at all
    md_off, md, bad = mn.md([], [0], np.zeros(0, np.uint32), [], [], text, LETTERS)
    assert md_off.tolist() == [0] and md.size == 0 and bad == 0
    # a table with duplicates is allowed
    assert mn.strings(*mn.md([0], [0, 3], cigar[:3], [0], [10], text, "NNNN")[:2]) == ["4N5"]


def test_rebuild_refuses_what_does_not_fit():
    import pytest

    runs = [run(4, EQ), run(1, X), run(5, EQ)]
    assert mn.rebuild("ACGTCCGTAC", runs, "4A5") == "ACGTACGTAC"
    for seq, md in (("ACGTCCGTAC", "10"), ("ACGTCCGTAC", "4A4"), ("ACGTCCGTA", "4A5"), ("ACGTCCGTAC", "4^A5")):
        with pytest.raises(ValueError):
            mn.rebuild(seq, runs, md)


# ---- 3. mapq_naive against a hand-written table -------------------------------------------------------------------------------------------
def test_mapq_naive_against_a_hand_written_table():
    E, U, N8, N16, CC, DC = 8, 255, 255, 0xFFFF, 1, 2
    #            unplaced  unique d=0  unique d=E  second==dist  second<dist  d > E   d=5, s=7
    strand = [U,        0,          1,          0,            1,           0,      0]
    dist = [255,      0,          8,          2,            3,           10,     5]
    second = [N8,       N8,         N8,         2,            1,           N8,     7]
    got, c = qn.mapq(strand, dist, second, E)
    assert got.tolist() == [0, 60, 10, 0, 0, 0, 20] and got.dtype == np.uint8 and c == dict(nr=7, n_zero=3, n_cap=1)
    # pairs: 0 concordant without a runner-up; 1 concordant with one; 2 the repeat mate and its unique partner; 3 discordant; 4 unplaced
    strand = [0, 1,   0, 1,   0, 1,    0, 0,    U, U]
    dist = [6, 7,   1, 1,   0, 0,    0, 0,    255, 255]
    second = [N8, N8, N8, 1,  0, N8,   0, N8,   N8, N8]
    cls = [CC, CC, CC, DC, 0]
    score = [13, 2, 0, 0, N16]
    second_score = [N16, 4, N16, N16, N16]
    pairs = dict(cls=cls, score=score, second_score=second_score)
    got, c = qn.mapq(strand, dist, second, E, **pairs)
    #                   max(30, min(40, 70)), max(20, min(40, 60));  60 stays, 0 -> min(20, 40);  0 -> min(60, 40), 60;  single rule;  0
    assert got.tolist() == [40, 40, 60, 20, 40, 60, 0, 60, 0, 0] and c == dict(nr=10, n_zero=1, n_cap=3)
    assert qn.mapq(strand, dist, second, E)[0].tolist() == [30, 20, 60, 0, 0, 60, 0, 60, 0, 0]          # the same reads without pairs
    # the repeat mate gets min(cap, pair_bonus)
    assert qn.mapq(strand, dist, second, E, cap=30, **pairs)[0].tolist()[4:6] == [30, 30]
    assert qn.mapq(strand, dist, second, E, pair_bonus=0, **pairs)[0].tolist() == [30, 20, 60, 0, 0, 60, 0, 60, 0, 0]
    assert qn.mapq(strand, dist, second, E, pair_bonus=0xFFFFFFFF, **pairs)[0].tolist() == [40, 40, 60, 20, 60, 60, 0, 60, 0, 0]
    # cap 0: everything is 0 and at the cap; cap 254; per_edit 0
    got, c = qn.mapq(strand, dist, second, E, cap=0, **pairs)
    assert not got.any() and c == dict(nr=10, n_zero=8, n_cap=10)
    got, c = qn.mapq(strand, dist, second, E, cap=254, per_edit=100, pair_bonus=1000, **pairs)
    assert got.tolist() == [254, 254, 254, 200, 254, 254, 0, 254, 0, 0] and c["n_cap"] == 6
    got, c = qn.mapq(strand, dist, second, E, per_edit=0, **pairs)
    assert not got.any() and c == dict(nr=10, n_zero=8, n_cap=0)
    got, c = qn.mapq([], [], [], E)
    assert got.size == 0 and c == dict(nr=0, n_zero=0, n_cap=0)
    assert qn.DEFAULTS == dict(cap=60, per_edit=10, pair_bonus=40)


# ---- 4. sam_lines -------------------------------------------------------------------------------------------------------------------------
def rc_string(s):
    return s[::-1].translate(str.maketrans("ACGT", "TGCA"))


def test_sam_lines_on_hand_made_pairs_of_all_five_classes():
    from kmer_index_amd import engine

    U = 255
    reads = [synth.ranks(900 + i, 6 + i, 4) for i in range(10)]
    ranks, roff = np.concatenate(reads), np.concatenate([[0], np.cumsum([r.size for r in reads])]).astype(np.uint64)
    #         unplaced  concordant  discordant  mate 1 only  mate 2 only
    strand = np.asarray([U, U,   0, 1,       0, 0,       1, U,        U, 0], np.uint8)
    start = np.asarray([0, 0,   100, 300,   500, 9000,  700, 0,      0, 800], np.uint32)
    dist = np.asarray([255, 255, 0, 2,      1, 0,       3, 255,      255, 0], np.uint8)
    end = start + 10
    placements = (np.zeros(10, np.uint32), strand, dist, start, end, np.full(10, 255, np.uint8))
    cls = np.asarray([engine.PAIR_UNPLACED, engine.PAIR_CONCORDANT, engine.PAIR_DISCORDANT, engine.PAIR_MATE1_ONLY, engine.PAIR_MATE2_ONLY], np.uint8)
    tlen = np.asarray([0, 210, 0, 0, 0], np.int32)
    pairs = (cls, tlen, np.zeros(5, np.uint16), np.zeros(5, np.uint16))
    cigars = ["" if s == U else f"{6 + i}=" for i, s in enumerate(strand)]
    mds = ["" if s == U else str(6 + i) for i, s in enumerate(strand)]
    mapq = np.asarray([0, 0, 60, 60, 10, 10, 30, 0, 0, 30], np.uint8)
    names = [f"r{i // 2}" for i in range(10)]
    lines = engine.sam_lines(names, ranks, roff, LETTERS, [3, 2, 1, 0], 4, "chr", placements, cigars, mds, mapq, pairs)
    flag, pos, pnext, tl = engine.sam_pair_fields(strand, start, cls, tlen)
    assert len(lines) == 10
    for i, line in enumerate(lines):
        f = line.split("\t")
        placed = strand[i] != U
        assert len(f) == (13 if placed else 11) and "\n" not in line
        seq = "".join(LETTERS[int(x)] for x in reads[i])
        assert f[0] == names[i] and int(f[1]) == flag[i] and int(f[3]) == pos[i] and int(f[4]) == mapq[i]
        assert int(f[7]) == pnext[i] and int(f[8]) == tl[i] and f[10] == "*"
        assert f[9] == (rc_string(seq) if placed and strand[i] == 1 else seq)
        assert f[5] == (cigars[i] if placed else "*")
        assert bool(int(f[1]) & 0x4) == (not placed) and bool(int(f[1]) & 0x10) == (placed and strand[i] == 1)
        assert bool(int(f[1]) & 0x40) == (i % 2 == 0) and bool(int(f[1]) & 0x80) == (i % 2 == 1) and int(f[1]) & 0x1
        assert bool(int(f[1]) & 0x8) == (strand[i ^ 1] == U) and bool(int(f[1]) & 0x2) == (cls[i // 2] == engine.PAIR_CONCORDANT)
        if placed:
            assert f[11] == f"NM:i:{dist[i]}" and f[12] == f"MD:Z:{mds[i]}"
    # an unplaced pair has no reference at all; an unplaced read with a placed mate sits at its mate's position
    assert lines[0].split("\t")[2:9] == ["*", "0", "0", "*", "*", "0", "0"]
    assert lines[7].split("\t")[2:8] == ["chr", "701", "0", "*", "=", "701"] and lines[6].split("\t")[6:8] == ["=", "701"]
    assert lines[2].split("\t")[6:9] == ["=", "301", "210"] and lines[3].split("\t")[6:9] == ["=", "101", "-210"]
    # the rescue's strings take the place of the placements' where the placements have none
    two = engine.sam_lines(names, ranks, roff, LETTERS, [3, 2, 1, 0], 4, "chr", placements, (["" if i == 2 else c for i, c in enumerate(cigars)],
                           ["7M" if i == 2 else "" for i in range(10)]), (mds, [""] * 10), mapq, pairs)
    assert two[2].split("\t")[5] == "7M" and [x for i, x in enumerate(two) if i != 2] == [x for i, x in enumerate(lines) if i != 2]


def test_sam_lines_on_hand_made_single_reads():
    from kmer_index_amd import engine

    reads = [ranks_of("ACGTTG"), ranks_of("GGGACA"), ranks_of("TTTT"), np.zeros(0, np.uint8)]
    ranks, roff = np.concatenate(reads), np.asarray([0, 6, 12, 16, 16], np.uint64)
    strand = np.asarray([0, 1, 255, 255], np.uint8)
    start = np.asarray([41, 7, 0, 0], np.uint32)
    placements = (np.zeros(4, np.uint32), strand, np.asarray([1, 0, 255, 255], np.uint8), start, start + 6, np.full(4, 255, np.uint8))
    lines = engine.sam_lines(["a", "b", "c", "d"], ranks, roff, b"ACGT", np.asarray([3, 2, 1, 0], np.uint8), 4, "ref", placements,
                             ["3=1X2=", "6=", "", ""], ["3A2", "6", "", ""], [10, 60, 0, 0])
    assert lines[0] == "a\t0\tref\t42\t10\t3=1X2=\t*\t0\t0\tACGTTG\t*\tNM:i:1\tMD:Z:3A2"
    assert lines[1] == "b\t16\tref\t8\t60\t6=\t*\t0\t0\tTGTCCC\t*\tNM:i:0\tMD:Z:6"
    assert lines[2] == "c\t4\t*\t0\t0\t*\t*\t0\t0\tTTTT\t*" and lines[3] == "d\t4\t*\t0\t0\t*\t*\t0\t0\t*\t*"


# ---- 5. the ABI ---------------------------------------------------------------------------------------------------------------------------
def test_struct_sizes_and_the_capability_macro(engine):
    assert C.sizeof(engine.MdOptions) == 8 and C.sizeof(engine.MapqOptions) == 24
    hdr = open(os.path.join(ROOT, "include", "kmx.h")).read()
    assert re.search(r"^#define KMX_SAM_TAGS 1$", hdr, re.M) and re.search(r"^#define KMX_VERSION 5$", hdr, re.M)
    assert "struct_size;  /* = sizeof(kmx_md_options): 8 */" in hdr and "struct_size;  /* = sizeof(kmx_mapq_options): 24 */" in hdr
    assert engine.SamTags._fields == ("mapq", "md", "rescue_scripts", "rescue_md")


def test_refusals_that_need_no_device(engine):
    L = engine.lib()
    out = C.c_void_p()
    table = np.frombuffer(b"ACGT", np.uint8).copy()
    md_opt = lambda **kw: engine.MdOptions(**dict(dict(struct_size=8, flags=0), **kw))
    for fn in (L.kmx_scripts_md, L.kmx_rescues_md):
        name = b"kmx_scripts_md" if fn is L.kmx_scripts_md else b"kmx_rescues_md"
        for o, letters, inout, word in ((None, table, out, b"options is NULL"), (md_opt(), table, None, b"inout is NULL"),
                                        (md_opt(struct_size=7), table, out, b"struct_size"), (md_opt(flags=1), table, out, b"flags"),
                                        (md_opt(), None, out, b"letters"), (md_opt(), table, out, b"index is NULL")):
            st = fn(None, None, None, letters.ctypes.data if letters is not None else None, C.byref(o) if o is not None else None, None,
                    C.byref(inout) if inout is not None else None)
            assert st == 1 and word in L.kmx_last_error() and name in L.kmx_last_error(), word
            assert not out.value                               # no handle was made
    assert L.kmx_md_counts(None, None, None, None) == 1 and L.kmx_md_view(None, None, None) == 1 and L.kmx_md_view_device(None, None, None) == 1
    L.kmx_md_free(None)
    mq_opt = lambda **kw: engine.MapqOptions(**dict(dict(struct_size=24, max_edits=8, cap=60, per_edit=10, pair_bonus=40, flags=0), **kw))
    for o, inout, word in ((None, out, b"options is NULL"), (mq_opt(), None, b"inout is NULL"), (mq_opt(struct_size=23), out, b"struct_size"),
                           (mq_opt(flags=1), out, b"flags"), (mq_opt(max_edits=251), out, b"max_edits"), (mq_opt(cap=255), out, b"cap > 254"),
                           (mq_opt(max_edits=250, cap=254, per_edit=0xFFFFFFFF, pair_bonus=0xFFFFFFFF), out, b"placements handle is NULL")):
        st = L.kmx_placements_mapq(None, None, C.byref(o) if o is not None else None, None, C.byref(inout) if inout is not None else None)
        assert st == 1 and word in L.kmx_last_error() and b"kmx_placements_mapq" in L.kmx_last_error(), word
        assert not out.value
    assert L.kmx_mapq_counts(None, None, None, None) == 1 and L.kmx_mapq_view(None, None) == 1 and L.kmx_mapq_view_device(None, None) == 1
    L.kmx_mapq_free(None)
