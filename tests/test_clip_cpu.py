"""Soft clipping without a GPU: tests/clip_naive.py (the contract of kmx_scripts_clip, kmx_clips_md and kmx_clips_rescues_md in
executable form) against a brute force over column intervals, the worked examples of the contract, its consequences on canonical
scripts, the MD of clipped entries, engine.sam_lines(clip_fields=) and engine.xa_strings(shift=) on hand-made arrays, and the ABI of
the new calls with the refusals that need no device."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from kmer_index_amd import synth
from tests import clip_naive as cn
from tests import md_naive as mn
from tests import script_naive as sn
from tests.chain_data import edited

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LETTERS = "ACGT"
EQ, X, I, D, S = cn.OP_EQ, cn.OP_X, cn.OP_I, cn.OP_D, cn.OP_S
NEW = ["kmx_scripts_clip", "kmx_clips_counts", "kmx_clips_view", "kmx_clips_view_device", "kmx_clips_md", "kmx_clips_rescues_md", "kmx_clips_free"]
NO_FLOOR = -10 ** 12                                           # a min_score nothing falls below


# ---- 1. clip_naive against a brute force over column intervals ---------------------------------------------------------------------------
def random_script(z):
    """A valid script from the numbers z: R <= 9 runs of 1 .. 6 letters, neighbours of different ops, no D at either end."""
    R = 1 + int(z[0] % 9)
    ops, runs = [], []
    for k in range(R):
        allowed = [op for op in (EQ, EQ, X, I, D) if (not ops or op != ops[-1]) and not (op == D and k in (0, R - 1))]
        ops.append(allowed[int(z[1 + 2 * k] % len(allowed))])
        runs.append(((1 + int(z[2 + 2 * k] % 6)) << 4) | ops[-1])
    return runs


def random_options(z):
    pick = lambda v, choices: choices[int(v % len(choices))]
    return dict(match=pick(z[0], (1, 1, 2, 3)), mismatch=pick(z[1], (0, 1, 2, 4, 4, 6)), gap_open=pick(z[2], (0, 2, 6, 6)),
                gap_extend=pick(z[3], (0, 1, 1, 2)), clip_penalty=pick(z[4], (0, 0, 1, 2, 5, 5)), min_score=NO_FLOOR)


def brute(runs, match, mismatch, gap_open, gap_extend, clip_penalty, **_):
    """Every column interval [c0, c1), c0 < c1, whose sides are unclipped or border a match column, scored from scratch:
    (the greatest value, the maximal intervals)."""
    cols = [int(v) & 15 for v in runs for _ in range(int(v) >> 4)]
    n = len(cols)
    best, at = None, []
    for c0 in range(n):
        if c0 and cols[c0] != EQ:
            continue
        for c1 in range(c0 + 1, n + 1):
            if c1 < n and cols[c1 - 1] != EQ:
                continue
            v = -clip_penalty * (c0 > 0) - clip_penalty * (c1 < n)
            for c in range(c0, c1):
                if cols[c] == EQ:
                    v += match
                elif cols[c] == X:
                    v -= mismatch
                else:
                    v -= gap_extend + (gap_open if c == c0 or cols[c - 1] != cols[c] else 0)
            if best is None or v > best:
                best, at = v, []
            if v == best:
                at.append((c0, c1))
    return best, at


def test_clip_naive_against_every_column_interval():
    n_scripts = 2400
    z = synth.u64_stream(7100, 32 * n_scripts).astype(np.int64) & 0x7FFFFFFF
    seen = dict(clipped=0, whole=0, tie=0, b0=0, x0=0, o0=0, p0=0)
    for k in range(n_scripts):
        zz = z[32 * k:32 * k + 32]
        runs, opt = random_script(zz), random_options(zz[24:])
        i, j, v, low = cn.choose(runs, **opt)
        best, at = brute(runs, **opt)
        assert not low and v == best, (runs, opt)
        # among the maximal intervals: the smallest left side, then the longest
        c0 = min(a for a, _ in at)
        c1 = max(b for a, b in at if a == c0)
        col = np.concatenate([[0], np.cumsum([int(r) >> 4 for r in runs])])
        assert (int(col[i]), int(col[j])) == (c0, c1), (runs, opt, at)
        whole = (i, j) == (0, len(runs))
        seen["clipped"] += not whole
        seen["whole"] += whole
        seen["tie"] += len(at) > 1
        for name, key in (("b0", "mismatch"), ("x0", "gap_extend"), ("o0", "gap_open"), ("p0", "clip_penalty")):
            seen[name] += opt[key] == 0
        # one above the value: the entry stays whole and is LOW, with the score of the whole script
        out = cn.clip_one(runs, **dict(opt, min_score=v + 1))
        assert out[0] == runs and out[2:] == (0, 0, 0, 0, sum(int(r) >> 4 for r in runs if (int(r) & 15) != EQ), cn.LOW)
        assert out[1] == cn.choose(runs, **dict(opt, clip_penalty=10 ** 9))[2]
    assert seen["clipped"] >= n_scripts // 4 and seen["whole"] >= n_scripts // 8 and seen["tie"] >= n_scripts // 10, seen
    assert min(seen[name] for name in ("b0", "x0", "o0", "p0")) >= 100, seen


# ---- 2. the worked examples ---------------------------------------------------------------------------------------------------------------
def one(cigar, **options):
    runs, score, sl, sr, tl, tr, nm, flags = cn.clip_one(cn.parse(cigar), **dict(cn.DEFAULTS, **options))
    return cn.strings([0, len(runs)], runs)[0], score, (sl, sr, tl, tr, nm), flags


def test_the_worked_examples_of_the_contract():
    assert cn.DEFAULTS == dict(match=1, mismatch=4, gap_open=6, gap_extend=1, clip_penalty=5, min_score=0)
    assert one("1X149=") == ("1X149=", 145, (0, 0, 0, 0, 1), 0)                       # a clip costs more than the mismatch
    assert one("1X149=", clip_penalty=0) == ("1S149=", 149, (1, 0, 1, 0, 0), 0)
    assert one("140=10I") == ("140=10S", 135, (0, 10, 0, 0, 0), 0)                    # an overhang: no text letter is clipped
    assert one("138=3X1=5X1=2X") == ("138=12S", 133, (0, 12, 0, 12, 0), 0)            # an adapter tail
    assert one("5=10X3=", clip_penalty=0) == ("5=13S", 5, (0, 13, 0, 13, 0), 0)
    assert one("2=1X2=", clip_penalty=0) == ("2=3S", 2, (0, 3, 0, 3, 0), 0)           # a tie: the smallest i
    assert one("4I") == ("4I", -10, (0, 0, 0, 0, 4), cn.LOW)
    # both ends at once, with a deletion inside
    assert one("10I3=1X100=2D40=2X1=8I") == ("14S100=2D40=11S", 140 - 8 - 10, (14, 11, 4, 3, 2), 0)
    assert one("") == ("", 0, (0, 0, 0, 0, 0), 0) and one("", min_score=1) == ("", 0, (0, 0, 0, 0, 0), cn.LOW)
    assert one("3D5=", clip_penalty=0) == ("5=", 5, (0, 0, 3, 0, 0), 0)               # (no script of the chain begins with D)
    # a foreign op: copied, score 0, LOW
    runs = [(5 << 4) | EQ, (3 << 4) | 0, (5 << 4) | EQ]
    assert cn.clip_one(runs, **cn.DEFAULTS) == (runs, 0, 0, 0, 0, 0, 0, cn.LOW)
    # the batch form: dtypes, offsets and the two counters
    cigs = ["1X149=", "140=10I", "4I", "", "10I3=1X100=2D40=2X1=8I"]
    cigar, off = [], [0]
    for c in cigs:
        cigar += cn.parse(c)
        off.append(len(cigar))
    out = cn.clip(off, np.asarray(cigar, np.uint32), **cn.DEFAULTS)
    assert [a.dtype for a in out[:9]] == [np.int32] + [np.uint16] * 5 + [np.uint8, np.uint64, np.uint32]
    assert cn.strings(out[7], out[8]) == ["1X149=", "140=10S", "4I", "", "14S100=2D40=11S"] and out[9:] == (2, 1)
    assert out[0].tolist() == [145, 135, -10, 0, 122] and out[7].tolist() == [0, 2, 4, 5, 5, 10]


# ---- 3. the consequences, on canonical scripts -------------------------------------------------------------------------------------------
def canonical_cases(n_pairs, seed):
    """(q, text, s, t, runs) of reads cut from a text, edited, some with a random tail, a random head or an overhang at the text's end"""
    text = synth.ranks(seed, 6000, 4)
    z = synth.u64_stream(seed + 1, 40 * n_pairs).astype(np.int64) & 0x7FFFFFFF
    for p in range(n_pairs):
        zz = z[40 * p:40 * p + 40]
        m, kind = 30 + int(zz[1] % 50), int(zz[2] % 6)
        s = int(zz[0] % (text.size - m))
        if kind == 4:
            s = text.size - m                                  # the read runs past the end of the text
        t = text[s:s + m]
        q = edited(zz[4:], t, int(zz[3] % 4))
        junk = (zz[16:16 + 4 + int(zz[15] % 9)] % 4).astype(np.uint8)
        if kind in (1, 3, 4):
            q = np.concatenate([q, junk])
        if kind in (2, 3):
            q = np.concatenate([junk[::-1], q])
        if kind == 5:
            q = np.full(m, 7, np.uint8)                        # letters outside the alphabet
        e = s + m
        while True:                                            # the chain's intervals are tight: no D at either end of a script
            runs = sn.rle(sn.walk(q, text[s:e], 4, sn.full_h(q, text[s:e], 4)))
            head, tail = ((v >> 4) if (v & 15) == D else 0 for v in (runs[0], runs[-1]))
            if not head and not tail:
                break
            s, e = s + head, e - tail
        yield q, text, s, e, runs


def test_the_consequences_of_the_contract_on_canonical_scripts():
    seen = dict(clipped=0, left=0, right=0, both=0, whole=0, no_eq=0, del_kept=0)
    for n, (q, text, s, t, runs) in enumerate(canonical_cases(2000, 7200)):
        opt = dict(cn.DEFAULTS, clip_penalty=(5, 0, 2)[n % 3], min_score=NO_FLOOR if n % 5 else 30)
        out, score, sl, sr, tl, tr, nm, flags = cn.clip_one(runs, **opt)
        ops = [v & 15 for v in out]
        kept = [v for v in out if (v & 15) != S]
        assert (out[0] & 15) != D and (out[-1] & 15) != D      # as the script, the clipped script never begins or ends with D
        assert S not in ops[1:-1] and len(out) <= len(runs) + 2
        assert (ops[0] == S) == (sl > 0) and (ops[-1] == S) == (sr > 0)
        if sl:
            assert out[0] >> 4 == sl and ops[1] == EQ
        if sr:
            assert out[-1] >> 4 == sr and ops[-2] == EQ
        assert kept and (kept[0] & 15) != D and (kept[-1] & 15) != D
        assert sl + sr + cn.letters_of(kept, (EQ, X, I)) == len(q)
        assert tl + tr + cn.letters_of(kept, (EQ, X, D)) == t - s
        # the kept runs are a true script of the clipped read against the clipped text interval, with nm edits
        assert sn.replay(q[sl:len(q) - sr], text[s + tl:t - tr], kept, 4) == (nm, True)
        assert score == sum(cn.weight(v, 1, 4, 6, 1) for v in kept) - opt["clip_penalty"] * ((sl > 0) + (sr > 0))
        if EQ not in [v & 15 for v in runs]:
            assert out == runs and sl + sr == 0
            seen["no_eq"] += 1
        if flags & cn.LOW:
            assert out == runs and score < opt["min_score"]
        else:
            assert score >= opt["min_score"] and score >= sum(cn.weight(v, 1, 4, 6, 1) for v in runs)
        seen["clipped"] += sl + sr > 0
        seen["left"] += sl > 0 and sr == 0
        seen["right"] += sr > 0 and sl == 0
        seen["both"] += sl > 0 and sr > 0
        seen["whole"] += sl + sr == 0
        seen["del_kept"] += sl + sr > 0 and D in ops
    assert seen["clipped"] >= 600 and seen["whole"] >= 300 and min(seen[k] for k in ("left", "right", "both", "no_eq", "del_kept")) >= 50, seen


# ---- 4. the MD of clipped entries -----------------------------------------------------------------------------------------------------------
def test_md_of_clipped_entries_is_md_naive_on_the_clipped_interval():
    sel, cig_off, cigar, start, end, want, seqs = [], [0], [], [], [], [], []
    text = None
    for q, text, s, t, runs in canonical_cases(600, 7300):
        sel.append(len(start))
        start.append(s)
        end.append(t)
        cigar += runs
        cig_off.append(len(cigar))
        seqs.append(q)
    out = cn.clip(cig_off, np.asarray(cigar, np.uint32), **cn.DEFAULTS)
    score, sl, sr, tl, tr, nm, flags, c_off, c_cigar = out[:9]
    md_off, md, bad = cn.md(sel, c_off, c_cigar, tl, tr, start, end, text, LETTERS)
    got = mn.strings(md_off, md)
    assert bad == 0 and md_off.dtype == np.uint64 and md.dtype == np.uint8
    n_changed = 0
    plain = mn.strings(*mn.md(sel, cig_off, np.asarray(cigar, np.uint32), start, end, text, LETTERS)[:2])
    for e in range(len(sel)):
        kept = [int(v) for v in c_cigar[int(c_off[e]):int(c_off[e + 1])] if (int(v) & 15) != S]
        assert got[e] == mn.md_one(kept, text, start[e] + int(tl[e]), LETTERS.encode()).decode() and mn.GRAMMAR.match(got[e])
        q = seqs[e][int(sl[e]):len(seqs[e]) - int(sr[e])]
        if (q < 4).all():
            seq = "".join(LETTERS[int(x)] for x in q)
            assert mn.rebuild(seq, kept, got[e]) == "".join(LETTERS[int(x)] for x in text[start[e] + int(tl[e]):end[e] - int(tr[e])])
        n_changed += got[e] != plain[e]
    assert n_changed >= 100
    # the mismatched clauses: tl + tr beyond the interval, sel out of bound, an op that is neither = X I D nor S
    runs = np.asarray(cn.parse("2S4=1X5=3S"), np.uint32)
    args = lambda tl, tr, s, t, **kw: cn.md([0], [0, len(runs)], runs, [tl], [tr], [s], [t], text, LETTERS, **kw)
    assert mn.strings(*args(2, 3, 100, 115)[:2]) == [f"4{LETTERS[int(text[106])]}5"] and args(2, 3, 100, 115)[2] == 0
    assert args(2, 3, 100, 114)[2] == 1 and args(9, 9, 100, 115)[2] == 1 and args(2, 3, 100, 115, bound=0)[2] == 1
    assert cn.md([0], [0, 1], np.asarray([(10 << 4) | 0], np.uint32), [0], [0], [100], [110], text, LETTERS)[2] == 1


# ---- 5. sam_lines and XA ------------------------------------------------------------------------------------------------------------------------
def test_sam_lines_with_clip_fields(engine):
    U = 255
    reads = [synth.ranks(800 + i, 20, 4) for i in range(6)]
    ranks, roff = np.concatenate(reads), (np.arange(7) * 20).astype(np.uint64)
    #                    pair 0: both placed        pair 1: mate 2 rescued      pair 2: mate 2 unplaced
    strand = np.asarray([0, 1,                      0, 1,                       1, U], np.uint8)
    start = np.asarray([100, 300,                   1000, 1200,                 2000, 0], np.uint32)
    dist = np.asarray([3, 0, 1, 9, 2, 255], np.uint8)
    placements = (np.zeros(6, np.uint32), strand, dist, start, start + 20, np.full(6, 255, np.uint8))
    pairs = (np.asarray([1, 1, 3], np.uint8), np.asarray([220, 220, 0], np.int32), np.zeros(3, np.uint16), np.zeros(3, np.uint16))
    cigars = (["3S17=", "20=", "19=1X", "", "18=2S", ""], ["", "", "", "5S15=", "", ""])
    mds = (["17", "20", "19A", "", "18", ""], ["", "", "", "15", "", ""])
    mapq = np.asarray([60, 60, 40, 40, 10, 0], np.uint8)
    names = [f"r{i // 2}" for i in range(6)]
    args = (names, ranks, roff, LETTERS, [3, 2, 1, 0], 4, "chr", placements, cigars, mds, mapq, pairs)
    old = engine.sam_lines(*args)
    assert engine.sam_lines(*args, clip_fields=None) == old
    z = np.zeros(6, np.int64)
    own = (np.asarray([3, 0, 0, 0, 0, 0]), np.asarray([0, 0, 1, 0, 0, 0]), np.asarray([12, 20, 15, 0, 13, 0]), np.asarray([1, 1, 1, 0, 1, 0], bool))
    res = (np.asarray([0, 0, 0, 5, 0, 0]), z, np.asarray([0, 0, 0, 10, 0, 0]), np.asarray([0, 0, 0, 1, 0, 0], bool))
    new = engine.sam_lines(*args, clip_fields=(own, res))
    f = [line.split("\t") for line in new]
    g = [line.split("\t") for line in old]
    # POS = start + tl + 1, the mate's PNEXT follows, TLEN stays the fold's
    assert [x[3] for x in f] == ["104", "301", "1001", "1206", "2001", "2001"] and [x[3] for x in g] == ["101", "301", "1001", "1201", "2001", "2001"]
    assert [x[7] for x in f] == ["301", "104", "1206", "1001", "2001", "2001"]
    assert [x[8] for x in f] == [x[8] for x in g] == ["220", "-220", "220", "-220", "0", "0"]
    # NM is the clipped one, AS:i: follows MD:Z:, an unplaced read has neither
    assert [x[11:] for x in f[:5]] == [["NM:i:0", "MD:Z:17", "AS:i:12"], ["NM:i:0", "MD:Z:20", "AS:i:20"], ["NM:i:1", "MD:Z:19A", "AS:i:15"],
                                       ["NM:i:0", "MD:Z:15", "AS:i:10"], ["NM:i:0", "MD:Z:18", "AS:i:13"]]
    assert len(f[5]) == 11 and new[5] == old[5]
    for a, b in zip(f, g):                                     # nothing else moves
        assert a[:3] + a[4:7] + a[8:11] == b[:3] + b[4:7] + b[8:11]
    # XA behind AS, and single reads with one group
    with_xa = engine.sam_lines(*args, xa=["chr,+5,20=,0;"] + [""] * 5, clip_fields=(own, res))
    assert with_xa[0] == new[0] + "\tXA:Z:chr,+5,20=,0;" and with_xa[1:] == new[1:]
    single = engine.sam_lines(names, ranks, roff, LETTERS, [3, 2, 1, 0], 4, "chr", placements, cigars[0], mds[0], mapq, clip_fields=own)
    assert single[0].split("\t")[3] == "104" and single[0].endswith("MD:Z:17\tAS:i:12") and single[3].endswith("NM:i:9\tMD:Z:")
    # contig coordinates: the local POS moves by tl as well
    located = (np.asarray([0, 0, 1, 1, 2, engine.NO_CONTIG], np.uint32), np.asarray([100, 300, 0, 200, 0, 0], np.uint32))
    loc = engine.sam_lines(*args[:6], ["cA", "cB", "cC"], *args[7:], located_host=located, clip_fields=(own, res))
    assert [x.split("\t")[2:4] for x in loc] == [["cA", "104"], ["cA", "301"], ["cB", "1"], ["cB", "206"], ["cC", "1"], ["cC", "1"]]
    assert [x.split("\t")[7] for x in loc] == ["301", "104", "206", "1", "1", "1"]
    with pytest.raises(ValueError):
        engine.sam_lines(*args, clip_fields=(own[:3],))
    with pytest.raises(ValueError):
        engine.sam_lines(*args, clip_fields=tuple(a[:5] for a in own))


def test_xa_strings_with_a_shift(engine):
    sec_off = np.asarray([0, 1, 2], np.uint64)
    start = np.asarray([99, 1004], np.uint32)
    old = engine.xa_strings(sec_off, [3, 2], start, None, ["40=", "10=1X29="], rname="chr")
    assert engine.xa_strings(sec_off, [3, 2], start, None, ["40=", "10=1X29="], rname="chr", shift=None) == old
    new = engine.xa_strings(sec_off, np.asarray([0, 1], np.uint16), start, None, ["3S37=", "10=1X25=4S"], rname="chr", shift=np.asarray([3, 0], np.uint16))
    assert old == ["chr,+100,40=,3;chr,-1005,10=1X29=,2;"] and new == ["chr,+103,3S37=,0;chr,-1005,10=1X25=4S,1;"]
    ctg = np.asarray([0, 1], np.uint32)
    assert engine.xa_strings(sec_off, [0, 1], start, ctg, ["3S37=", "40="], located=(["cA", "cB"], [0, 1000, 2000]), shift=[3, 2]) == ["cA,+103,3S37=,0;cB,-7,40=,1;"]
    assert engine.CIGAR_OPS[S] == "S"


# ---- 6. the ABI ---------------------------------------------------------------------------------------------------------------------------------
def test_struct_size_constants_and_the_capability_macro(engine):
    assert C.sizeof(engine.ClipOptions) == 32 and engine.CLIP_LOW == cn.LOW == 1
    hdr = open(os.path.join(ROOT, "include", "kmx.h")).read()
    assert re.search(r"^#define KMX_SOFT_CLIP 1$", hdr, re.M) and re.search(r"^#define KMX_VERSION 5$", hdr, re.M)
    assert re.search(r"^#define KMX_CLIP_LOW 1u", hdr, re.M) and "struct_size;   /* = sizeof(kmx_clip_options): 32 */" in hdr
    assert "NOT A SMITH-WATERMAN REALIGNMENT" in hdr and "not the best local alignment of the read" in hdr
    for name in NEW:
        assert name in engine.EXPORTS and re.search(r"\b" + name + r"\(", hdr) and hasattr(engine.lib(), name)


def test_refusals_that_need_no_device(engine):
    L = engine.lib()
    out = C.c_void_p()
    one = C.c_void_p(1)                                        # never dereferenced: the refusal comes first
    opt = lambda **kw: engine.ClipOptions(**dict(dict(struct_size=32, match=1, mismatch=4, gap_open=6, gap_extend=1, clip_penalty=5, min_score=0,
                                                      flags=0), **kw))
    for sc, o, inout, word in ((one, None, out, b"options is NULL"), (one, opt(), None, b"inout is NULL"), (one, opt(struct_size=31), out, b"struct_size"),
                               (one, opt(flags=1), out, b"flags must be 0"), (one, opt(match=0), out, b"match"), (one, opt(match=256), out, b"match"),
                               (one, opt(mismatch=256), out, b"mismatch"), (one, opt(gap_open=256), out, b"gap_open"),
                               (one, opt(gap_extend=256), out, b"gap_extend"), (one, opt(clip_penalty=65536), out, b"clip_penalty"),
                               (None, opt(match=255, mismatch=255, gap_open=255, gap_extend=255, clip_penalty=65535, min_score=-2 ** 31), out,
                                b"scripts handle is NULL"), (None, opt(mismatch=0, gap_open=0, gap_extend=0, clip_penalty=0, min_score=2 ** 31 - 1), out,
                                                             b"scripts handle is NULL")):
        st = L.kmx_scripts_clip(sc, C.byref(o) if o is not None else None, None, C.byref(inout) if inout is not None else None)
        assert st == 1 and word in L.kmx_last_error() and b"kmx_scripts_clip" in L.kmx_last_error(), word
        assert not out.value                                   # no handle was made
    assert L.kmx_clips_counts(None, None, None, None, None) == 1 and b"kmx_clips_counts" in L.kmx_last_error()
    assert L.kmx_clips_view(None, *[None] * 9) == 1 and b"kmx_clips_view" in L.kmx_last_error()
    assert L.kmx_clips_view_device(None, *[None] * 9) == 1 and b"kmx_clips_view_device" in L.kmx_last_error()
    L.kmx_clips_free(None)
    mo = engine.MdOptions(8, 0)
    letters = np.frombuffer(b"ACGT", np.uint8)
    for fn, name, source in ((L.kmx_clips_md, b"kmx_clips_md", b"alignments"), (L.kmx_clips_rescues_md, b"kmx_clips_rescues_md", b"rescues")):
        for ix, sc, cl, src, tab, o, inout, word in ((one, one, one, one, letters, None, out, b"options is NULL"), (one, one, one, one, letters, mo, None, b"inout is NULL"),
                                                     (one, one, one, one, letters, engine.MdOptions(7, 0), out, b"struct_size"),
                                                     (one, one, one, one, letters, engine.MdOptions(8, 1), out, b"flags must be 0"),
                                                     (one, one, one, one, None, mo, out, b"NULL letters table"), (None, one, one, one, letters, mo, out, b"index is NULL"),
                                                     (one, None, one, one, letters, mo, out, b"scripts handle is NULL"),
                                                     (one, one, None, one, letters, mo, out, b"clips handle is NULL"),
                                                     (one, one, one, None, letters, mo, out, source + b" handle is NULL")):
            st = fn(ix, sc, cl, src, tab.ctypes.data if tab is not None else None, C.byref(o) if o is not None else None, None,
                    C.byref(inout) if inout is not None else None)
            assert st == 1 and word in L.kmx_last_error() and name + b": " in L.kmx_last_error(), word
            assert not out.value


def test_header_with_clip_declarations_is_c99(tmp_path):
    src = tmp_path / "clip.c"
    src.write_text('#include "kmx.h"\n'
                   "#if KMX_SOFT_CLIP != 1 || KMX_VERSION != 5\n#error capability macro\n#endif\n"
                   "_Static_assert(sizeof(kmx_clip_options) == 32, \"eight words\");\n"
                   "_Static_assert(KMX_CLIP_LOW == 1u, \"flag\");\n"
                   "int use(const kmx_index* ix, const kmx_scripts* sc, const kmx_alignments* al, const kmx_rescues* rs, const uint8_t* letters, void* stream) {\n"
                   "  kmx_clip_options o = {sizeof(kmx_clip_options), 1, 4, 6, 1, 5, -3, 0};\n"
                   "  kmx_md_options mo = {sizeof(kmx_md_options), 0};\n"
                   "  kmx_clips* c = 0; kmx_md* m = 0; uint64_t ns, no, nc, nl;\n"
                   "  const int32_t* score; const uint16_t *sl, *sr, *tl, *tr, *nm; const uint8_t* fl; const uint64_t* off; const uint32_t* cigar;\n"
                   "  if (kmx_scripts_clip(sc, &o, stream, &c) != KMX_OK) return 1;\n"
                   "  if (kmx_clips_counts(c, &ns, &no, &nc, &nl) != KMX_OK) return 2;\n"
                   "  if (kmx_clips_view(c, &score, &sl, &sr, &tl, &tr, &nm, &fl, &off, &cigar) != KMX_OK) return 3;\n"
                   "  if (kmx_clips_view_device(c, &score, &sl, &sr, &tl, &tr, &nm, &fl, &off, &cigar) != KMX_OK) return 4;\n"
                   "  if (kmx_clips_md(ix, sc, c, al, letters, &mo, stream, &m) != KMX_OK) return 5;\n"
                   "  if (kmx_clips_rescues_md(ix, sc, c, rs, letters, &mo, stream, &m) != KMX_OK) return 6;\n"
                   "  kmx_md_free(m); kmx_clips_free(c);\n"
                   "  return 0;\n}\n")
    res = subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Wextra", "-Werror", "-c", f"-I{os.path.join(ROOT, 'include')}",
                          str(src), "-o", str(tmp_path / "clip.o")], capture_output=True, text=True)
    assert res.returncode == 0, res.stderr
