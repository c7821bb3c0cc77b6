"""The contract of kmx_scripts_clip in executable form, on the host arrays of a scripts handle (cig_off, cigar), and of
kmx_clips_md / kmx_clips_rescues_md on top of tests/md_naive.py.

This is post-alignment trimming of the edit-optimal script, not a Smith-Waterman realignment: the clipped alignment is the
best-scoring PART OF THE CANONICAL SCRIPT, not the best local alignment of the read.

Entry e has the runs r_0 .. r_{R-1} = cigar[cig_off[e] .. cig_off[e + 1]) as len << 4 | op with I = 1, D = 2, '=' = 7, X = 8.  With
the options a = match, b = mismatch, o = gap_open, x = gap_extend, p = clip_penalty, everything in int64:

  w('=' of len) = len a,  w(X) = -len b,  w(I) = w(D) = -(o + len x);  W[0] = 0, W[k + 1] = W[k] + w(r_k).
  A left cut i is 0 or any k with r_k an '=' run; a right cut j is R or any k with r_{k-1} an '=' run.
  The candidates are all (i, j) with i < j, and (0, R) always (even for R = 0).
  V(i, j) = W[j] - W[i] - p [i > 0] - p [j < R].
  The candidate with the greatest V is taken; among equals the smallest i, then the largest j.
  If that V < min_score the entry stays whole, (i, j) = (0, R), and the bit LOW is set in cflags[e].

Outputs per entry: score = V of the (i, j) that is kept (for a LOW entry V(0, R) = W[R]) saturated to int32; sl / sr = the read
letters (= X I) of the runs in front of i / from j on, tl / tr = their text letters (= X D), nm = the X + I + D lengths of the kept
runs (all five saturated at 65535); the new runs: sl S (op 4) when sl > 0, r_i .. r_{j-1}, sr S when sr > 0.

An entry with an op other than = X I D is copied unclipped with score 0, sl = sr = tl = tr = nm = 0 and the LOW bit.

clip() returns (score i32, sl u16, sr u16, tl u16, tr u16, nm u16, cflags u8, cig_off u64[n_sel + 1], cigar u32, n_clipped, n_low)."""
import numpy as np

from tests import md_naive

OP_I, OP_D, OP_S, OP_EQ, OP_X = 1, 2, 4, 7, 8
LOW = 1
LETTER = {OP_I: "I", OP_D: "D", OP_S: "S", OP_EQ: "=", OP_X: "X"}
DEFAULTS = dict(match=1, mismatch=4, gap_open=6, gap_extend=1, clip_penalty=5, min_score=0)


def weight(v, match, mismatch, gap_open, gap_extend):
    length, op = int(v) >> 4, int(v) & 15
    if op == OP_EQ:
        return length * match
    if op == OP_X:
        return -length * mismatch
    return -(gap_open + length * gap_extend)


def choose(runs, match=1, mismatch=4, gap_open=6, gap_extend=1, clip_penalty=5, min_score=0):
    """(i, j, V, low) of one entry whose ops are all = X I D: every candidate is looked at."""
    R = len(runs)
    W = [0]
    for v in runs:
        W.append(W[-1] + weight(v, match, mismatch, gap_open, gap_extend))
    lefts = [0] + [k for k in range(1, R) if (int(runs[k]) & 15) == OP_EQ]
    rights = [k for k in range(1, R) if (int(runs[k - 1]) & 15) == OP_EQ] + [R]
    cands = {(0, R)} | {(i, j) for i in lefts for j in rights if i < j}
    value = {(i, j): W[j] - W[i] - clip_penalty * (i > 0) - clip_penalty * (j < R) for i, j in cands}
    i, j = max(cands, key=lambda c: (value[c], -c[0], c[1]))
    if value[(i, j)] < min_score:
        return 0, R, value[(0, R)], True
    return i, j, value[(i, j)], False


def letters_of(runs, ops):
    return sum(int(v) >> 4 for v in runs if (int(v) & 15) in ops)


def clip_one(runs, **options):
    """(new runs, score, sl, sr, tl, tr, nm, cflags) of one entry."""
    runs = [int(v) for v in runs]
    if any((v & 15) not in (OP_I, OP_D, OP_EQ, OP_X) for v in runs):
        return runs, 0, 0, 0, 0, 0, 0, LOW
    i, j, v, low = choose(runs, **options)
    sat = lambda n: min(n, 0xFFFF)
    sl, sr = sat(letters_of(runs[:i], (OP_EQ, OP_X, OP_I))), sat(letters_of(runs[j:], (OP_EQ, OP_X, OP_I)))
    tl, tr = sat(letters_of(runs[:i], (OP_EQ, OP_X, OP_D))), sat(letters_of(runs[j:], (OP_EQ, OP_X, OP_D)))
    nm = sat(letters_of(runs[i:j], (OP_X, OP_I, OP_D)))
    out = ([(sl << 4) | OP_S] if sl else []) + runs[i:j] + ([(sr << 4) | OP_S] if sr else [])
    return out, max(-2 ** 31, min(2 ** 31 - 1, v)), sl, sr, tl, tr, nm, LOW if low else 0


def clip(cig_off, cigar, **options):
    n = len(cig_off) - 1
    score, cflags = np.zeros(n, np.int32), np.zeros(n, np.uint8)
    sl, sr, tl, tr, nm = (np.zeros(n, np.uint16) for _ in range(5))
    off, out = [0], []
    for e in range(n):
        runs, score[e], sl[e], sr[e], tl[e], tr[e], nm[e], cflags[e] = clip_one(cigar[int(cig_off[e]):int(cig_off[e + 1])], **options)
        out += runs
        off.append(len(out))
    n_clipped = int(((sl.astype(np.int64) + sr) > 0).sum())
    return score, sl, sr, tl, tr, nm, cflags, np.asarray(off, np.uint64), np.asarray(out, np.uint32), n_clipped, int((cflags & LOW).astype(bool).sum())


def parse(cigar_string):
    """The runs of a CIGAR string such as "138=3X1=5X1=2X"."""
    code = {c: op for op, c in LETTER.items()}
    runs, num = [], ""
    for ch in cigar_string:
        if ch.isdigit():
            num += ch
        else:
            runs.append((int(num) << 4) | code[ch])
            num = ""
    return runs


def strings(cig_off, cigar):
    return ["".join(f"{int(v) >> 4}{LETTER[int(v) & 15]}" for v in cigar[int(a):int(b)]) for a, b in zip(cig_off[:-1], cig_off[1:])]


def md(sel, clip_cig_off, clip_cigar, tl, tr, start, end, text, letters, bound=None):
    """The contract of kmx_clips_md / kmx_clips_rescues_md: the rule of md_naive.md on the clipped runs with the text cursor starting
    at start[sel[e]] + tl[e], the end test against end[sel[e]] - tr[e], and S treated like I.  An entry whose tl + tr exceeds
    end - start is mismatched.  Returns (md_off u64, md u8, n_mismatched)."""
    bound = len(start) if bound is None else bound
    n = len(sel)
    s2, t2 = np.zeros(n, np.int64), np.zeros(n, np.int64)
    for e, l in enumerate(sel):
        if int(l) < bound:
            s, t = int(start[int(l)]), int(end[int(l)])
            if s <= t and int(tl[e]) + int(tr[e]) <= t - s:
                s2[e], t2[e] = s + int(tl[e]), t - int(tr[e])
            else:
                s2[e], t2[e] = 1, 0                            # refused by the rule: not s <= t
        else:
            s2[e], t2[e] = 1, 0
    as_insert = np.asarray([(int(v) & ~15) | OP_I if (int(v) & 15) == OP_S else int(v) for v in clip_cigar], np.uint32)
    return md_naive.md(np.arange(n), clip_cig_off, as_insert, s2, t2, text, letters)
