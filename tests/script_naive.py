"""The contract of kmx_alignments_scripts in executable form, on the host arrays of a loci handle and an alignments handle, the
reads and the text.

Selection: locus l of read r is selected when best[r] != NO_BEST and l == locus_off[r] + best[r]; with `all` when
dist[l] < SKIPPED.  sel = the selected loci, ascending; read_sel_off = the exclusive prefix sum of the per-read counts.

The script of an entry: q the read (m letters), t = text[start[l]:end[l]] (L letters), a read letter >= sigma equals nothing.
H[i][j] = the unit-cost Levenshtein distance of q[:i] and t[:j] (H[0][j] = j, H[i][0] = i).  Walk from (m, L) to (0, 0); at (i, j)
the first that applies: 1. i > 0, j > 0 and H[i-1][j-1] + c == H[i][j] (c = 0 on equal letters, else 1): '=' or 'X', to
(i-1, j-1); 2. j > 0 and H[i][j-1] + 1 == H[i][j]: 'D', to (i, j-1); 3. 'I', to (i-1, j).  The ops in forward order, run-length
encoded: len << 4 | op with I = 1, D = 2, '=' = 7, X = 8; with `m` both '=' and 'X' become M = 0 before the runs are formed.

An entry whose read is longer than MAX_READ, or with |m - L| > dist[l], or with H[m][L] != dist[l] has an empty script and is
counted as mismatched.

scripts() returns (read_sel_off[nr + 1] u64, sel u32, cig_off[n_sel + 1] u64, cigar u32, n_mismatched)."""
import numpy as np

from tests.align_naive import MAX_READ, NO_BEST, SKIPPED

OP_M, OP_I, OP_D, OP_EQ, OP_X = 0, 1, 2, 7, 8
LETTER = {OP_M: "M", OP_I: "I", OP_D: "D", OP_EQ: "=", OP_X: "X"}


def full_h(q, t, sigma):
    """H[0 .. m][0 .. L] by rows: the horizontal chain as a running minimum."""
    q = np.asarray(q).astype(np.int64)
    t = np.asarray(t).astype(np.int64)
    idx = np.arange(t.size + 1, dtype=np.int64)
    h = np.empty((q.size + 1, t.size + 1), np.int64)
    h[0] = idx
    for i in range(q.size):
        c = int(q[i])
        u = np.empty(t.size + 1, np.int64)
        u[0] = i + 1
        sub = h[i, :-1] + ((t != c) | (c >= sigma))
        np.minimum(h[i, 1:] + 1, sub, out=u[1:])
        h[i + 1] = np.minimum.accumulate(u - idx) + idx
    return h


def walk(q, t, sigma, h):
    """The ops of the canonical script in forward order."""
    i, j = len(q), len(t)
    ops = []
    while i or j:
        if i and j:
            c = 0 if int(q[i - 1]) == int(t[j - 1]) and int(q[i - 1]) < sigma else 1
            if h[i - 1][j - 1] + c == h[i][j]:
                ops.append(OP_X if c else OP_EQ)
                i -= 1
                j -= 1
                continue
        if j and h[i][j - 1] + 1 == h[i][j]:
            ops.append(OP_D)
            j -= 1
        else:
            ops.append(OP_I)
            i -= 1
    return ops[::-1]


def rle(ops, m=False):
    runs = []
    for op in ops:
        if m and op in (OP_EQ, OP_X):
            op = OP_M
        if runs and runs[-1][0] == op:
            runs[-1][1] += 1
        else:
            runs.append([op, 1])
    return [(n << 4) | op for op, n in runs]


def script_one(q, t, d, sigma, m=False):
    """(runs, mismatched) of one entry."""
    if len(q) > MAX_READ or abs(len(q) - len(t)) > d:
        return [], True
    h = full_h(q, t, sigma)
    if int(h[len(q)][len(t)]) != d:
        return [], True
    return rle(walk(q, t, sigma, h), m), False


def select(locus_off, dist, best, all=False):
    """(read_sel_off u64, sel u32)"""
    nr = len(locus_off) - 1
    off, sel = [0], []
    for r in range(nr):
        a, b = int(locus_off[r]), int(locus_off[r + 1])
        if all:
            sel += [l for l in range(a, b) if int(dist[l]) < SKIPPED]
        elif int(best[r]) != NO_BEST:
            sel.append(a + int(best[r]))
        off.append(len(sel))
    return np.asarray(off, np.uint64), np.asarray(sel, np.uint32)


def scripts(text, ranks, roff, locus_off, dist, start, end, best, sigma, all=False, m=False):
    read_sel_off, sel = select(locus_off, dist, best, all)
    read_of = np.repeat(np.arange(len(roff) - 1), np.diff(read_sel_off.astype(np.int64)))
    cig_off, cigar, bad = [0], [], 0
    for r, l in zip(read_of, sel):
        q = ranks[int(roff[r]):int(roff[r + 1])]
        runs, mismatched = script_one(q, text[int(start[l]):int(end[l])], int(dist[l]), sigma, m)
        bad += mismatched
        cigar += runs
        cig_off.append(len(cigar))
    return read_sel_off, sel, np.asarray(cig_off, np.uint64), np.asarray(cigar, np.uint32), bad


def replay(q, t, runs, sigma):
    """Applies a script to q and t: (edits counted, whether it consumes q and t exactly and every '=' / 'X' tells the truth).  M counts
    an edit where the letters differ."""
    i = j = edits = 0
    for v in runs:
        n, op = int(v) >> 4, int(v) & 15
        for _ in range(n):
            if op in (OP_EQ, OP_X, OP_M):
                if i >= len(q) or j >= len(t):
                    return edits, False
                same = int(q[i]) == int(t[j]) and int(q[i]) < sigma
                if (op == OP_EQ and not same) or (op == OP_X and same):
                    return edits, False
                edits += not same
                i += 1
                j += 1
            elif op == OP_I:
                edits += 1
                i += 1
            elif op == OP_D:
                edits += 1
                j += 1
            else:
                return edits, False
    return edits, i == len(q) and j == len(t)


def strings(cig_off, cigar):
    return ["".join(f"{int(v) >> 4}{LETTER[int(v) & 15]}" for v in cigar[int(a):int(b)]) for a, b in zip(cig_off[:-1], cig_off[1:])]
