"""The contract of kmx_scripts_realign in executable form, cell by cell, on the host arrays of a scripts handle, of its alignments
handle, of the reads and of the text.  Everything is in int (int64 on the device side of the contract).

Entry e of the scripts: locus l = sel[e]; read r = the internal read with read_sel_off[r] <= e < read_sel_off[r + 1]; q = its m
letters; t = text[start[l], end[l]), L letters; d = dist[l].  Options: a = match, b = mismatch, o = gap_open, x = gap_extend,
p = clip_penalty, min_score.  A gap of len letters costs o + len x.  A read letter >= sigma equals nothing.

  Cell (i, j) exists for 0 <= i <= m, 0 <= j <= L, |j - i| <= d.  Every other cell is -inf in every state.
  Z(i) = 0 if i == 0 else -p                      a path may begin at any cell; a left clip pays p
  s(i, j) = a if q[i - 1] == t[j - 1] and q[i - 1] < sigma else -b
  E(i, j) = max(E(i, j - 1) - x, H(i, j - 1) - o - x)                ends with D (a text letter)
  F(i, j) = max(F(i - 1, j) - x, H(i - 1, j) - o - x)                ends with I (a read letter)
  H(i, j) = max(Z(i), H(i - 1, j - 1) + s(i, j), E(i, j), F(i, j))
  V(i, j) = H(i, j) - p [i < m]

  End cell (i1, j1): the greatest V; among equals the least i, then the least j.
  Walk from (i1, j1) in state H.
    H at (i, j), the first that applies: 1. H == Z(i): stop, (i0, j0) = (i, j).  2. i, j > 0 and H == H(i - 1, j - 1) + s: emit '=' or
      'X', go to (i - 1, j - 1) in state H.  3. H == E(i, j): state E.  4. state F.
    E: emit D; the next state is H if E(i, j) == H(i, j - 1) - o - x, else E; go to (i, j - 1).
    F: the same with I, F, H(i - 1, j) and (i - 1, j).

The entry is REALIGNED when the path is not empty and V(i1, j1) >= min_score: score = V, sl = i0, sr = m - i1, tl = j0, tr = L - j1,
nm = the X + I + D ops, runs = sl S (if sl > 0), the ops forwards as BAM runs, sr S (if sr > 0), cflags = REALIGNED (2).
Every other entry is what kmx_scripts_clip makes of a LOW entry (tests/clip_naive.py): the script's own runs, score = W[R],
sl = sr = tl = tr = 0, nm = its X + I + D lengths, cflags = LOW (1).  An entry whose script is empty is not looked at: zeros, no
runs, LOW.

Handles that do not belong together (guards()).  An entry with runs is such an "other entry", whole and LOW, and neither its read
nor its text is looked at, when there is no read r for it; when its read range is not one (roff[r] <= roff[r + 1] <= the letters
handed over); when m > MAX_READ; when sel[e] is not below the number of loci; when start[l] <= end[l] <= n does not hold; when
dist[l] > MAX_EDITS; or when |m - L| > dist[l].  Every entry of handles that do belong together passes all of them.

realign() returns (score i32, sl u16, sr u16, tl u16, tr u16, nm u16, cflags u8, cig_off u64[n_sel + 1], cigar u32, n_clipped, n_low)."""
import numpy as np

from tests import clip_naive as cn
from tests.align_naive import MAX_EDITS, MAX_READ

OP_I, OP_D, OP_S, OP_EQ, OP_X = cn.OP_I, cn.OP_D, cn.OP_S, cn.OP_EQ, cn.OP_X
LOW, REALIGNED = 1, 2
DEFAULTS = dict(cn.DEFAULTS)
NEG = -(1 << 60)                                               # -inf: whatever falls below half of it is put back to it
strings, parse = cn.strings, cn.parse


def _floor(v):
    return NEG if v < NEG // 2 else v


class Band:
    """One state of the recurrence over the cells that exist, a row of 2d + 1 diagonals per read letter: [i, j] is -inf off the band
    and off the rectangle."""

    def __init__(self, m, L, d):
        self.m, self.L, self.d = m, L, d
        self.rows = [[NEG] * (2 * d + 1) for _ in range(m + 1)]

    def exists(self, i, j):
        return 0 <= i <= self.m and 0 <= j <= self.L and abs(j - i) <= self.d

    def __getitem__(self, ij):
        i, j = ij
        return self.rows[i][j - i + self.d] if self.exists(i, j) else NEG

    def __setitem__(self, ij, v):
        self.rows[ij[0]][ij[1] - ij[0] + self.d] = v


def tables(q, t, d, sigma, match=1, mismatch=4, gap_open=6, gap_extend=1, clip_penalty=5, **_):
    """(H, E, F, s, Z): the three states as Bands, s and Z as functions."""
    m, L = len(q), len(t)
    q, t = [int(c) for c in q], [int(c) for c in t]
    a, b, o, x, p = match, mismatch, gap_open, gap_extend, clip_penalty
    Z = lambda i: 0 if i == 0 else -p
    s = lambda i, j: a if q[i - 1] == t[j - 1] and q[i - 1] < sigma else -b
    H, E, F = Band(m, L, d), Band(m, L, d), Band(m, L, d)
    for i in range(m + 1):
        for j in range(max(0, i - d), min(L, i + d) + 1):
            e = _floor(max(E[i, j - 1] - x, H[i, j - 1] - o - x))
            f = _floor(max(F[i - 1, j] - x, H[i - 1, j] - o - x))
            h = max(Z(i), e, f)
            if i > 0 and j > 0:
                h = max(h, _floor(H[i - 1, j - 1] + s(i, j)))
            H[i, j], E[i, j], F[i, j] = h, e, f
    return H, E, F, s, Z


def end_cell(H, clip_penalty):
    """(V, i1, j1): the greatest V, the least i, the least j"""
    best = None
    for i in range(H.m + 1):
        for j in range(max(0, i - H.d), min(H.L, i + H.d) + 1):
            v = H[i, j] - (clip_penalty if i < H.m else 0)
            if best is None or v > best[0]:                    # (rows and columns ascend: the first of equals stays)
                best = (v, i, j)
    return best


def align_one(q, t, d, sigma, **options):
    """(V, i0, j0, i1, j1, ops forwards as a list of op codes) of one rectangle"""
    opt = dict(DEFAULTS, **options)
    o, x = opt["gap_open"], opt["gap_extend"]
    H, E, F, s, Z = tables(q, t, d, sigma, **opt)
    v, i, j = end_cell(H, opt["clip_penalty"])
    i1, j1 = i, j
    ops, state = [], "H"
    while True:
        if state == "H":
            h = H[i, j]
            if h == Z(i):
                break
            if i > 0 and j > 0 and H.exists(i - 1, j - 1) and h == H[i - 1, j - 1] + s(i, j):
                ops.append(OP_EQ if s(i, j) > 0 else OP_X)
                i, j = i - 1, j - 1
            elif h == E[i, j]:
                state = "E"
            else:
                state = "F"
        elif state == "E":
            ops.append(OP_D)
            state = "H" if E[i, j] == H[i, j - 1] - o - x else "E"
            j -= 1
        else:
            ops.append(OP_I)
            state = "H" if F[i, j] == H[i - 1, j] - o - x else "F"
            i -= 1
    return v, i, j, i1, j1, ops[::-1]


def run_length(ops):
    runs = []
    for op in ops:
        if runs and runs[-1][0] == op:
            runs[-1][1] += 1
        else:
            runs.append([op, 1])
    return [(n << 4) | op for op, n in runs]


def whole(script_runs, **options):
    """what kmx_scripts_clip makes of a LOW entry: (runs, score, 0, 0, 0, 0, nm, LOW)"""
    opt = dict(DEFAULTS, **options)
    opt["min_score"] = 1 << 62
    return cn.clip_one(script_runs, **opt)


def realign_one(q, t, d, sigma, script_runs, **options):
    """(new runs, score, sl, sr, tl, tr, nm, cflags) of one entry with the script `script_runs`"""
    script_runs = [int(v) for v in script_runs]
    if not script_runs:
        return [], 0, 0, 0, 0, 0, 0, LOW
    opt = dict(DEFAULTS, **options)
    v, i0, j0, i1, j1, ops = align_one(q, t, d, sigma, **opt)
    if not ops or v < opt["min_score"]:
        return whole(script_runs, **opt)
    sl, sr = i0, len(q) - i1
    runs = ([(sl << 4) | OP_S] if sl else []) + run_length(ops) + ([(sr << 4) | OP_S] if sr else [])
    return runs, v, sl, sr, j0, len(t) - j1, sum(op != OP_EQ for op in ops), REALIGNED


GUARDS = ("no_read", "roff", "long_read", "interval", "dist", "gap", "locus")


def guards(l, n_loci, r, roff, n_letters, dist, start, end, n):
    """The names of the guards that keep entry (l, r) from the band, [] for none: the rule for handles that do not belong together.
      no_read    there is no read r with read_sel_off[r] <= e < read_sel_off[r + 1]
      roff       its read range is not one: roff[r] <= roff[r + 1] <= the letters handed over does not hold
      long_read  m > MAX_READ
      locus      sel[e] is not below the number of loci
      interval   start <= end <= n does not hold
      dist       dist > MAX_EDITS (a locus that was skipped or not aligned among them)
      gap        |m - L| > dist
    A guard is looked at only where the arrays it needs can be read."""
    out = []
    m = None
    if r is None:
        out.append("no_read")
    elif not int(roff[r]) <= int(roff[r + 1]) <= n_letters:
        out.append("roff")
    else:
        m = int(roff[r + 1]) - int(roff[r])
        if m > MAX_READ:
            out.append("long_read")
    if l >= n_loci:
        return out + ["locus"]
    s, t, d = int(start[l]), int(end[l]), int(dist[l])
    if not s <= t <= n:
        out.append("interval")
    if d > MAX_EDITS:
        out.append("dist")
    if not out and abs(m - (t - s)) > d:
        out.append("gap")
    return out


def realign(read_sel_off, sel, cig_off, cigar, dist, start, end, ranks, roff, text, sigma, n_loci=None, why=None, **options):
    """The nine clips arrays and the two counters of a scripts handle (read_sel_off, sel, cig_off, cigar), its alignments (dist, start,
    end; n_loci of them: all by default), the internal reads (ranks, roff) and the text.  why: a dict that receives guards() of every
    entry with runs."""
    n = len(sel)
    n_loci = len(dist) if n_loci is None else n_loci
    nr = len(roff) - 1
    score, cflags = np.zeros(n, np.int32), np.zeros(n, np.uint8)
    sl, sr, tl, tr, nm = (np.zeros(n, np.uint16) for _ in range(5))
    off, out = [0], []
    for e in range(n):
        script = [int(v) for v in cigar[int(cig_off[e]):int(cig_off[e + 1])]]
        l = int(sel[e])
        r = int(np.searchsorted(read_sel_off, e, side="right")) - 1         # the read with read_sel_off[r] <= e < read_sel_off[r + 1]
        if not (0 <= r < nr and int(read_sel_off[r]) <= e < int(read_sel_off[r + 1])):
            r = None
        held = guards(l, n_loci, r, roff, len(ranks), dist, start, end, len(text)) if script else []
        if why is not None and script:
            why[e] = held
        if held:                                               # handles that do not belong together: whole and LOW, nothing else is read
            runs, score[e], sl[e], sr[e], tl[e], tr[e], nm[e], cflags[e] = whole(script, **options)
        else:
            q = ranks[int(roff[r]):int(roff[r + 1])] if script else ranks[:0]
            t = text[int(start[l]):int(end[l])] if script else text[:0]
            runs, score[e], sl[e], sr[e], tl[e], tr[e], nm[e], cflags[e] = realign_one(q, t, int(dist[l]) if script else 0, sigma, script, **options)
        out += runs
        off.append(len(out))
    n_clipped = int(((sl.astype(np.int64) + sr) > 0).sum())
    return score, sl, sr, tl, tr, nm, cflags, np.asarray(off, np.uint64), np.asarray(out, np.uint32), n_clipped, int((cflags & LOW).astype(bool).sum())
