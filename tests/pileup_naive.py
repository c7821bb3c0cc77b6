"""The contracts of kmx_clips_pileup_device / kmx_clips_rescues_pileup and of kmx_pileup_sites (include/kmx.h, KMX_PILEUP) as plain
loops over Python ints: test infrastructure, never imported by the package.

add() replays the runs of every entry against its read into the (sigma + 3, hi - lo) planes; sites() lists the positions where
something other than the reference letter is frequent.  The channels: the letters by rank, OTHER = sigma, DEL = sigma + 1,
INS = sigma + 2."""
import numpy as np

OP_I, OP_D, OP_S, OP_EQ, OP_X = 1, 2, 4, 7, 8
CLIP_LOW = 1
NO_FLOOR = -2 ** 31
SITES = ("pos", "ref", "alt", "depth", "count", "ref_count")
U32 = 0xFFFFFFFF


def planes(lo, hi, sigma):
    """zeroed planes of the region [lo, hi)"""
    return np.zeros((sigma + 3, hi - lo), np.uint32)


def runs_of(cig_off, n_ops, e):
    """the runs [a, b) of entry e, inside cigar[n_ops] whatever the offsets hold"""
    a = min(int(cig_off[e]), n_ops)
    return a, min(max(int(cig_off[e + 1]), a), n_ops)


CAUSES = ("bound", "no_read", "roff", "interval", "clip", "op", "inner_s", "text_len", "read_len")


def mismatch_causes(l, bound, r, roff, n_letters, start, end, n, tl, tr, runs):
    """Rule 3 of the contract for one entry with runs: the names of the causes that hold, [] for none.  A cause is looked at only where
    the arrays it needs can be read: the interval's behind the bound's, the lengths' behind those of the read and of the interval.
      bound      l >= the bound of start / end
      no_read    there is no read r with read_sel_off[r] <= e < read_sel_off[r + 1]
      roff       its roff range is not one: roff[r] <= roff[r + 1] <= the letters handed over does not hold
      interval   not s <= t <= n
      clip       tl + tr > t - s
      op         an op other than = X I D S
      inner_s    an S run that is neither the first nor the last
      text_len   the = X D lengths differ from t - s - tl - tr
      read_len   the = X I S lengths differ from m"""
    out = []
    if l >= bound:
        out.append("bound")
    if r is None:
        out.append("no_read")
    elif not int(roff[r]) <= int(roff[r + 1]) <= n_letters:
        out.append("roff")
    if l < bound:
        s, t = int(start[l]), int(end[l])
        if not s <= t <= n:
            out.append("interval")
        elif tl + tr > t - s:
            out.append("clip")
    if any(op not in (OP_EQ, OP_X, OP_I, OP_D, OP_S) for op, _ in runs):
        out.append("op")
    if any(op == OP_S and k not in (0, len(runs) - 1) for k, (op, _) in enumerate(runs)):
        out.append("inner_s")
    if out:
        return out
    if sum(ln for op, ln in runs if op in (OP_EQ, OP_X, OP_D)) != t - s - tl - tr:
        out.append("text_len")
    if sum(ln for op, ln in runs if op in (OP_EQ, OP_X, OP_I, OP_S)) != int(roff[r + 1]) - int(roff[r]):
        out.append("read_len")
    return out


def add(counts, lo, hi, sigma, scripts, clips, start, end, ranks, roff, mapq=None, *, n, bound=None, min_score=NO_FLOOR, min_mapq=0,
        skip_low=False, why=None):
    """counts[(sigma + 3, hi - lo)] += the pileup of the entries, in place.  scripts = (read_sel_off, sel, cig_off, cigar), the host view
    of a Scripts; clips = the host view of its Clips (score, sl, sr, tl, tr, nm, cflags, cig_off, cigar) or None; start / end: the
    arrays that sel indexes (`bound` of them: all by default); ranks / roff: the reads the entries run over; mapq: one value per pair of
    internal reads, or None; n: the text length; why: a dict that receives, for every entry that reaches rule 3, the causes that make it
    MISMATCHED ([] for an ADDED one).  Returns dict(n_added, n_filtered, n_mismatched, n_cells) of this call."""
    read_sel_off, sel, cig_off, cigar = scripts
    if clips is not None:
        score, _, _, ctl, ctr, _, cflags, cig_off, cigar = clips
    bound = len(start) if bound is None else bound
    nr = len(roff) - 1
    out = dict(n_added=0, n_filtered=0, n_mismatched=0, n_cells=0)
    DEL, INS = sigma + 1, sigma + 2

    def put(c, pos):
        if lo <= pos < hi:
            counts[c, pos - lo] = (int(counts[c, pos - lo]) + 1) & U32
            out["n_cells"] += 1

    for e in range(len(sel)):
        a, b = runs_of(cig_off, len(cigar), e)
        if b <= a:                                             # 1. no runs: no counter moves
            continue
        runs = [(int(v) & 15, int(v) >> 4) for v in cigar[a:b]]
        r = int(np.searchsorted(read_sel_off, e, side="right")) - 1         # the read with read_sel_off[r] <= e < read_sel_off[r + 1]
        if not (0 <= r < nr and int(read_sel_off[r]) <= e < int(read_sel_off[r + 1])):
            r = None
        tl, tr = (int(ctl[e]), int(ctr[e])) if clips is not None else (0, 0)
        # 2. the filters
        if clips is not None and skip_low and int(cflags[e]) & CLIP_LOW:
            out["n_filtered"] += 1
            continue
        if clips is not None and int(score[e]) < min_score:
            out["n_filtered"] += 1
            continue
        if mapq is not None and r is not None and int(mapq[r >> 1]) < min_mapq:
            out["n_filtered"] += 1
            continue
        # 3. the pass over the runs in front of any add
        l = int(sel[e])
        causes = mismatch_causes(l, bound, r, roff, len(ranks), start, end, n, tl, tr, runs)
        if why is not None:
            why[e] = causes
        if causes:
            out["n_mismatched"] += 1
            continue
        s, t = int(start[l]), int(end[l])
        q = ranks[int(roff[r]):int(roff[r + 1])]
        # 4. the replay
        out["n_added"] += 1
        t0, t1 = s + tl, t - tr
        i, j = 0, t0
        for op, ln in runs:
            if op == OP_S:
                i += ln
            elif op in (OP_EQ, OP_X):
                for x in range(ln):
                    c = int(q[i + x])
                    put(c if c < sigma else sigma, j + x)
                i += ln
                j += ln
            elif op == OP_D:
                for x in range(ln):
                    put(DEL, j + x)
                j += ln
            else:                                              # I: once per run, at the text letter in front of it; not at either end
                if t0 < j < t1:
                    put(INS, j - 1)
                i += ln
    return out


def sites(counts, lo, text, sigma, ctg_off=None, *, min_depth=1, min_alt=1, frac=(1, 5)):
    """The records of the planes counts[(sigma + 3, len)] over [lo, lo + len): (pos u32, ref u8, alt u8, depth u32, count u32,
    ref_count u32, ctg u32 or None, n_covered).  One record per position and passing channel, ordered by (pos, channel)."""
    num, den = frac
    rec = []
    n_covered = 0
    for x in range(counts.shape[1]):
        pos = lo + x
        depth = sum(int(counts[c, x]) for c in range(sigma + 2))
        if depth < max(min_depth, 1):
            continue
        n_covered += 1
        ref = int(text[pos])
        for c in list(range(sigma)) + [sigma + 1, sigma + 2]:
            cnt = int(counts[c, x])
            if c != ref and cnt >= max(min_alt, 1) and cnt * den >= num * depth:
                ctg = None if ctg_off is None else int(np.searchsorted(np.asarray(ctg_off, np.uint64), pos, side="right")) - 1
                rec.append((pos, ref, c, min(depth, U32), cnt, int(counts[ref, x]) if ref < sigma else 0, ctg))
    col = lambda k, dt: np.asarray([r[k] for r in rec], dt)
    return (col(0, np.uint32), col(1, np.uint8), col(2, np.uint8), col(3, np.uint32), col(4, np.uint32), col(5, np.uint32),
            None if ctg_off is None else col(6, np.uint32), n_covered)


def expanded(counts, lo, hi, sigma, runs, q, t0):
    """A second implementation of the replay of one consistent entry: the CIGAR is expanded to a string of per-column ops first, and
    the columns are walked with both cursors.  runs: (op, len) pairs, q: the read, t0: the first text position."""
    cols = "".join({OP_EQ: "=", OP_X: "X", OP_I: "I", OP_D: "D", OP_S: "S"}[op] * ln for op, ln in runs)
    t1 = t0 + sum(c in "=XD" for c in cols)
    i, j = 0, t0
    for k, c in enumerate(cols):
        if c in "=X":
            pos, ch = j, (int(q[i]) if int(q[i]) < sigma else sigma)
        elif c == "D":
            pos, ch = j, sigma + 1
        elif c == "I" and (k == 0 or cols[k - 1] != "I") and t0 < j < t1:
            pos, ch = j - 1, sigma + 2
        else:
            pos = None
        if pos is not None and lo <= pos < hi:
            counts[ch, pos - lo] += 1
        i += c in "=XIS"
        j += c in "=XD"
