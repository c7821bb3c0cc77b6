"""The contract of kmx_loci_align in executable form, on the host arrays of a loci handle, the reads and the text.

Locus l of read r (m letters q), D = diag[l], S = span[l], E = max_edits, everything in Python integers:
  S > max_span or m > MAX_READ: dist = SKIPPED, start = end = 0.  Otherwise lo = max(0, D - E), hi = max(lo, min(n, D + S + m + E)),
  T = text[lo:hi) and d = the least Levenshtein distance (unit costs) between q and any substring of T, the empty one included.  A
  read letter >= sigma equals no text letter.  d > E: dist = NONE, start = end = 0.  Else dist = d, end = the smallest offset at which
  a substring at distance d ends, start = the largest s <= end with lev(q, text[s:end)) == d.
  aligned[r] = the loci of the read with dist <= E, best[r] = the index within the read of the one with the least (dist, index),
  0xFFFFFFFF when there is none.

align() is a row-wise numpy DP (free first row, the horizontal chain as a running minimum, then the anchored pass on the reversed
prefix); brute() is the definition itself.  Both return (dist u8, start u32, end u32, best u32, aligned u32)."""
import numpy as np

MAX_EDITS, MAX_READ, SKIPPED, NONE, NO_BEST = 250, 1024, 254, 255, 0xFFFFFFFF


def _last_row(q, t, sigma, anchored):
    """D[m][0 .. len(t)] of q against t: row 0 is zero (free start in t) or 0, 1, 2, ... (anchored at t[0])."""
    idx = np.arange(t.size + 1, dtype=np.int64)
    row = idx.copy() if anchored else np.zeros(t.size + 1, np.int64)
    t = t.astype(np.int64)
    for i in range(q.size):
        c = int(q[i])
        u = np.empty_like(row)
        u[0] = i + 1
        sub = row[:-1] + ((t != c) | (c >= sigma))
        np.minimum(row[1:] + 1, sub, out=u[1:])
        row = np.minimum.accumulate(u - idx) + idx
    return row


def window(n, m, D, S, E):
    lo = max(0, D - E)
    return lo, max(lo, min(n, D + S + m + E))


def align_one(text, q, D, S, E, sigma):
    """(d, start, end) of one locus that is not skipped; d > E comes without its ends."""
    lo, hi = window(text.size, q.size, D, S, E)
    t = text[lo:hi]
    row = _last_row(q, t, sigma, False)
    j = int(np.argmin(row))
    d = int(row[j])
    if d > E:
        return d, 0, 0
    back = _last_row(q[::-1], t[:j][::-1], sigma, True)
    jb = int(np.flatnonzero(back == d)[0])
    return d, lo + j - jb, lo + j


def _lev(a, b, sigma):
    prev = list(range(len(b) + 1))
    for i, x in enumerate(a):
        cur = [i + 1]
        for j, y in enumerate(b):
            cur.append(min(prev[j + 1] + 1, cur[j] + 1, prev[j] + (0 if x == y and x < sigma else 1)))
        prev = cur
    return prev[-1]


def brute_one(text, q, D, S, E, sigma):
    lo, hi = window(text.size, q.size, D, S, E)
    q = [int(x) for x in q]
    best = None
    for e in range(lo, hi + 1):
        for s in range(lo, e + 1):
            key = (_lev(q, [int(x) for x in text[s:e]], sigma), e, -s)
            if best is None or key < best:
                best = key
    return best[0], -best[2], best[1]


def _run(one, text, ranks, roff, locus_off, diag, span, E, max_span, sigma):
    nr, nl = len(roff) - 1, len(diag)
    dist = np.zeros(nl, np.uint8); start = np.zeros(nl, np.uint32); end = np.zeros(nl, np.uint32)
    best = np.full(nr, NO_BEST, np.uint32); aligned = np.zeros(nr, np.uint32)
    for r in range(nr):
        q = np.asarray(ranks[int(roff[r]):int(roff[r + 1])])
        key = None
        for l in range(int(locus_off[r]), int(locus_off[r + 1])):
            if int(span[l]) > max_span or q.size > MAX_READ:
                dist[l] = SKIPPED
                continue
            d, s, e = one(text, q, int(diag[l]), int(span[l]), E, sigma)
            if d > E:
                dist[l] = NONE
                continue
            dist[l], start[l], end[l] = d, s, e
            aligned[r] += 1
            if key is None or (d, l) < key:
                key = (d, l)
        if key is not None:
            best[r] = key[1] - int(locus_off[r])
    return dist, start, end, best, aligned


def align(text, ranks, roff, locus_off, diag, span, E, max_span, sigma):
    return _run(align_one, text, ranks, roff, locus_off, diag, span, E, max_span, sigma)


def brute(text, ranks, roff, locus_off, diag, span, E, max_span, sigma):
    return _run(brute_one, text, ranks, roff, locus_off, diag, span, E, max_span, sigma)
