"""The contract of kmx_placements_secondaries in executable form (include/kmx.h, KMX_MAP_SECONDARIES).

On the host arrays of the loci and alignments of a doubled batch and of the placements (Placements.host(): locus, strand, dist,
start, end first).  For public read i: a = locus_off[2i], b = locus_off[2i + 1], c = locus_off[2i + 2], clamped into [0, n_loci] and
made ascending; locus l in [a, c) has strand 0 if l < b, else 1.  The primary is P = (strand[i], start[i], end[i]) with distance
dist[i]; an unplaced read (strand 255) has no entries.  A locus is a candidate when dist[l] < SKIPPED, l != locus[i] and
dist[l] <= dist[i] + max_delta (None or 0xFFFFFFFF: no bound).  Two places lie elsewhere from each other when their strands differ or
max(x0, y0) >= min(x1, y1).  Greedy: T = {P}; among the candidates not yet taken that lie elsewhere from every member of T take the
one with the least (dist, l); none: more = 0; N taken already: more = 1; else add it to T and repeat.  The entries of a read are
its taken loci in ascending locus index; sec_off counts them per internal read.

secondaries and secondaries_loop return (sec_off u64[2 nr + 1], locus u32, dist u8, start u32, end u32, more u8[nr], n_sec,
n_multi, n_truncated)."""
import numpy as np

SKIPPED, NONE = 254, 255
NO_BEST = 0xFFFFFFFF
NO_DELTA = 0xFFFFFFFF
SECONDARY_MAX = 32
NAMES = ("sec_off", "locus", "dist", "start", "end", "more", "n_sec", "n_multi", "n_truncated")


def _ranges(locus_off, n_loci, i):
    a = min(max(int(locus_off[2 * i]), 0), n_loci)
    b = min(max(int(locus_off[2 * i + 1]), a), n_loci)
    c = min(max(int(locus_off[2 * i + 2]), b), n_loci)
    return a, b, c


def _pack(nr, taken_per_read, more, dist, start, end):
    cnt = np.zeros(2 * nr, np.int64)
    flat = []
    for i, (b, taken) in enumerate(taken_per_read):
        taken = sorted(taken)
        cnt[2 * i] = sum(1 for l in taken if l < b)
        cnt[2 * i + 1] = len(taken) - cnt[2 * i]
        flat += taken
    sec_off = np.zeros(2 * nr + 1, np.uint64)
    sec_off[1:] = np.cumsum(cnt)
    locus = np.asarray(flat, np.uint32)
    idx = locus.astype(np.int64)
    more = np.asarray(more, np.uint8)
    n_multi = sum(1 for _, t in taken_per_read if t)
    return (sec_off, locus, np.asarray(dist, np.uint8)[idx], np.asarray(start, np.uint32)[idx], np.asarray(end, np.uint32)[idx], more,
            int(locus.size), int(n_multi), int(more.sum()))


def secondaries(locus_off, dist, start, end, placements_host, N, max_delta=None):
    """The greedy selection by masks over the loci of a read."""
    p_locus, p_strand, p_dist, p_start, p_end = (np.asarray(x).astype(np.int64) for x in placements_host[:5])
    d_all = np.asarray(dist).astype(np.int64); s_all = np.asarray(start).astype(np.int64); e_all = np.asarray(end).astype(np.int64)
    nr = (len(locus_off) - 1) // 2
    bounded = max_delta is not None and int(max_delta) != NO_DELTA
    per, more = [], np.zeros(nr, np.uint8)
    for i in range(nr):
        a, b, c = _ranges(locus_off, d_all.size, i)
        taken = []
        per.append((b, taken))
        if p_strand[i] == 255:
            continue
        l = np.arange(a, c)
        s = (l >= b).astype(np.int64)
        d, x0, x1 = d_all[a:c], s_all[a:c], e_all[a:c]

        def elsewhere(t, y0, y1):
            return (s != t) | (np.maximum(x0, y0) >= np.minimum(x1, y1))

        live = (d < SKIPPED) & (l != p_locus[i]) & elsewhere(p_strand[i], p_start[i], p_end[i])
        if bounded:
            live &= d <= p_dist[i] + int(max_delta)
        key = d * (1 << 32) + l
        while live.any():
            if len(taken) == N:
                more[i] = 1
                break
            j = int(np.where(live, key, np.iinfo(np.int64).max).argmin())
            taken.append(int(l[j]))
            live[j] = False
            live &= elsewhere(s[j], x0[j], x1[j])
    return _pack(nr, per, more, dist, start, end)


def secondaries_loop(locus_off, dist, start, end, placements_host, N, max_delta=None):
    """The definition one locus at a time: every round tests every candidate against every member of T (the checker of the
    checker)."""
    p_locus, p_strand, p_dist, p_start, p_end = placements_host[:5]
    nr = (len(locus_off) - 1) // 2
    bounded = max_delta is not None and int(max_delta) != NO_DELTA
    per, more = [], [0] * nr
    for i in range(nr):
        a, b, c = _ranges(locus_off, len(dist), i)
        taken = []
        per.append((b, taken))
        if int(p_strand[i]) == 255:
            continue
        T = [(int(p_strand[i]), int(p_start[i]), int(p_end[i]))]
        while True:
            pick = None
            for l in range(a, c):
                d = int(dist[l])
                if d >= SKIPPED or l == int(p_locus[i]) or l in taken:
                    continue
                if bounded and d > int(p_dist[i]) + int(max_delta):
                    continue
                s, x0, x1 = (0 if l < b else 1), int(start[l]), int(end[l])
                if all(s != t or max(x0, y0) >= min(x1, y1) for t, y0, y1 in T):
                    if pick is None or (d, l) < pick:
                        pick = (d, l)
            if pick is None:
                break
            if len(taken) == N:
                more[i] = 1
                break
            l = pick[1]
            taken.append(l)
            T.append((0 if l < b else 1, int(start[l]), int(end[l])))
    return _pack(nr, per, more, dist, start, end)


def xa(sec_off, dist, start, cigars, rname=None, ctg=None, names=None, ctg_off=None, strand_names="+-"):
    """One XA:Z: value per public read: "" or items rname,<strand><pos>,CIGAR,NM; with pos 1-based; with ctg / names / ctg_off the
    name of the entry's contig and a contig-local pos."""
    out = []
    for i in range((len(sec_off) - 1) // 2):
        text = ""
        for e in range(int(sec_off[2 * i]), int(sec_off[2 * i + 2])):
            sign = strand_names[0 if e < int(sec_off[2 * i + 1]) else 1]
            if ctg is not None:
                name, pos = names[int(ctg[e])], int(start[e]) - int(ctg_off[int(ctg[e])]) + 1
            else:
                name, pos = rname, int(start[e]) + 1
            text += f"{name},{sign}{pos},{cigars[e] or '*'},{int(dist[e])};"
        out.append(text)
    return out
