"""The contract of kmx_reads_strands and kmx_alignments_fold_strands in executable form (include/kmx.h, KMX_MAP_STRANDS).

The doubled batch.  Internal read 2i is read i, internal read 2i + 1 its reverse complement rc(q)[j] = complement[c] if c < sigma
else c, with c = q[m - 1 - j]; the letters lie side by side: roff2[2i] = 2 roff[i], roff2[2i + 1] = 2 roff[i] + m.

The fold, on the host arrays of the loci and alignments of a doubled batch.  For public read i: a = locus_off[2i],
b = locus_off[2i + 1], c = locus_off[2i + 2]; locus l in [a, c) has strand 0 if l < b, else 1, and is aligned when
dist[l] < SKIPPED.  The winner w is the aligned locus with the least (dist, strand, l) — the better of a + best[2i] and
b + best[2i + 1], forward on a tie.  second = the least dist over the aligned l != w that lie elsewhere: on the other strand, or
max(start[l], start[w]) >= min(end[l], end[w]).  best2 is best with the loser's entry cleared.

fold and fold_loop return (locus u32, strand u8, dist u8, start u32, end u32, second u8, best2 u32, n_placed, n_reverse,
n_ambiguous)."""
import numpy as np

SKIPPED, NONE = 254, 255
NO_BEST = 0xFFFFFFFF


def revcomp(q, complement, sigma):
    q = np.asarray(q, np.uint8)[::-1]
    comp = np.asarray(complement, np.uint8)
    return np.where(q < sigma, comp[np.minimum(q, sigma - 1)], q).astype(np.uint8)


def double_reads(ranks, roff, complement, sigma):
    """(ranks2 u8, roff2 u64) of the doubled batch."""
    nr = len(roff) - 1
    ranks = np.asarray(ranks, np.uint8)
    parts, roff2 = [], np.zeros(2 * nr + 1, np.uint64)
    for i in range(nr):
        a, b = int(roff[i]), int(roff[i + 1])
        q = ranks[a:b]
        parts += [q, revcomp(q, complement, sigma)]
        roff2[2 * i] = 2 * a
        roff2[2 * i + 1] = 2 * a + (b - a)
    roff2[2 * nr] = 2 * int(roff[nr]) if nr else 0
    return (np.concatenate(parts) if parts else np.zeros(0, np.uint8)), roff2


def fold(locus_off, dist, start, end, best):
    """The winner from best[], the runner-up by masks over the loci of the read."""
    off = np.asarray(locus_off).astype(np.int64)
    dist = np.asarray(dist).astype(np.int64); start = np.asarray(start).astype(np.int64); end = np.asarray(end).astype(np.int64)
    best = np.asarray(best).astype(np.int64)
    nr = (off.size - 1) // 2
    locus = np.full(nr, NO_BEST, np.uint32); strand = np.full(nr, 255, np.uint8); d_out = np.full(nr, NONE, np.uint8)
    s_out = np.zeros(nr, np.uint32); e_out = np.zeros(nr, np.uint32); second = np.full(nr, 255, np.uint8)
    best2 = np.full(2 * nr, NO_BEST, np.uint32)
    for i in range(nr):
        a, b, c = off[2 * i], off[2 * i + 1], off[2 * i + 2]
        cand = [(dist[base + best[2 * i + s]], s, base + best[2 * i + s]) for s, base in ((0, a), (1, b)) if best[2 * i + s] != NO_BEST]
        if not cand:
            continue
        d, s, w = min(cand)
        locus[i], strand[i], d_out[i], s_out[i], e_out[i] = w, s, d, start[w], end[w]
        best2[2 * i + s] = best[2 * i + s]
        l = np.arange(a, c)
        elsewhere = ((l >= b) != bool(s)) | (np.maximum(start[a:c], start[w]) >= np.minimum(end[a:c], end[w]))
        rest = dist[a:c][(dist[a:c] < SKIPPED) & (l != w) & elsewhere]
        if rest.size:
            second[i] = rest.min()
    placed = strand != 255
    return (locus, strand, d_out, s_out, e_out, second, best2, int(placed.sum()), int((strand == 1).sum()), int((placed & (second == d_out)).sum()))


def fold_loop(locus_off, dist, start, end, best):
    """The same one locus at a time, the winner by (dist, strand, l) over every aligned locus: best[] is not looked at but to copy
    the winner's entry (the checker of the checker)."""
    nr = (len(locus_off) - 1) // 2
    locus, strand, d_out, s_out, e_out, second, best2 = [], [], [], [], [], [], []
    n_placed = n_reverse = n_ambiguous = 0
    for i in range(nr):
        a, b, c = int(locus_off[2 * i]), int(locus_off[2 * i + 1]), int(locus_off[2 * i + 2])
        w = None
        for l in range(a, c):
            if int(dist[l]) >= SKIPPED:
                continue
            key = (int(dist[l]), 0 if l < b else 1, l)
            if w is None or key < w:
                w = key
        if w is None:
            locus.append(NO_BEST); strand.append(255); d_out.append(NONE); s_out.append(0); e_out.append(0); second.append(255)
            best2 += [NO_BEST, NO_BEST]
            continue
        wd, ws, wl = w
        sec = 255
        for l in range(a, c):
            if int(dist[l]) >= SKIPPED or l == wl:
                continue
            other_strand = (0 if l < b else 1) != ws
            disjoint = max(int(start[l]), int(start[wl])) >= min(int(end[l]), int(end[wl]))
            if other_strand or disjoint:
                sec = min(sec, int(dist[l]))
        locus.append(wl); strand.append(ws); d_out.append(wd); s_out.append(int(start[wl])); e_out.append(int(end[wl])); second.append(sec)
        best2 += [int(best[2 * i]), NO_BEST] if ws == 0 else [NO_BEST, int(best[2 * i + 1])]
        n_placed += 1
        n_reverse += ws
        n_ambiguous += sec == wd
    return (np.asarray(locus, np.uint32), np.asarray(strand, np.uint8), np.asarray(d_out, np.uint8), np.asarray(s_out, np.uint32),
            np.asarray(e_out, np.uint32), np.asarray(second, np.uint8), np.asarray(best2, np.uint32), n_placed, n_reverse, n_ambiguous)
