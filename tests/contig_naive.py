"""The contract of the contig table in the mapping chain in executable form (include/kmx.h, KMX_MAP_CONTIGS), built from the naive
modules of the stages it changes: no alignment code of its own.

Contig c is text[ctg_off[c]:ctg_off[c + 1]).  Everything in Python integers.

contig_of    c(l) of a locus that is not skipped: the contig that contains mid = clamp(D + (S + m) // 2, 0, n - 1).
align        align_naive.align_one per locus on the contig's letters alone with diagonal D - ctg_off[c], shifted back by ctg_off[c];
             skipped loci as in align_naive.  Also returns ctg[n_loci] (0xFFFFFFFF for a skipped locus).
fold_pairs   pair_naive.fold_pairs on coordinates with contig c shifted by c * 2^32: a pair across contigs then fails the order test
             or the insert bound (max_insert < 2^31), differences inside a contig are unchanged.  start / end come back unshifted.
rescue       rescue_naive.rescue on a SPREAD text: the contigs separated by max_insert + 1 letters of value sigma, which equals no read
             letter, so that the plain window of rescue_naive cannot reach a letter of the next contig.  Coordinates go there and
             back; lo / hi of a job are mapped back and cut to the contig (the padding belongs to none).
locate       (ctg, pos, n_located, n_mismatched) of kmx_placements_locate."""
import numpy as np

from tests import align_naive as an
from tests import pair_naive as pn
from tests import rescue_naive as rn

NO_CONTIG = 0xFFFFFFFF
SHIFT = 1 << 32


def contig_of(ctg_off, n, D, S, m):
    mid = min(max(int(D) + (int(S) + int(m)) // 2, 0), int(n) - 1)
    off = [int(v) for v in ctg_off]
    c = 0
    while c + 1 < len(off) - 1 and off[c + 1] <= mid:
        c += 1
    return c


def window(ctg_off, c, m, D, S, E):
    """[lo, hi) of kmx.h, from the formula itself"""
    b0, b1 = int(ctg_off[c]), int(ctg_off[c + 1])
    lo = min(max(b0, D - E), b1)
    return lo, max(lo, min(b1, D + S + m + E))


def align(text, ctg_off, ranks, roff, locus_off, diag, span, E, max_span, sigma, one=an.align_one):
    """(dist u8, start u32, end u32, best u32, aligned u32, ctg u32)"""
    text = np.asarray(text)
    n = int(text.size)
    seen = []                                                  # c(l) of the loci that are not skipped, in order

    def on_contig(_, q, D, S, E_, sigma_):
        c = contig_of(ctg_off, n, D, S, q.size)
        seen.append(c)
        b0, b1 = int(ctg_off[c]), int(ctg_off[c + 1])
        d, s, e = one(text[b0:b1], q, D - b0, S, E_, sigma_)
        return (d, s + b0, e + b0) if d <= E_ else (d, 0, 0)

    res = an._run(on_contig, text, ranks, roff, locus_off, diag, span, E, max_span, sigma)   # calls it for exactly those loci
    ctg = np.full(len(diag), NO_CONTIG, np.uint32)
    ctg[res[0] != an.SKIPPED] = seen
    return (*res, ctg)


def fold_pairs(locus_off, dist, start, end, best, ctg, min_insert, max_insert, orientation, unpaired_penalty=pn.NO_PENALTY):
    """pair_naive.fold_pairs under the contig rule; the tuple of pair_naive.fold_pairs.  Intervals of different contigs are disjoint
    with and without the shift (no alignment contains a junction), so `second` and the runner-up rule see the same overlaps."""
    assert max_insert < (1 << 31)
    start = np.asarray(start).astype(np.int64); end = np.asarray(end).astype(np.int64)
    c = np.asarray(ctg).astype(np.int64)
    c = np.where(c == NO_CONTIG, 0, c)
    out = list(pn.fold_pairs(locus_off, dist, start + c * SHIFT, end + c * SHIFT, best, min_insert, max_insert, orientation, unpaired_penalty))
    # the placements' intervals are those of the chosen loci: taken from the unshifted arrays (the naive folds narrow theirs to u32)
    locus, placed = out[0].astype(np.int64), out[1] != 255
    for k, arr in ((3, start), (4, end)):
        v = np.zeros(locus.size, np.uint32)
        v[placed] = arr[locus[placed]]
        out[k] = v
    return tuple(out)


def spread(text, ctg_off, gap, sigma):
    """(spread text, add[nc]): contig c starts at ctg_off[c] + add[c] of the spread text; `gap` letters of value sigma between contigs"""
    text = np.asarray(text, np.uint8)
    nc = len(ctg_off) - 1
    add = np.arange(nc, dtype=np.int64) * gap
    parts = []
    for c in range(nc):
        if c:
            parts.append(np.full(gap, sigma, np.uint8))
        parts.append(text[int(ctg_off[c]):int(ctg_off[c + 1])])
    return (np.concatenate(parts) if parts else text), add


def rescue_window(ctg_off, c, up, Sa, Ea, max_insert):
    """[lo, hi) of a job whose anchor [Sa, Ea) lies in contig c: the clamped formula of kmx.h"""
    b0, b1 = int(ctg_off[c]), int(ctg_off[c + 1])
    if up:
        lo = min(max(Sa, b0), b1)
        return lo, min(b1, lo + max_insert)
    hi = max(min(Ea, b1), b0)
    return max(b0, hi - max_insert), hi


def rescue(text, ctg_off, ctg, sigma, ranks2, roff2, locus_off, ldist, lstart, lend, placements, pairs, min_insert, max_insert, max_edits,
           orientation=rn.FR, discordant=False, unpaired_penalty=rn.NO_PENALTY):
    """rescue_naive.rescue on the spread text, mapped back.  ctg: the contig of every locus (the alignments').  Every anchor is placed
    by a locus.  Returns the tuple of rescue_naive.rescue."""
    assert sigma < 255
    off = np.asarray(ctg_off).astype(np.int64)
    gap = int(max_insert) + 1
    wide, add = spread(text, off, gap, sigma)
    lc = np.asarray(ctg).astype(np.int64)
    ladd = np.where(lc == NO_CONTIG, 0, add[np.where(lc == NO_CONTIG, 0, lc)])
    locus, strand, dist, start, end, second, best2 = [np.array(a, copy=True) for a in placements]
    placed = strand != 255
    assert (locus[placed] != an.NO_BEST).all(), "an anchor is always placed by a locus"
    padd = np.zeros(strand.size, np.int64)
    padd[placed] = ladd[locus[placed]]
    # the spread coordinates may pass 2^32 only for texts far beyond a test's: assert it
    assert wide.size < (1 << 32)
    pl_w = (locus, strand, dist, (start.astype(np.int64) + padd).astype(np.uint32), (end.astype(np.int64) + padd).astype(np.uint32), second, best2)
    pl, pr, counters, jobs, totals = rn.rescue(wide, sigma, ranks2, roff2, locus_off, ldist, np.asarray(lstart).astype(np.int64) + ladd,
                                               np.asarray(lend).astype(np.int64) + ladd, pl_w, pairs, min_insert, max_insert, max_edits, orientation,
                                               discordant, unpaired_penalty)
    # back: a job lies in its anchor's contig, a rescued read too
    job_off, read, lo, hi, jd, js, je, status = [np.array(a, copy=True) for a in jobs]
    lo = lo.astype(np.int64); hi = hi.astype(np.int64); js = js.astype(np.int64); je = je.astype(np.int64)
    pl = [np.array(a, copy=True) for a in pl]
    new_start = pl[3].astype(np.int64); new_end = pl[4].astype(np.int64)
    now_placed = pl[1] != 255
    for j in range(read.size):
        r = int(read[j])
        p, b = r // 4, (r // 2) % 2
        anchor = 2 * p + (1 - b)
        a = int(padd[anchor])
        c = int(lc[int(locus[anchor])])
        b0, b1 = int(off[c]), int(off[c + 1])
        lo[j] = min(max(lo[j] - a, b0), b1)                    # the padding belongs to no contig
        hi[j] = min(max(hi[j] - a, b0), b1)
        if jd[j] <= max_edits:
            js[j] -= a
            je[j] -= a
            assert b0 <= js[j] <= je[j] <= b1, "an alignment that touches the padding: it equals no read letter"
        if status[j] == 3:
            i = 2 * p + b
            new_start[i] -= a
            new_end[i] -= a
            padd[i] = 0                                        # (already mapped back)
    keep = now_placed & (pl[0] != an.NO_BEST)
    new_start[keep] -= padd[keep]
    new_end[keep] -= padd[keep]
    pl[3], pl[4] = new_start.astype(np.uint32), new_end.astype(np.uint32)
    jobs = (job_off, read, lo.astype(np.uint32), hi.astype(np.uint32), jd, js.astype(np.uint32), je.astype(np.uint32), status)
    return tuple(pl), pr, counters, jobs, totals


def locate(ctg_off, lctg, locus, strand, start, mates=False):
    """(ctg u32, pos u32, n_located, n_mismatched) of kmx_placements_locate, from the placements' host arrays"""
    off = [int(v) for v in ctg_off]
    nc, nl, nr = len(off) - 1, len(lctg), len(strand)
    ctg = np.full(nr, NO_CONTIG, np.uint32); pos = np.zeros(nr, np.uint32)
    n_located = n_mismatched = 0
    for i in range(nr):
        if strand[i] == 255:
            continue
        l = int(locus[i])
        if l == an.NO_BEST and mates and strand[i ^ 1] != 255:
            l = int(locus[i ^ 1])
        ok = False
        if l < nl:
            c = int(lctg[l])
            if c < nc and off[c] <= int(start[i]) <= off[c + 1]:
                ctg[i], pos[i], ok = c, int(start[i]) - off[c], True
        n_located += ok
        n_mismatched += not ok
    return ctg, pos, n_located, n_mismatched
