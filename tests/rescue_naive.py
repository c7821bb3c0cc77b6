"""The contract of kmx_pairs_rescue in executable form (include/kmx.h, KMX_PAIR_RESCUE), on the host arrays of one chain: the text, the
doubled reads, the loci and alignments of the doubled batch, and the placements and pairs of kmx_alignments_fold_pairs.

Jobs.  Pair p has mates a (the anchor) and b = 1 - a, public reads 2p + a and 2p + b.  A job (p, b) exists when cls[p] is the ONLY
class in which a is the placed mate, or when cls[p] == DISCORDANT and `discordant` is set, then for both b.  With s_a, S_a, E_a the
anchor's strand, start and end in the placements: s_b = 1 - s_a for FR and RF, s_a for FF; the anchor is upstream iff s_a == 0 (FR),
s_a == 1 (RF), (a is mate 1) == (s_a == 0) (FF).  The job's read q is internal read 4p + 2b + s_b (m letters), its window [lo, hi):
lo = S_a, hi = min(n, S_a + max_insert) with the anchor upstream, hi = E_a, lo = max(0, E_a - max_insert) with it downstream.  Jobs
are ordered by internal read; job_off[nr2 + 1] is the exclusive prefix sum of the jobs per internal read.

Alignment.  m == 0, m > MAX_READ or m <= E: dist = SKIPPED, start = end = 0.  Otherwise d = the least Levenshtein distance between q
and any substring of text[lo:hi) (a read letter >= sigma equals nothing); d > E: dist = NONE, start = end = 0; else dist = d, end =
the smallest end of a substring at distance d, start = the largest s <= end with lev(q, text[s:end)) == d.

Choice.  A found job is concordant by pair_naive's test on the anchor's interval and [start, end) with the strands s_a, s_b; its
score is dist[anchor] + d.  An ONLY pair takes its concordant job; a DISCORDANT pair the concordant job with the least (score, b)
when score <= dist[mate 1] + dist[mate 2] + unpaired_penalty.  status: 0 skipped or none, 1 found, 2 concordant, 3 taken.  A taken
job sets cls = CONCORDANT, tlen = +-T (positive iff the upstream one is mate 1), score, second_score = 0xFFFF for the pair and, for
public read 2p + b, locus = 0xFFFFFFFF, strand = s_b, dist / start / end the job's, both best2 entries 0xFFFFFFFF and second = the
least dist over the read's aligned loci that lie elsewhere from (s_b, [start, end)) (another strand, or no letter shared), else 255.
Everything else stays, and all counters are those of the final arrays.

rescue and rescue_loop return (placements: 7 arrays as pair_naive.PLACEMENTS, pairs: 4 arrays as pair_naive.PAIRS, counters: the dict
of pair_naive.COUNTERS, jobs: (job_off u64, read u32, lo u32, hi u32, dist u8, start u32, end u32, status u8), totals: a dict with
nr2, n_jobs, n_found, n_concordant, n_taken)."""
import numpy as np

from tests import align_naive as an
from tests import pair_naive as pn

SKIPPED, NONE, NO_BEST, MAX_READ = an.SKIPPED, an.NONE, an.NO_BEST, an.MAX_READ
FR, RF, FF = pn.FR, pn.RF, pn.FF
NO_PENALTY, NO_SCORE = pn.NO_PENALTY, pn.NO_SCORE
MAX_INSERT = 65536
JOBS = ("job_off", "read", "lo", "hi", "dist", "start", "end", "status")
TOTALS = ("nr2", "n_jobs", "n_found", "n_concordant", "n_taken")
_JOB_TYPES = (np.uint32, np.uint32, np.uint32, np.uint8, np.uint32, np.uint32, np.uint8)


def align_window(text, q, lo, hi, E, sigma):
    """(dist, start, end) of read q against text[lo:hi) by the rows of align_naive"""
    if q.size == 0 or q.size > MAX_READ or q.size <= E:
        return SKIPPED, 0, 0
    t = text[lo:hi]
    row = an._last_row(q, t, sigma, False)
    j = int(np.argmin(row))
    d = int(row[j])
    if d > E:
        return NONE, 0, 0
    back = an._last_row(q[::-1], t[:j][::-1], sigma, True)
    jb = int(np.flatnonzero(back == d)[0])
    return d, lo + j - jb, lo + j


def _pack(nr2, jobs, placements, pairs):
    placements = tuple(placements)
    cls, tlen, score, second_score = pairs
    fin = pn._finish(placements, cls, tlen, score, second_score)
    job_off = np.zeros(nr2 + 1, np.uint64)
    for j in jobs:
        job_off[j[0] + 1] += 1
    job_off = np.cumsum(job_off).astype(np.uint64)
    cols = [np.asarray([j[k] for j in jobs], d) for k, d in enumerate(_JOB_TYPES)]
    status = cols[6]
    totals = dict(nr2=nr2, n_jobs=len(jobs), n_found=int((status >= 1).sum()), n_concordant=int((status >= 2).sum()), n_taken=int((status == 3).sum()))
    return fin[:7], fin[7:11], fin[11], (job_off, *cols), totals


def rescue(text, sigma, ranks2, roff2, locus_off, ldist, lstart, lend, placements, pairs, min_insert, max_insert, max_edits, orientation=FR,
           discordant=False, unpaired_penalty=NO_PENALTY):
    """The jobs as records, aligned by align_window, the `second` of a rescued read as one mask over its loci."""
    text = np.asarray(text)
    n = int(text.size)
    off = np.asarray(locus_off).astype(np.int64)
    ldist = np.asarray(ldist).astype(np.int64); lstart = np.asarray(lstart).astype(np.int64); lend = np.asarray(lend).astype(np.int64)
    locus, strand, dist, start, end, second, best2 = [np.array(a, copy=True) for a in placements]
    cls, tlen, score, second_score = [np.array(a, copy=True) for a in pairs]
    nr2 = len(roff2) - 1
    jobs = []                                                  # [read, lo, hi, dist, start, end, status]
    for p in range(nr2 // 4):
        c0 = int(cls[p])
        if c0 == pn.MATE1_ONLY:
            looked = (1,)
        elif c0 == pn.MATE2_ONLY:
            looked = (0,)
        elif c0 == pn.DISCORDANT and discordant:
            looked = (0, 1)
        else:
            continue
        cand = []
        mine = []
        for b in looked:
            a = 1 - b
            sa, Sa, Ea, da = int(strand[2 * p + a]), int(start[2 * p + a]), int(end[2 * p + a]), int(dist[2 * p + a])
            sb = sa if orientation == FF else 1 - sa
            up = sa == 0 if orientation == FR else sa == 1 if orientation == RF else (a == 0) == (sa == 0)
            lo, hi = (Sa, min(n, Sa + max_insert)) if up else (max(0, Ea - max_insert), Ea)
            r = 4 * p + 2 * b + sb
            q = np.asarray(ranks2[int(roff2[r]):int(roff2[r + 1])])
            d, s, e = align_window(text, q, lo, hi, max_edits, sigma)
            job = [r, lo, hi, d, s, e, 0]
            mine.append(job)
            if d > max_edits:
                continue
            job[6] = 1
            (us, ue), (vs, ve) = ((Sa, Ea), (s, e)) if up else ((s, e), (Sa, Ea))
            T = ve - us
            if us <= vs and ue <= ve and min_insert <= T <= max_insert:
                job[6] = 2
                first = (a == 0) == up                        # the upstream one is mate 1
                cand.append((da + d, b, T if first else -T, job))
        jobs += mine
        if not cand:
            continue
        sc, b, t, job = min(cand, key=lambda x: x[:2])
        if c0 == pn.DISCORDANT and sc > int(dist[2 * p]) + int(dist[2 * p + 1]) + int(unpaired_penalty):
            continue
        job[6] = 3
        r, _, _, d, s, e, _ = job
        i, sb = 2 * p + b, r & 1
        cls[p], tlen[p], score[p], second_score[p] = pn.CONCORDANT, t, sc, NO_SCORE
        locus[i], strand[i], dist[i], start[i], end[i] = NO_BEST, sb, d, s, e
        best2[2 * i] = best2[2 * i + 1] = NO_BEST
        l = np.arange(off[2 * i], off[2 * i + 2])
        sl = (l >= off[2 * i + 1]).astype(np.int64)
        elsewhere = (sl != sb) | (np.maximum(lstart[l], s) >= np.minimum(lend[l], e))
        rest = ldist[l][(ldist[l] < SKIPPED) & elsewhere]
        second[i] = rest.min() if rest.size else 255
    return _pack(nr2, jobs, (locus, strand, dist, start, end, second, best2), (cls, tlen, score, second_score))


def _lev(a, b, sigma):
    prev = list(range(len(b) + 1))
    for i, x in enumerate(a):
        cur = [i + 1]
        for j, y in enumerate(b):
            cur.append(min(prev[j + 1] + 1, cur[j] + 1, prev[j] + (0 if x == y and x < sigma else 1)))
        prev = cur
    return prev[-1]


def brute_window(text, q, lo, hi, E, sigma):
    """The definition itself: every substring of the window whose length differs from m by at most E (no other can lie within E
    edits), the least (distance, end, -start)."""
    m = len(q)
    if m == 0 or m > MAX_READ or m <= E:
        return SKIPPED, 0, 0
    best = None
    for e in range(lo, hi + 1):
        for s in range(max(lo, e - m - E), min(e, e - m + E) + 1):
            if s < lo:
                continue
            key = (_lev(q, [int(x) for x in text[s:e]], sigma), e, -s)
            if best is None or key < best:
                best = key
    if best is None or best[0] > E:
        return NONE, 0, 0
    return best[0], -best[2], best[1]


def rescue_loop(text, sigma, ranks2, roff2, locus_off, ldist, lstart, lend, placements, pairs, min_insert, max_insert, max_edits, orientation=FR,
                discordant=False, unpaired_penalty=NO_PENALTY):
    """The same one job at a time in Python integers, with its own Levenshtein brute force, its own concordance test by cases and the
    counters added up by hand (the checker of the checker)."""
    n = len(text)
    out_pl = [[int(v) for v in a] for a in placements]
    out_pr = [[int(v) for v in a] for a in pairs]
    locus, strand, dist, start, end, second, best2 = out_pl
    cls, tlen, score, second_score = out_pr
    nr2 = len(roff2) - 1
    jobs = []
    for r in range(nr2):
        p, b, s = r // 4, (r // 2) % 2, r % 2
        a = 1 - b
        only = cls[p] == (pn.MATE1_ONLY if a == 0 else pn.MATE2_ONLY)
        if not (only or (cls[p] == pn.DISCORDANT and discordant)):
            continue
        sa = strand[2 * p + a]
        if orientation == FR:
            sb, up = 1 - sa, sa == 0
        elif orientation == RF:
            sb, up = 1 - sa, sa == 1
        else:
            sb, up = sa, (sa == 0 and a == 0) or (sa == 1 and a == 1)
        if s != sb:
            continue
        if up:
            lo = start[2 * p + a]
            hi = min(n, lo + max_insert)
        else:
            hi = end[2 * p + a]
            lo = max(0, hi - max_insert)
        q = [int(x) for x in ranks2[int(roff2[r]):int(roff2[r + 1])]]
        d, js, je = brute_window(text, q, lo, hi, max_edits, sigma)
        jobs.append([r, lo, hi, d, js, je, 0])
    by_pair = {}
    for job in jobs:
        by_pair.setdefault(job[0] // 4, []).append(job)
    for p, mine in sorted(by_pair.items()):
        before = (cls[p], dist[2 * p], dist[2 * p + 1])
        taken = None
        for job in mine:                                       # in the order of b
            r, lo, hi, d, js, je, _ = job
            if d > max_edits:
                continue
            job[6] = 1
            b, sb = (r // 2) % 2, r % 2
            a = 1 - b
            sa, Sa, Ea = strand[2 * p + a], start[2 * p + a], end[2 * p + a]
            x, y = ((sb, js, je), (sa, Sa, Ea)) if b == 0 else ((sa, Sa, Ea), (sb, js, je))      # mate 1, mate 2
            if orientation == FF:
                if x[0] != y[0]:
                    continue
                first = x[0] == 0
            else:
                if x[0] == y[0]:
                    continue
                first = x[0] == (0 if orientation == FR else 1)
            u, v = (x, y) if first else (y, x)
            if u[1] > v[1] or u[2] > v[2]:
                continue
            t = v[2] - u[1]
            if t < min_insert or t > max_insert:
                continue
            job[6] = 2
            sc = dist[2 * p + a] + d
            if taken is None or sc < taken[0]:
                taken = (sc, b, t if first else -t, job)
        if taken is None:
            continue
        if before[0] == pn.DISCORDANT and taken[0] > before[1] + before[2] + int(unpaired_penalty):
            continue
        sc, b, t, job = taken
        job[6] = 3
        r, _, _, d, js, je, _ = job
        i, sb = 2 * p + b, r % 2
        cls[p], tlen[p], score[p], second_score[p] = pn.CONCORDANT, t, sc, NO_SCORE
        locus[i], strand[i], dist[i], start[i], end[i] = NO_BEST, sb, d, js, je
        best2[2 * i], best2[2 * i + 1] = NO_BEST, NO_BEST
        sec = 255
        for l in range(int(locus_off[2 * i]), int(locus_off[2 * i + 2])):
            if int(ldist[l]) >= SKIPPED:
                continue
            sl = 0 if l < int(locus_off[2 * i + 1]) else 1
            if sl != sb or max(int(lstart[l]), js) >= min(int(lend[l]), je):
                sec = min(sec, int(ldist[l]))
        second[i] = sec
    placed = [s != 255 for s in strand]
    counters = dict(nr=len(strand), n_placed=sum(placed), n_reverse=sum(1 for s in strand if s == 1),
                    n_ambiguous=sum(1 for i, ok in enumerate(placed) if ok and second[i] == dist[i]), np=len(cls),
                    n_concordant=sum(1 for c in cls if c == pn.CONCORDANT), n_discordant=sum(1 for c in cls if c == pn.DISCORDANT),
                    n_single=sum(1 for c in cls if c in (pn.MATE1_ONLY, pn.MATE2_ONLY)), n_unplaced=sum(1 for c in cls if c == pn.UNPLACED),
                    n_pairs_ambiguous=sum(1 for c, a, b in zip(cls, score, second_score) if c == pn.CONCORDANT and a == b))
    dt = (np.uint32, np.uint8, np.uint8, np.uint32, np.uint32, np.uint8, np.uint32)
    pl = tuple(np.asarray(a, d) for a, d in zip(out_pl, dt))
    pr = tuple(np.asarray(a, d) for a, d in zip(out_pr, (np.uint8, np.int32, np.uint16, np.uint16)))
    job_off = np.zeros(nr2 + 1, np.uint64)
    for j in jobs:
        job_off[j[0] + 1:] += 1
    cols = tuple(np.asarray([j[k] for j in jobs], d) for k, d in enumerate(_JOB_TYPES))
    status = [j[6] for j in jobs]
    totals = dict(nr2=nr2, n_jobs=len(jobs), n_found=sum(1 for s in status if s >= 1), n_concordant=sum(1 for s in status if s >= 2),
                  n_taken=sum(1 for s in status if s == 3))
    return pl, pr, counters, (job_off, *cols), totals


def forward_segmented(text, q, lo, hi, E, sigma, G):
    """What the segmented forward pass of the kernels computes, in numpy: segment g owns the end columns (lo + g G, lo + (g + 1) G],
    starts with a fresh state m + E columns earlier (clamped at lo) and reports its least score and the first end that reaches it when
    that score is <= E.  Returns the least (d, end) over the segments, or None.  G = None: one serial pass."""
    m = q.size
    best = None
    W = hi - lo
    G = max(W, 1) if G is None else G
    for g in range((W + G - 1) // G):
        c0 = lo + g * G
        c1 = min(hi, c0 + G)
        ws = max(lo, c0 - (m + E))
        row = an._last_row(q, text[ws:c1], sigma, False)       # row[j]: the score at end ws + j
        own = row[c0 + 1 - ws:]                                # the ends c0 + 1 .. c1
        j = int(np.argmin(own))
        d = int(own[j])
        if d <= E and d < m:
            key = (d, c0 + 1 + j)
            if best is None or key < best:
                best = key
    return best
