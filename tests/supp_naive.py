"""The contract of kmx_clips_supplementaries in executable form (include/kmx.h, KMX_MAP_SUPPLEMENTARY), written from the header's
text: plain Python loops over the host arrays of a doubled batch.

The parts are the best-scoring parts of the edit-optimal scripts (clip_naive), not Smith-Waterman realignments.

For public read i: m = min(roff2[2i + 1] - roff2[2i], 65535); ea, eb, ec = read_sel_off[2i], [2i + 1], [2i + 2] clamped into
[0, n_sel] and made ascending.  Entry e in [ea, ec) has strand 0 if e < eb, else 1, and the locus l = sel[e].  Its read interval is
[sl, m - sr) on strand 0 and [sr, m - sl) on strand 1; its text interval [start[l] + tl, end[l] - tr); it has runs when
cig_off[e + 1] > cig_off[e].  The primary is the least p with sel[p] == locus[i]; a read that is unplaced (strand 255) or rescued
(locus 0xFFFFFFFF), without such a p, or whose p has no runs, has no entries.  A candidate c != p has runs, no LOW bit,
sel[c] < n_loci, score >= min_score and q1 - q0 >= min_len.  ov(a, b) = max(0, min(q1) - max(q0)).  Greedy: T = {p}; among the
candidates not yet taken with ov(c, t) <= max_overlap for every t in T the greatest score, then the least e; none: more = 0; N taken
already: more = 1; else take it.  second_score[x] = the greatest score of a candidate c != x with ov(c, x) > max_overlap that lies
elsewhere from x on the text intervals (strands differ, or max(t0) >= min(t1)); 0 for none.

supplementaries() returns a dict: sup_off u64[nr + 1], ent u32, locus u32, strand u8, q0 u16, q1 u16, t0 u32, t1 u32, score i32,
second_score i32, nm u16, ctg u32 or None, more u8[nr], and the counters n_sup, n_split, n_truncated."""
import numpy as np

LOW = 1
RESCUED = 0xFFFFFFFF
MAX_READ_LOOKED_AT = 65535
SUPPLEMENTARY_MAX = 8
DEFAULTS = dict(max_supplementary=4, min_len=20, max_overlap=10, min_score=20)
ARRAYS = ("sup_off", "ent", "locus", "strand", "q0", "q1", "t0", "t1", "score", "second_score", "nm", "ctg", "more")
COUNTERS = ("n_sup", "n_split", "n_truncated")


def _clamped(read_sel_off, n_sel, i):
    ea = min(int(read_sel_off[2 * i]), n_sel)
    eb = min(max(int(read_sel_off[2 * i + 1]), ea), n_sel)
    ec = min(max(int(read_sel_off[2 * i + 2]), eb), n_sel)
    return ea, eb, ec


def _ov(a, b):
    return max(0, min(a[1], b[1]) - max(a[0], b[0]))


def supplementaries(roff2, start, end, ctg, placements_host, read_sel_off, sel, clips_host, max_supplementary=4, min_len=20, max_overlap=10,
                    min_score=20):
    """roff2: the offsets of the doubled reads; start, end (and ctg, or None): the alignments'; placements_host: Placements.host()
    (locus and strand are read); read_sel_off, sel: the all-loci scripts'; clips_host: Clips.host() of their clips."""
    p_locus, p_strand = placements_host[0], placements_host[1]
    score, sl, sr, tl, tr, nm, cflags, cig_off = clips_host[:8]
    n_sel, n_loci = len(sel), len(start)
    nr = (len(roff2) - 1) // 2
    N = int(max_supplementary)
    rows, sup_off, more = [], [0], [0] * nr
    for i in range(nr):
        m = min((int(roff2[2 * i + 1]) - int(roff2[2 * i])) % (1 << 64), MAX_READ_LOOKED_AT)
        ea, eb, ec = _clamped(read_sel_off, n_sel, i)

        def q(e):
            a, b = (int(sl[e]), int(sr[e])) if e < eb else (int(sr[e]), int(sl[e]))
            return a, m - b

        def t(e):
            l = int(sel[e])
            return int(start[l]) + int(tl[e]), int(end[l]) - int(tr[e])

        def runs(e):
            return int(cig_off[e + 1]) > int(cig_off[e])

        p = None
        if int(p_strand[i]) != 255 and int(p_locus[i]) != RESCUED:
            p = next((e for e in range(ea, ec) if int(sel[e]) == int(p_locus[i])), None)
        taken = []
        if p is not None and runs(p):
            cands = [c for c in range(ea, ec)
                     if c != p and runs(c) and not (int(cflags[c]) & LOW) and int(sel[c]) < n_loci and int(score[c]) >= min_score
                     and q(c)[1] - q(c)[0] >= min_len]
            T = [p]
            while True:
                ok = [c for c in cands if c not in T and all(_ov(q(c), q(x)) <= max_overlap for x in T)]
                if not ok:
                    break
                if len(taken) == N:
                    more[i] = 1
                    break
                pick = max(ok, key=lambda c: (int(score[c]), -c))
                taken.append(pick)
                T.append(pick)
            for x in sorted(taken):
                s_x = 0 if x < eb else 1
                rivals = [int(score[c]) for c in cands
                          if c != x and _ov(q(c), q(x)) > max_overlap
                          and ((0 if c < eb else 1) != s_x or max(t(c)[0], t(x)[0]) >= min(t(c)[1], t(x)[1]))]
                l = int(sel[x])
                rows.append((x, l, s_x, q(x)[0], q(x)[1], t(x)[0] % (1 << 32), t(x)[1] % (1 << 32), int(score[x]), max(rivals, default=0),
                             int(nm[x]), None if ctg is None else int(ctg[l])))
        sup_off.append(len(rows))
    cols = list(zip(*rows)) if rows else [[] for _ in range(11)]
    dtypes = (np.uint32, np.uint32, np.uint8, np.uint16, np.uint16, np.uint32, np.uint32, np.int32, np.int32, np.uint16)
    out = dict(sup_off=np.asarray(sup_off, np.uint64), more=np.asarray(more, np.uint8))
    for name, col, dt in zip(ARRAYS[1:11], cols, dtypes):
        out[name] = np.asarray(col, dt)
    out["ctg"] = None if ctg is None else np.asarray(cols[10], np.uint32)
    out.update(n_sup=len(rows), n_split=sum(1 for a, b in zip(sup_off[:-1], sup_off[1:]) if b > a), n_truncated=int(sum(more)))
    return out


def mapq(score, second_score, cap=60):
    """0 where second_score >= score, else min(cap, cap (score - second_score) // score): a stated gap rule, not a calibrated one."""
    return [0 if int(b) >= int(a) else min(cap, cap * (int(a) - int(b)) // int(a)) for a, b in zip(score, second_score)]
