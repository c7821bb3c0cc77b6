"""The contract of kmx_windows_vote in executable form, on the four host arrays of a windows result.

Window j of read r (query win_off[r] + j of the result) lies at read offset o = j * stride.  It votes when it has hits and
(max_occ == 0 or at most max_occ of them); a window with hits that does not vote is counted in skipped[r].  Every hit p of a
voting window is one vote on the diagonal D = p - o.  A read's votes sorted by D fall into loci, maximal runs in which each D is
at most `band` above the one before it: diag = the smallest D, span = largest - smallest, votes = their number.  The loci with
votes >= min_votes are reported per read in ascending diag.

Both functions return (locus_off[nr + 1] u64, diag i64, span u32, votes u32, skipped[nr] u32, n_votes)."""
import numpy as np


def vote(hit_off, positions, win_off, stride, band, min_votes, max_occ):
    hit_off = hit_off.astype(np.int64); win_off = win_off.astype(np.int64); pos = positions.astype(np.int64)
    nr = win_off.size - 1
    cnt = np.diff(hit_off); read_of_w = np.repeat(np.arange(nr), np.diff(win_off))
    j = np.arange(win_off[-1]) - win_off[read_of_w]
    use = (cnt > 0) & ((max_occ == 0) | (cnt <= max_occ))
    skipped = np.bincount(read_of_w[(cnt > 0) & ~use], minlength=nr).astype(np.uint32)
    wv = np.repeat(np.arange(cnt.size), np.where(use, cnt, 0))
    d = pos[np.repeat(use, cnt)] - j[wv] * stride; r = read_of_w[wv]
    empty = (np.zeros(nr + 1, np.uint64), np.zeros(0, np.int64), np.zeros(0, np.uint32), np.zeros(0, np.uint32), skipped, 0)
    if d.size == 0: return empty
    o = np.lexsort((d, r)); d = d[o]; r = r[o]
    head = np.ones(d.size, bool); head[1:] = (r[1:] != r[:-1]) | (d[1:] - d[:-1] > band)
    hs = np.flatnonzero(head); ends = np.append(hs[1:], d.size)
    votes = ends - hs; k = votes >= min_votes
    off = np.zeros(nr + 1, np.uint64); off[1:] = np.cumsum(np.bincount(r[hs][k], minlength=nr))
    return off, d[hs][k], (d[ends - 1] - d[hs])[k].astype(np.uint32), votes[k].astype(np.uint32), skipped, d.size


def vote_loop(hit_off, positions, win_off, stride, band, min_votes, max_occ):
    """The same one read at a time, with a Python sorted() (the checker of the checker)."""
    nr = len(win_off) - 1
    off, diag, span, votes, skipped, n_votes = [0], [], [], [], [], 0
    for r in range(nr):
        ds, sk = [], 0
        for j, q in enumerate(range(int(win_off[r]), int(win_off[r + 1]))):
            hits = [int(p) for p in positions[int(hit_off[q]):int(hit_off[q + 1])]]
            if not hits:
                continue
            if max_occ != 0 and len(hits) > max_occ:
                sk += 1
                continue
            ds += [p - j * stride for p in hits]
        skipped.append(sk)
        n_votes += len(ds)
        ds = sorted(ds)
        loci = []                                             # [first diagonal, last diagonal, votes]
        for d in ds:
            if loci and d - loci[-1][1] <= band:
                loci[-1][1] = d
                loci[-1][2] += 1
            else:
                loci.append([d, d, 1])
        for a, b, c in loci:
            if c >= min_votes:
                diag.append(a); span.append(b - a); votes.append(c)
        off.append(len(diag))
    return (np.asarray(off, np.uint64), np.asarray(diag, np.int64), np.asarray(span, np.uint32), np.asarray(votes, np.uint32),
            np.asarray(skipped, np.uint32), n_votes)
