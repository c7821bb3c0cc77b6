"""The contract of kmx_search_windows in executable form: the batch of windows written out as separate queries.

Read r of len_r letters holds c_r = 0 windows when len_r < w, else (len_r - w) // stride + 1; window j of read r is
ranks[roff[r] + j * stride, + w) and query win_off[r] + j, win_off being the exclusive prefix sum of c_r.  A windows search
returns array for array what kmx_search_batch returns for (qranks, qoff) below."""
import numpy as np


def window_counts(roff, w, stride):
    lens = np.diff(np.asarray(roff, np.uint64).astype(np.int64))
    return np.where(lens < w, 0, (lens - w) // stride + 1).astype(np.int64)


def expand(ranks, roff, w, stride):
    """(qranks[nq * w] u8, qoff[nq + 1] u64, win_off[nr + 1] u64) of the windows of a batch of reads."""
    ranks = np.asarray(ranks, np.uint8)
    roff = np.asarray(roff, np.uint64).astype(np.int64)
    c = window_counts(roff, w, stride)
    win_off = np.zeros(c.size + 1, np.int64)
    win_off[1:] = np.cumsum(c)
    nq = int(win_off[-1])
    read = np.repeat(np.arange(c.size, dtype=np.int64), c)              # the read of every window
    j = np.arange(nq, dtype=np.int64) - win_off[read]                   # ... and its number inside that read
    start = roff[read] + j * stride
    qranks = ranks[(start[:, None] + np.arange(w, dtype=np.int64)[None, :]).reshape(-1)] if nq else np.zeros(0, np.uint8)
    qoff = (np.arange(nq + 1, dtype=np.int64) * w).astype(np.uint64)
    return qranks, qoff, win_off.astype(np.uint64)


def expand_loop(ranks, roff, w, stride):
    """The same by the plainest loop there is (the checker of the checker)."""
    qs, win_off = [], [0]
    for r in range(len(roff) - 1):
        a, b = int(roff[r]), int(roff[r + 1])
        s = a
        while s + w <= b:
            qs.append(np.asarray(ranks[s:s + w], np.uint8))
            s += stride
        win_off.append(len(qs))
    qranks = np.concatenate(qs) if qs else np.zeros(0, np.uint8)
    qoff = (np.arange(len(qs) + 1) * w).astype(np.uint64)
    return qranks, qoff, np.asarray(win_off, np.uint64)
