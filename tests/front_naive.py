"""The contract of kmx_search_windows in executable form, from the text alone: no index, no engine.

Read r of len_r letters holds c_r = 0 windows when len_r < w, else (len_r - w) // stride + 1; window j of read r is
ranks[roff[r] + j * stride, + w) and query win_off[r] + j, win_off being the exclusive prefix sum of c_r.  A window that holds a
letter >= sigma has no hits and the status Q_BAD_RANK; every other window has the status Q_OK and as its hits the positions p with
text[p:p + w] equal to it, ascending.  A text k-mer that holds a letter >= sigma is nobody's hit.

hits() takes the k-mer codes of the text (base sigma, in int64: sigma ** w must stay below 2^63), a stable argsort of them (so that
every hit list comes out ascending) and two binary searches per window; hits_loop() is the definition itself, window by window
against every text position (the checker of the checker).  Both return (win_off[nr + 1] u64, hit_off[nq + 1] u64, positions u32,
status[nq] u8)."""
import numpy as np

Q_OK, Q_BAD_RANK = 0, 4


def _codes(letters, sigma, w):
    """(code i64, bad bool) of the w-mer at every offset 0 .. len - w of `letters`; bad: it holds a letter >= sigma"""
    letters = np.asarray(letters, np.uint8)
    n = letters.size - w + 1
    if n <= 0:
        return np.zeros(0, np.int64), np.zeros(0, bool)
    assert float(sigma) ** w < 2.0 ** 63
    ok = letters < sigma
    x = np.where(ok, letters, 0).astype(np.int64)
    code = np.zeros(n, np.int64)
    for j in range(w):
        code = code * sigma + x[j:j + n]
    n_bad = np.zeros(letters.size + 1, np.int64)
    n_bad[1:] = np.cumsum(~ok)
    return code, (n_bad[w:w + n] - n_bad[:n]) > 0


def window_starts(roff, w, stride):
    """(win_off i64[nr + 1], start i64[nq]): the offset into ranks of every window"""
    roff = np.asarray(roff, np.uint64).astype(np.int64)
    lens = np.diff(roff)
    c = np.where(lens < w, 0, (lens - w) // stride + 1)
    win_off = np.zeros(c.size + 1, np.int64)
    win_off[1:] = np.cumsum(c)
    read = np.repeat(np.arange(c.size, dtype=np.int64), c)
    j = np.arange(int(win_off[-1]), dtype=np.int64) - win_off[read]
    return win_off, roff[read] + j * stride


def hits(text, sigma, ranks, roff, w, stride):
    t_code, t_bad = _codes(text, sigma, w)
    at = np.flatnonzero(~t_bad)
    order = at[np.argsort(t_code[at], kind="stable")]
    keys = t_code[order]
    win_off, start = window_starts(roff, w, stride)
    r_code, r_bad = _codes(ranks, sigma, w)
    code, bad = r_code[start], r_bad[start]
    lo = np.searchsorted(keys, code, "left")
    cnt = np.where(bad, 0, np.searchsorted(keys, code, "right") - lo)
    hit_off = np.zeros(cnt.size + 1, np.int64)
    hit_off[1:] = np.cumsum(cnt)
    within = np.arange(int(hit_off[-1]), dtype=np.int64) - np.repeat(hit_off[:-1], cnt)
    positions = order[np.repeat(lo, cnt) + within].astype(np.uint32)
    status = np.where(bad, Q_BAD_RANK, Q_OK).astype(np.uint8)
    return win_off.astype(np.uint64), hit_off.astype(np.uint64), positions, status


def hits_loop(text, sigma, ranks, roff, w, stride):
    text = [int(x) for x in text]
    win_off, hit_off, positions, status = [0], [0], [], []
    for r in range(len(roff) - 1):
        a, b = int(roff[r]), int(roff[r + 1])
        s = a
        while s + w <= b:
            q = [int(x) for x in ranks[s:s + w]]
            if max(q) >= sigma:
                status.append(Q_BAD_RANK)
            else:
                status.append(Q_OK)
                positions += [p for p in range(len(text) - w + 1) if text[p:p + w] == q]
            hit_off.append(len(positions))
            s += stride
        win_off.append(len(status))
    return np.asarray(win_off, np.uint64), np.asarray(hit_off, np.uint64), np.asarray(positions, np.uint32), np.asarray(status, np.uint8)
