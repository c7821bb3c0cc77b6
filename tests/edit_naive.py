"""Independent checker of the edit-distance search (kmx_search_approx with KMX_APPROX_EDIT): plain numpy, no product code.
edit_naive is validated against brute_force, the definition itself, in tests/test_edit_cpu.py."""
import numpy as np


def edit_naive(text, q, e):
    """(positions u32, distances u8, lengths u32) by the definition in the issue."""
    n, m = int(text.size), int(q.size)
    z = (np.zeros(0, np.uint32), np.zeros(0, np.uint8), np.zeros(0, np.uint32))
    if m == 0 or m <= e:
        return z
    # free-start distance on the reversed strings: E[i][j] = min over s of ed(qr[:i], tr[s:j]); S[p] = E[m][n - p]
    tr, qr = text[::-1], q[::-1]
    j = np.arange(n + 1, dtype=np.int64)
    prev = np.zeros(n + 1, np.int64)
    for i in range(1, m + 1):
        x = np.empty(n + 1, np.int64)
        x[0] = i
        x[1:] = np.minimum(prev[:-1] + (tr != qr[i - 1]), prev[1:] + 1)
        prev = np.minimum.accumulate(x - j) + j            # min over j' <= j of x[j'] + (j - j')
    S = prev[::-1]                                         # S[p], p = 0 .. n
    p = np.nonzero(S[:n] <= e)[0]
    if p.size == 0:
        return z
    # lengths: forward pass of q against text[p : p + m + e] for every reported p at once
    W = m + e
    idx = p[:, None] + np.arange(W)[None, :]
    win = np.where(idx < n, text[np.minimum(idx, n - 1)], 255).astype(np.int64)   # 255: outside the text
    c = np.arange(W + 1, dtype=np.int64)
    row = np.tile(c, (p.size, 1))
    for i in range(1, m + 1):
        x = np.empty_like(row)
        x[:, 0] = i
        x[:, 1:] = np.minimum(row[:, :-1] + (win != int(q[i - 1])), row[:, 1:] + 1)
        row = np.minimum.accumulate(x - c, axis=1) + c
    big = 1 << 30
    row = np.where((p[:, None] + c[None, :] <= n) & (c[None, :] >= 1), row, big)
    d = row.min(axis=1)
    assert np.array_equal(d, S[p]), "the two passes disagree"
    key = np.where(row == d[:, None], np.abs(c - m)[None, :] * 2 * (W + 2) + c[None, :], big)
    return p.astype(np.uint32), d.astype(np.uint8), key.argmin(axis=1).astype(np.uint32)


def brute_force(text, q, e):
    """[(p, d, L)] straight from the definition, plain Python lists (tiny texts: checks the checker)."""
    def lev(a, b):
        prev = list(range(len(b) + 1))
        for i in range(1, len(a) + 1):
            cur = [i] + [0] * len(b)
            for k in range(1, len(b) + 1):
                cur[k] = min(prev[k - 1] + (a[i - 1] != b[k - 1]), prev[k] + 1, cur[k - 1] + 1)
            prev = cur
        return prev[-1]
    n, m, out = len(text), len(q), []
    if m == 0 or m <= e:
        return out
    for p in range(n):
        best = None
        for L in range(max(1, m - e), min(m + e, n - p) + 1):
            dd = lev(q, text[p:p + L])
            if dd <= e and (best is None or (dd, abs(L - m), L) < best):
                best = (dd, abs(L - m), L)
        if best:
            out.append((p, best[0], best[2]))
    return out


def compare_batch(text, qranks, qoff, e, hit_off, positions, distances, lengths, status, ok=0):
    """Asserts every query with status `ok` against edit_naive (positions, distances and lengths equal); returns how many
    were checked."""
    assert hit_off[0] == 0 and np.all(np.diff(hit_off.astype(np.int64)) >= 0)
    assert positions.size == distances.size == lengths.size == int(hit_off[-1])
    checked = 0
    for i in range(qoff.size - 1):
        a, b = int(hit_off[i]), int(hit_off[i + 1])
        if status[i] != ok:
            assert a == b, f"query {i}: status {status[i]} with hits"
            continue
        q = qranks[int(qoff[i]):int(qoff[i + 1])]
        p_ref, d_ref, l_ref = edit_naive(text, q, e)
        got = positions[a:b]
        assert np.all(np.diff(got.astype(np.int64)) > 0), f"query {i}: positions not strictly ascending"
        assert np.array_equal(got, p_ref), f"query {i} (m={q.size}, e={e}): {got.size} hits, checker {p_ref.size}"
        assert np.array_equal(distances[a:b], d_ref), f"query {i} (m={q.size}, e={e}): distances differ"
        assert np.array_equal(lengths[a:b], l_ref), f"query {i} (m={q.size}, e={e}): lengths differ"
        checked += 1
    return checked
