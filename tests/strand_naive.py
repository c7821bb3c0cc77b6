"""Independent checker of the both-strand search (kmx_search_approx_strands): plain numpy, no product code.  The existing
checkers (approx_naive, edit_naive) on the query and on its reverse complement, the two lists merged by (position, strand).
strand_naive is validated against brute-force loops in tests/test_strands_cpu.py."""
import numpy as np

from tests.approx_naive import approx_naive
from tests.edit_naive import edit_naive


def revcomp(q, complement):
    """rc(q)[i] = complement[q[m - 1 - i]]"""
    return np.asarray(complement, np.uint8)[np.asarray(q, np.uint8)[::-1]]


def strand_naive(text, q, e, complement, edit=False):
    """(positions u32, strands u8, distances u8, lengths u32 or None) ordered by (position, strand)."""
    parts = []
    for strand, query in enumerate((np.asarray(q, np.uint8), revcomp(q, complement))):
        if edit:
            p, d, length = edit_naive(text, query, e)
        else:
            p, d = approx_naive(text, query, e)
            length = np.zeros(p.size, np.uint32)
        parts.append((p, np.full(p.size, strand, np.uint8), d, length))
    p, s, d, length = (np.concatenate([a[k] for a in parts]) for k in range(4))
    order = np.lexsort((s, p))                     # by position, the forward hit of an offset in front of the reverse one
    return p[order], s[order], d[order], (length[order] if edit else None)


def compare_batch(text, qranks, qoff, e, complement, hit_off, positions, strands, distances, lengths, status, edit=False, ok=0):
    """Asserts every query with status `ok` against strand_naive: positions, strands, distances and (edit) lengths equal and
    strictly ascending in (position, strand); every other query without hits.  Returns how many were checked."""
    assert hit_off[0] == 0 and np.all(np.diff(hit_off.astype(np.int64)) >= 0)
    assert positions.size == strands.size == distances.size == int(hit_off[-1])
    assert (lengths is not None) == edit and (not edit or lengths.size == positions.size)
    assert np.all(strands <= 1)
    checked = 0
    for i in range(qoff.size - 1):
        a, b = int(hit_off[i]), int(hit_off[i + 1])
        if status[i] != ok:
            assert a == b, f"query {i}: status {status[i]} with hits"
            continue
        q = qranks[int(qoff[i]):int(qoff[i + 1])]
        p_ref, s_ref, d_ref, l_ref = strand_naive(text, q, e, complement, edit)
        key = positions[a:b].astype(np.int64) * 2 + strands[a:b]
        assert np.all(np.diff(key) > 0), f"query {i}: hits not strictly ascending in (position, strand)"
        assert np.array_equal(positions[a:b], p_ref), f"query {i} (m={q.size}, e={e}): {b - a} hits, checker {p_ref.size}"
        assert np.array_equal(strands[a:b], s_ref), f"query {i} (m={q.size}, e={e}): strands differ"
        assert np.array_equal(distances[a:b], d_ref), f"query {i} (m={q.size}, e={e}): distances differ"
        if edit:
            assert np.array_equal(lengths[a:b], l_ref), f"query {i} (m={q.size}, e={e}): lengths differ"
        checked += 1
    return checked
