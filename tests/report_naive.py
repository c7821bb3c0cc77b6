"""Independent checker of the reporting options of kmx_search_approx_opts (KMX_APPROX_LOCI, KMX_APPROX_BEST, max_hits): plain
numpy and Python loops, no product code.  The three rules of include/kmx.h applied, as literally as the contract states them,
to H(q) as the existing checkers give it (approx_naive, edit_naive, strand_naive).  A hit is a tuple (p, strand, d, L); L is 0
for Hamming hits, strand 0 throughout for one strand.  Validated in tests/test_report_cpu.py."""
import numpy as np

from tests.approx_naive import approx_naive
from tests.edit_naive import edit_naive
from tests.strand_naive import strand_naive


def hits_naive(text, q, e, edit=False, complement=None):
    """H(q) as a list of (p, strand, d, L) in (p, strand) order."""
    if complement is not None:
        p, s, d, length = strand_naive(text, q, e, complement, edit)
    elif edit:
        p, d, length = edit_naive(text, q, e)
        s = np.zeros(p.size, np.uint8)
    else:
        p, d = approx_naive(text, q, e)
        s, length = np.zeros(p.size, np.uint8), None
    if length is None:
        length = np.zeros(p.size, np.uint32)
    return list(zip(p.tolist(), s.tolist(), d.tolist(), length.tolist()))


def loci(H, e):
    """Step 1: (p, s, d) survives unless H holds (p', s, d') with p' != p, |p' - p| <= e and (d', p') < (d, p)."""
    out = []
    for (p, s, d, length) in H:
        dead = False
        for (p2, s2, d2, _) in H:
            if s2 == s and p2 != p and abs(p2 - p) <= e and (d2, p2) < (d, p):
                dead = True
        if not dead:
            out.append((p, s, d, length))
    return out


def best(H):
    """Step 2: the hits whose d is the least d of the list."""
    if not H:
        return []
    least = min(h[2] for h in H)
    return [h for h in H if h[2] == least]


def cap(H, max_hits):
    """Step 3: (found, kept): the first max_hits hits in (d, p, strand) order, reported in (p, strand) order."""
    found = len(H)
    if max_hits and found > max_hits:
        first = sorted(H, key=lambda h: (h[2], h[0], h[1]))[:max_hits]
        H = sorted(first, key=lambda h: (h[0], h[1]))
    return found, H


def report_naive(H, e, use_loci=False, use_best=False, max_hits=0):
    """(found, kept) of one query's H(q) under the three steps, in their order."""
    if use_loci:
        H = loci(H, e)
    if use_best:
        H = best(H)
    return cap(H, max_hits)


def reference(text, qranks, qoff, e, edit=False, complement=None):
    """Per query (H(q), loci(H(q), e)): what compare_batch takes as `ref`, so that tests sharing a batch compute it once."""
    out = []
    for i in range(qoff.size - 1):
        H = hits_naive(text, qranks[int(qoff[i]):int(qoff[i + 1])], e, edit, complement)
        out.append((H, loci(H, e)))
    return out


def compare_batch(text, qranks, qoff, e, hit_off, positions, strands, distances, lengths, status, found, edit=False, complement=None,
                  use_loci=False, use_best=False, max_hits=0, ok=0, ref=None):
    """Asserts every query with status `ok` against report_naive of hits_naive: positions, strands (None for one strand),
    distances, lengths (None for Hamming) and found equal; every other query without hits and with found 0.  ref: the value
    of reference() for the same batch (computed here when None).  Returns (queries checked, hits LOCI removed, hits BEST
    removed, queries the cap cut)."""
    nq = qoff.size - 1
    assert hit_off.size == nq + 1 and hit_off[0] == 0 and np.all(np.diff(hit_off.astype(np.int64)) >= 0)
    assert positions.size == distances.size == int(hit_off[-1]) and found.size == nq and status.size == nq
    assert (strands is not None) == (complement is not None) and (strands is None or strands.size == positions.size)
    assert (lengths is not None) == edit and (not edit or lengths.size == positions.size)
    checked = by_loci = by_best = cut = 0
    for i in range(nq):
        a, b = int(hit_off[i]), int(hit_off[i + 1])
        if status[i] != ok:
            assert a == b and found[i] == 0, f"query {i}: status {status[i]} with hits"
            continue
        q = qranks[int(qoff[i]):int(qoff[i + 1])]
        H, HL = ref[i] if ref is not None else (hits_naive(text, q, e, edit, complement), None)
        H1 = (HL if HL is not None else loci(H, e)) if use_loci else H
        H2 = best(H1) if use_best else H1
        want_found, want = cap(H2, max_hits)
        by_loci += len(H) - len(H1)
        by_best += len(H1) - len(H2)
        cut += want_found > len(want)
        got = list(zip(positions[a:b].tolist(), strands[a:b].tolist() if strands is not None else [0] * (b - a), distances[a:b].tolist(),
                       lengths[a:b].tolist() if edit else [0] * (b - a)))
        assert all(x[:2] < y[:2] for x, y in zip(got, got[1:])), f"query {i}: hits not strictly ascending in (position, strand)"
        assert got == want, f"query {i} (m={q.size}, e={e}): {len(got)} hits, checker {len(want)} of {len(H)}"
        assert int(found[i]) == want_found, f"query {i}: found {int(found[i])}, checker {want_found}"
        checked += 1
    return checked, by_loci, by_best, cut
