"""What tests/test_report_gpu.py shares with the child process of its chunking test: the text with twenty near-copies of one unit,
the planted reads of a grid cell with the checker's reference, and kmx_search_approx_opts called directly."""
import ctypes as C
import functools

import numpy as np

from kmer_index_amd import synth
from tests.report_naive import reference
from tests.strand_naive import revcomp

DNA4 = np.array([3, 2, 1, 0], np.uint8)
NQ, M = 40, 24


def fixture_text(seed=3, rc_copies=False):
    """500 random letters, 20 copies of one 200-letter unit with 6 letters (3 %) of each substituted, 500 random letters:
    n = 5000.  rc_copies: every other copy reverse-complemented (reads then hit both strands)."""
    rng = np.random.default_rng(seed)
    unit = rng.integers(0, 4, 200).astype(np.uint8)
    parts = [rng.integers(0, 4, 500).astype(np.uint8)]
    for c in range(20):
        u = unit.copy()
        at = rng.choice(200, 6, replace=False)
        u[at] = (u[at] + rng.integers(1, 4, 6)) % 4
        parts.append(revcomp(u, DNA4) if rc_copies and c % 2 else u.astype(np.uint8))
    parts.append(rng.integers(0, 4, 500).astype(np.uint8))
    text = np.concatenate(parts)
    assert text.size == 5000, text.size
    return text


@functools.lru_cache(maxsize=None)
def fixture_batch(edit, strands, e, rc_copies=False):
    """(text, qranks, qoff, complement or None, reference): the planted reads of one grid cell and the checker's H(q) and
    loci(H(q)) for them, computed once and shared (nothing modifies them)."""
    text = fixture_text(rc_copies=rc_copies)
    if strands:
        gen = synth.planted_reads_edit_strands if edit else synth.planted_reads_strands
        q, off = gen(100 + e, text, NQ, M, 4, e, DNA4)[:2]
    else:
        q, off = (synth.planted_reads_edit if edit else synth.planted_reads)(100 + e, text, NQ, M, 4, e)[:2]
    comp = DNA4 if strands else None
    return text, q, off, comp, reference(text, q, off, e, edit, comp)


def opts_search(engine, idx, qranks, qoff, e, edit=False, comp=None, loci=False, best=False, max_hits=0):
    """kmx_search_approx_opts called directly (also with no option set, which Index.search_approx routes to the older entry
    points): dict of hit_off, pos, strands or None, dist, lens or None, status, found, counts."""
    qranks = np.ascontiguousarray(qranks, np.uint8)
    qoff = np.ascontiguousarray(qoff, np.uint64)
    flags = (engine.APPROX_EDIT if edit else 0) | (engine.APPROX_LOCI if loci else 0) | (engine.APPROX_BEST if best else 0)
    o = engine.ApproxOptions(C.sizeof(engine.ApproxOptions), e, flags, max_hits, comp.ctypes.data if comp is not None else None)
    r = engine.ApproxResult()
    engine._check(engine.lib().kmx_search_approx_opts(idx._h, qranks.ctypes.data if qranks.size else None, qoff.ctypes.data, qoff.size - 1,
                                                      C.byref(o), C.byref(r._h)))
    ho, pos, dist, st = r.host()
    out = {"ho": ho, "pos": pos, "strands": r.strands() if comp is not None else None, "dist": dist, "lens": r.lengths() if edit else None,
           "st": st, "found": r.found(), "counts": r.counts()}
    r.close()
    return out
