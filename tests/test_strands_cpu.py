"""Both-strand search, CPU part: the independent checker against brute-force loops, the complement tables, the planted
strand reads, argument validation of the C-ABI (refused before any device is touched) and the header with the new names
as C99."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from kmer_index_amd import synth
from tests import approx_naive, edit_naive
from tests.strand_naive import revcomp, strand_naive

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID = 1
COMP = {2: [1, 0], 4: [3, 2, 1, 0], 5: [4, 2, 1, 3, 0]}


def _brute(text, q, e, comp, edit):
    """[(p, strand, d, L)] from plain Python loops over both strands, sorted by (p, strand); L is 0 for Hamming."""
    out = []
    for strand, query in enumerate((list(q), [comp[c] for c in reversed(q)])):
        if edit:
            out += [(p, strand, d, length) for p, d, length in edit_naive.brute_force(text, query, e)]
        else:
            pos, mm = approx_naive.brute_force(text, query, e)
            out += [(p, strand, d, 0) for p, d in zip(pos, mm)]
    return sorted(out)


@pytest.mark.parametrize("edit", [False, True], ids=["hamming", "edit"])
def test_checker_equals_brute_force(edit):
    rng = np.random.default_rng(7)
    hits = twice = self_rc = 0
    for trial in range(240):
        sigma = [2, 4, 5][trial % 3]
        comp = COMP[sigma]
        n = int(rng.integers(2, 60))
        text = rng.integers(0, sigma, n).astype(np.uint8)
        m = int(rng.integers(1, 11))
        e = int(rng.integers(0, 4))
        kind = trial % 4
        if kind == 0:
            q = rng.integers(0, sigma, m).astype(np.uint8)
        elif kind == 3:                               # its own reverse complement: a half and the reverse complement of it
            half = rng.integers(0, sigma, max(m // 2, 1)).astype(np.uint8)
            q = np.concatenate([half, revcomp(half, comp)])
            assert np.array_equal(revcomp(q, comp), q)
            if n >= q.size:
                s = int(rng.integers(0, n - q.size + 1))
                text[s:s + q.size] = q
            self_rc += 1
        else:
            m = min(m, n)
            s = int(rng.integers(0, n - m + 1))
            q = text[s:s + m].copy()
            if kind == 2:
                q = revcomp(q, comp)
        if edit and q.size <= e:
            continue
        p, s_, d, length = strand_naive(text, q, e, comp, edit)
        got = list(zip(p.tolist(), s_.tolist(), d.tolist(), length.tolist() if edit else [0] * p.size))
        want = _brute(text.tolist(), q.tolist(), e, comp, edit)
        assert got == want, (trial, sigma, n, q.size, e)
        hits += len(want)
        twice += sum(1 for a, b in zip(want, want[1:]) if a[0] == b[0])
        if kind == 3:                                 # every hit on both strands, forward first
            assert len(want) % 2 == 0 and all(a[0] == b[0] and (a[1], b[1]) == (0, 1) and a[2:] == b[2:]
                                              for a, b in zip(want[::2], want[1::2]))
    assert hits > 0 and twice > 0 and self_rc > 0


def test_complement_tables(engine):
    for sigma in (4, 5, 15):
        t = engine.complement_table(sigma)
        assert t.dtype == np.uint8 and t.size == sigma
        assert np.all(t < sigma) and np.array_equal(t[t], np.arange(sigma))
    assert engine.complement_table(4).tolist() == [3, 2, 1, 0]
    assert engine.complement_table(5).tolist() == [4, 2, 1, 3, 0]          # ACGNT: N maps to N
    chars = "ABCDGHKMNRSTVWY"                                              # the rank order of alphabet.hpp's dna15
    iupac = {"A": "T", "C": "G", "G": "C", "T": "A", "R": "Y", "Y": "R", "S": "S", "W": "W", "K": "M", "M": "K",
             "B": "V", "V": "B", "D": "H", "H": "D", "N": "N"}
    t = engine.complement_table(15)
    for r, c in enumerate(chars):
        assert chars[int(t[r])] == iupac[c], c
    hdr = open(os.path.join(ROOT, "include", "kmer_index_amd", "alphabet.hpp")).read()
    assert f'dna15_chars[] = "{chars}"' in hdr and 'dna5_chars[] = "ACGNT"' in hdr and 'dna4_chars[] = "ACGT"' in hdr
    with pytest.raises(ValueError):
        engine.complement_table(20)


def test_revcomp_of_a_batch():
    comp = np.array(COMP[4], np.uint8)
    q = np.array([0, 1, 2, 3, 0, 0, 1, 3], np.uint8)
    off = np.array([0, 3, 3, 4, 8], np.uint64)                             # lengths 3, 0, 1, 4
    assert synth.revcomp(q, off, comp).tolist() == [1, 2, 3, 0, 0, 2, 3, 3]
    assert np.array_equal(synth.revcomp(synth.revcomp(q, off, comp), off, comp), q)
    assert synth.revcomp(np.zeros(0, np.uint8), np.array([0, 0], np.uint64), comp).size == 0
    for i in range(4):
        a, b = int(off[i]), int(off[i + 1])
        assert np.array_equal(synth.revcomp(q, off, comp)[a:b], revcomp(q[a:b], comp))


@pytest.mark.parametrize("edit", [False, True], ids=["hamming", "edit"])
def test_planted_strand_reads_are_found_on_their_strand(edit):
    text = synth.ranks(5, 20_000, 4)
    comp = np.array(COMP[4], np.uint8)
    nq, m, e = 120, 24, 3
    gen = synth.planted_reads_edit_strands if edit else synth.planted_reads_strands
    q, off, strand, start = gen(9, text, nq, m, 4, e, comp)
    assert off.size == nq + 1 and q.size == nq * m and strand.size == nq and start.size == nq
    assert 0 < int(strand.sum()) < nq                                      # both strands occur
    plain = (synth.planted_reads_edit if edit else synth.planted_reads)(9, text, nq, m, 4, e)[0]
    for i in range(nq):
        read = q[i * m:(i + 1) * m]
        src = plain[i * m:(i + 1) * m]
        assert np.array_equal(read, revcomp(src, comp) if strand[i] else src)
        p, s, d, _ = strand_naive(text, read, e, comp, edit)
        assert np.any((p == start[i]) & (s == strand[i])), i               # its source start, on the recorded strand


def test_strand_calls_refuse_bad_arguments_without_a_device(engine):
    L = engine.lib()
    out = C.c_void_p()
    qoff = np.array([0, 4], np.uint64)
    qr = np.zeros(4, np.uint8)
    comp = np.array([3, 2, 1, 0], np.uint8)
    dummy = C.create_string_buffer(64)         # never dereferenced: the arguments are refused first
    ix = C.addressof(dummy)
    args = (qr.ctypes.data, qoff.ctypes.data, 1)
    assert L.kmx_search_approx_strands(None, *args, 1, 0, comp.ctypes.data, C.byref(out)) == INVALID
    assert L.kmx_search_approx_strands(ix, *args, 1, 0, comp.ctypes.data, None) == INVALID
    assert L.kmx_search_approx_strands(ix, *args, 1, 0, None, C.byref(out)) == INVALID
    assert b"complement" in L.kmx_last_error()
    assert L.kmx_search_approx_strands(ix, *args, 4, 0, comp.ctypes.data, C.byref(out)) == INVALID
    assert b"max_subst" in L.kmx_last_error()
    for flags in (2, 3, 4):
        assert L.kmx_search_approx_strands(ix, *args, 1, flags, comp.ctypes.data, C.byref(out)) == INVALID
        assert b"flag" in L.kmx_last_error()
    p = C.c_void_p()
    assert L.kmx_approx_strands(None, C.byref(p)) == INVALID
    assert L.kmx_approx_strands(None, None) == INVALID
    assert L.kmx_version() == 5


def test_header_with_strand_names_is_c99(tmp_path):
    src = tmp_path / "strands.c"
    src.write_text('#include "kmx.h"\n'
                   "_Static_assert(KMX_APPROX_BOTH_STRANDS == 1, \"capability\");\n"
                   "int use(const kmx_index* ix, const uint8_t* q, const uint64_t* o) {\n"
                   "  static const uint8_t comp[4] = {3, 2, 1, 0};\n"
                   "  kmx_approx_result* r = 0; const uint64_t* h; const uint32_t* p; const uint8_t* d; const uint8_t* st;\n"
                   "  const uint8_t* strands;\n"
                   "  if (kmx_search_approx_strands(ix, q, o, 1, 2, KMX_APPROX_EDIT, comp, &r) != KMX_OK) return 1;\n"
                   "  kmx_approx_view(r, &h, &p, &d, &st);\n"
                   "  if (kmx_approx_strands(r, &strands) != KMX_OK) return 2;\n"
                   "  kmx_approx_free(r);\n"
                   "  return 0;\n}\n")
    res = subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Wextra", "-Werror", "-c", f"-I{os.path.join(ROOT, 'include')}",
                          str(src), "-o", str(tmp_path / "strands.o")], capture_output=True, text=True)
    assert res.returncode == 0, res.stderr
