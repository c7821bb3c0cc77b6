"""Edit-distance search, CPU part: the independent checker against the brute-force definition, the planted-read generator,
argument validation of the C-ABI (refused before any device is touched) and the header with the new names as C99."""
import ctypes as C
import os
import subprocess

import numpy as np

from kmer_index_amd import synth
from tests.edit_naive import brute_force, edit_naive

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID = 1


def test_checker_equals_brute_force():
    rng = np.random.default_rng(1)
    hits = other_length = 0
    for trial in range(300):
        sigma = [2, 3, 4][trial % 3]
        n = int(rng.integers(1, 70))
        text = rng.integers(0, sigma, n).astype(np.uint8)
        m = int(rng.integers(1, 12))
        e = int(rng.integers(0, 4))
        if trial % 2 and n > m:
            s = int(rng.integers(0, n - m + 1))
            q = text[s:s + m].copy()
        else:
            q = rng.integers(0, sigma, m).astype(np.uint8)
        p, d, L = edit_naive(text, q, e)
        want = brute_force(text.tolist(), q.tolist(), e)
        got = list(zip(p.tolist(), d.tolist(), L.tolist()))
        assert got == want, (trial, sigma, n, m, e)
        hits += len(want)
        other_length += sum(1 for _, _, length in want if length != m)
    assert hits > 0 and other_length > 0


def test_checker_serves_queries_longer_than_the_text():
    text = np.array([0, 1, 2, 3, 0, 1], np.uint8)
    q = np.array([0, 1, 2, 3, 0, 1, 2], np.uint8)           # m = n + 1: the whole text is one deletion away
    p, d, L = edit_naive(text, q, 1)
    assert (p.tolist(), d.tolist(), L.tolist()) == ([0], [1], [6])
    assert edit_naive(text, q, 0)[0].size == 0


def test_planted_edit_reads_are_within_their_edits():
    text = synth.ranks(5, 20_000, 4)
    q, off, start = synth.planted_reads_edit(9, text, 200, 24, 4, 3)
    assert off.size == 201 and q.size == 200 * 24 and start.size == 200
    seen = set()
    other_length = 0
    for i in range(200):
        p, d, L = edit_naive(text, q[i * 24:(i + 1) * 24], 3)
        at = np.nonzero(p == start[i])[0]
        assert at.size == 1, i                       # its source start is within 3 edits
        seen.add(int(d[at[0]]))
        other_length += int(L[at[0]] != 24)
    assert seen == {0, 1, 2, 3} and other_length > 0   # ... and some of them through insertions or deletions
    q0, _, s0 = synth.planted_reads_edit(9, text, 50, 24, 4, 0)
    for i in range(50):
        assert np.array_equal(q0[i * 24:(i + 1) * 24], text[int(s0[i]):int(s0[i]) + 24])


def test_edit_calls_refuse_bad_arguments_without_a_device(engine):
    L = engine.lib()
    out = C.c_void_p()
    qoff = np.array([0, 4], np.uint64)
    qr = np.zeros(4, np.uint8)
    assert engine.APPROX_EDIT == 1
    assert L.kmx_search_approx(None, qr.ctypes.data, qoff.ctypes.data, 1, 1, engine.APPROX_EDIT, C.byref(out)) == INVALID
    dummy = C.create_string_buffer(64)         # never dereferenced: the arguments are refused first
    assert L.kmx_search_approx(C.addressof(dummy), qr.ctypes.data, qoff.ctypes.data, 1, 1, 2, C.byref(out)) == INVALID
    assert b"flag" in L.kmx_last_error()
    assert L.kmx_search_approx(C.addressof(dummy), qr.ctypes.data, qoff.ctypes.data, 1, 1, 3, C.byref(out)) == INVALID
    assert L.kmx_search_approx(C.addressof(dummy), qr.ctypes.data, qoff.ctypes.data, 1, 4, engine.APPROX_EDIT, C.byref(out)) == INVALID
    assert b"max_subst" in L.kmx_last_error()
    p = C.c_void_p()
    assert L.kmx_approx_lengths(None, C.byref(p)) == INVALID
    assert L.kmx_approx_lengths(None, None) == INVALID
    assert L.kmx_version() == 5


def test_header_with_edit_names_is_c99(tmp_path):
    src = tmp_path / "edit.c"
    src.write_text('#include "kmx.h"\n'
                   "_Static_assert(KMX_APPROX_EDIT == 1u, \"flag\");\n"
                   "int use(const kmx_index* ix, const uint8_t* q, const uint64_t* o) {\n"
                   "  kmx_approx_result* r = 0; const uint64_t* h; const uint32_t* p; const uint8_t* d; const uint8_t* st;\n"
                   "  const uint32_t* len;\n"
                   "  if (kmx_search_approx(ix, q, o, 1, 2, KMX_APPROX_EDIT, &r) != KMX_OK) return 1;\n"
                   "  kmx_approx_view(r, &h, &p, &d, &st);\n"
                   "  if (kmx_approx_lengths(r, &len) != KMX_OK) return 2;\n"
                   "  kmx_approx_free(r);\n"
                   "  return 0;\n}\n")
    res = subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Wextra", "-Werror", "-c", f"-I{os.path.join(ROOT, 'include')}",
                          str(src), "-o", str(tmp_path / "edit.o")], capture_output=True, text=True)
    assert res.returncode == 0, res.stderr
