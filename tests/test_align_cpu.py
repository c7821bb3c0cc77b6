"""kmx_loci_align, CPU part: the contract in numpy (tests/align_naive.align) against the definition itself (align_naive.brute),
every refusal the header promises before a handle is looked at, and the header with the new declarations as C99."""
import ctypes as C
import os
import subprocess

import numpy as np

from kmer_index_amd import synth
from tests.align_naive import MAX_READ, NO_BEST, NONE, SKIPPED, align, brute

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID = 1
NAMES = ("dist", "start", "end", "best", "aligned")
SIGMA = 3


def tiny_case(i):
    """Text of 5 .. 30 letters over three letters; two reads of 1 .. 8 letters, cut from the text with a letter changed now and
    then, or random; per read 1 .. 3 loci with D in -6 .. n + 3 and S in 0 .. 3; E in 0 .. 4."""
    z = synth.u64_stream(9001 + i, 64).astype(np.int64) & 0x7FFFFFFF
    n = 5 + int(z[0] % 26)
    text = synth.ranks(100 + i, n, SIGMA)
    E = int(z[1] % 5)
    reads, off, diag, span = [], [0], [], []
    at = 2
    for r in range(2):
        m = 1 + int(z[at] % 8)
        s = int(z[at + 1] % n)
        if z[at + 2] % 4 == 0 or s + m > n:
            q = synth.ranks(7000 + 2 * i + r, m, SIGMA)
        else:
            q = text[s:s + m].copy()
            if z[at + 3] % 2:
                q[int(z[at + 4] % m)] = (SIGMA, (int(q[0]) + 1) % SIGMA)[int(z[at + 5] % 2)]      # a letter >= sigma now and then
        n_loci = 1 + int(z[at + 6] % 3)
        for k in range(n_loci):
            near = z[at + 7 + 3 * k] % 2 == 0
            diag.append(s - 1 + int(z[at + 8 + 3 * k] % 3) if near else int(z[at + 8 + 3 * k] % (n + 10)) - 6)
            span.append(int(z[at + 9 + 3 * k] % 4))
        off.append(len(diag))
        reads.append(np.asarray(q, np.uint8))
        at += 20
    roff = np.zeros(3, np.uint64)
    roff[1:] = np.cumsum([q.size for q in reads])
    return (text, np.concatenate(reads), roff, np.asarray(off, np.uint64), np.asarray(diag, np.int64), np.asarray(span, np.uint32), E)


def test_align_equals_the_definition():
    """Tests the oracle (align_naive.align against align_naive.brute), not the engine."""
    n_loci = n_aligned = n_none = n_front = n_behind = n_edits = 0
    for i in range(320):
        text, ranks, roff, off, diag, span, E = tiny_case(i)
        got = align(text, ranks, roff, off, diag, span, E, 3, SIGMA)
        want = brute(text, ranks, roff, off, diag, span, E, 3, SIGMA)
        for name, g, x in zip(NAMES, got, want):
            assert g.dtype == x.dtype and np.array_equal(g, x), (i, name, g, x)
        n_loci += diag.size
        n_aligned += int(got[4].sum())
        n_none += int(np.count_nonzero(got[0] == NONE))
        n_edits += int(np.count_nonzero((got[0] > 0) & (got[0] <= E)))
        n_front += int(np.count_nonzero(diag < 0))
        n_behind += int(np.count_nonzero(diag > text.size - 2))
    # the cases are not vacuous: loci that align (with and without edits), loci that do not, diagonals off both ends of the text
    assert n_loci >= 900 and n_aligned >= n_loci // 4 and n_none >= n_loci // 8 and n_edits >= 100
    assert n_front >= 40 and n_behind >= 40


def test_skipped_loci_best_and_aligned():
    """Tests the oracle on a hand-made batch, not the engine."""
    text = synth.ranks(5, 3000, 4)
    long_read = text[100:100 + MAX_READ + 1]
    reads = [text[10:30], long_read, text[50:60], np.zeros(0, np.uint8)]
    ranks = np.concatenate(reads)
    roff = np.zeros(5, np.uint64)
    roff[1:] = np.cumsum([len(q) for q in reads])
    off = np.asarray([0, 3, 4, 6, 6], np.uint64)
    diag = np.asarray([500, 9, 10, 100, 50, 50], np.int64)     # read 0: a wrong place, one letter off, the place itself
    span = np.asarray([0, 0, 5, 0, 0, 0], np.uint32)           # ... whose span is above max_span
    dist, start, end, best, aligned = align(text, ranks, roff, off, diag, span, 2, 4, 4)
    assert dist[0] == NONE and dist[1] == 0 and (start[1], end[1]) == (10, 30) and dist[2] == SKIPPED
    assert dist[3] == SKIPPED and start[3] == 0 and end[3] == 0                                  # the read of MAX_READ + 1 letters
    assert dist[4] == 0 and dist[5] == 0 and (start[5], end[5]) == (50, 60)
    assert list(best) == [1, NO_BEST, 0, NO_BEST] and list(aligned) == [1, 0, 2, 0]


def _opts(engine, max_edits=0, max_span=0, flags=0, size=None):
    return engine.AlignOptions(C.sizeof(engine.AlignOptions) if size is None else size, max_edits, max_span, flags)


def test_align_refuses_bad_arguments_before_the_handles(engine):
    L = engine.lib()
    dummy = C.create_string_buffer(1 << 16)                  # stands for the index and the loci handle: never looked into
    h = C.addressof(dummy)
    roff = (C.c_uint64 * 2)(0, 0)
    out = C.c_void_p()
    ok = _opts(engine)
    for fn, extra in ((L.kmx_loci_align, ()), (L.kmx_loci_align_device, (None,))):
        def call(index, loci, ro, o, inout):
            return fn(index, loci, None, ro, 1, o, *extra, inout)
        for args, word in (((None, h, roff, C.byref(ok), C.byref(out)), b"index"), ((h, None, roff, C.byref(ok), C.byref(out)), b"loci"),
                           ((h, h, roff, None, C.byref(out)), b"options"), ((h, h, roff, C.byref(ok), None), b"inout"),
                           ((h, h, None, C.byref(ok), C.byref(out)), b"roff")):
            assert call(*args) == INVALID
            assert word in L.kmx_last_error()
        assert call(h, h, roff, C.byref(_opts(engine, size=12)), C.byref(out)) == INVALID
        assert b"struct_size" in L.kmx_last_error()
        for flags in (1, 2, 1 << 31):
            assert call(h, h, roff, C.byref(_opts(engine, flags=flags)), C.byref(out)) == INVALID
            assert b"flags" in L.kmx_last_error()
        assert call(h, h, roff, C.byref(_opts(engine, max_edits=engine.ALIGN_MAX_EDITS + 1)), C.byref(out)) == INVALID
        assert b"max_edits" in L.kmx_last_error()
        assert not out.value
    assert L.kmx_alignments_counts(None, None, None, None, None) == INVALID
    assert L.kmx_alignments_view(None, None, None, None, None, None) == INVALID
    assert L.kmx_alignments_view_device(None, None, None, None, None, None) == INVALID
    L.kmx_alignments_free(None)
    assert C.sizeof(engine.AlignOptions) == 16
    assert (engine.ALIGN_MAX_EDITS, engine.ALIGN_MAX_READ, engine.ALIGN_SKIPPED, engine.ALIGN_NONE) == (250, MAX_READ, SKIPPED, NONE)
    assert L.kmx_version() == 5


def test_header_with_align_declarations_is_c99(tmp_path):
    src = tmp_path / "align.c"
    src.write_text('#include "kmx.h"\n'
                   "#if KMX_LOCI_ALIGN != 1 || KMX_VERSION != 5\n#error capability macro\n#endif\n"
                   "_Static_assert(sizeof(kmx_align_options) == 16, \"four words\");\n"
                   "_Static_assert(KMX_ALIGN_MAX_EDITS == 250u && KMX_ALIGN_MAX_READ == 1024u && KMX_ALIGN_SKIPPED == 254u && KMX_ALIGN_NONE == 255u, \"limits\");\n"
                   "int use(const kmx_index* ix, const kmx_loci* l, const uint8_t* ranks, const uint64_t* roff, void* stream) {\n"
                   "  kmx_alignments* a = 0; kmx_align_options o; uint64_t nr, nl, na, ns;\n"
                   "  const uint8_t* dist; const uint32_t* start; const uint32_t* end; const uint32_t* best; const uint32_t* aligned;\n"
                   "  o.struct_size = (uint32_t)sizeof o; o.max_edits = 8; o.max_span = 64; o.flags = 0;\n"
                   "  if (kmx_loci_align(ix, l, ranks, roff, 1, &o, &a) != KMX_OK) return 1;\n"
                   "  if (kmx_loci_align_device(ix, l, ranks, roff, 1, &o, stream, &a) != KMX_OK) return 2;\n"
                   "  if (kmx_alignments_counts(a, &nr, &nl, &na, &ns) != KMX_OK) return 3;\n"
                   "  if (kmx_alignments_view(a, &dist, &start, &end, &best, &aligned) != KMX_OK) return 4;\n"
                   "  if (kmx_alignments_view_device(a, &dist, &start, &end, &best, &aligned) != KMX_OK) return 5;\n"
                   "  kmx_alignments_free(a);\n"
                   "  return 0;\n}\n")
    res = subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Wextra", "-Werror", "-c", f"-I{os.path.join(ROOT, 'include')}",
                          str(src), "-o", str(tmp_path / "align.o")], capture_output=True, text=True)
    assert res.returncode == 0, res.stderr
