"""kmx_alignments_scripts, CPU part: the contract in Python (tests/script_naive) against an enumeration of every optimal script, the
consequences the header lists on random aligned loci of align_naive, every refusal the header promises before a handle is looked
at, and the header with the new declarations as C99."""
import ctypes as C
import os
import subprocess

import numpy as np

from kmer_index_amd import synth
from tests import script_naive as sn
from tests.align_naive import align_one

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID = 1
RANK = {sn.OP_EQ: 2, sn.OP_X: 2, sn.OP_D: 1, sn.OP_I: 0}        # the order of the walk: '=' / 'X' before 'D' before 'I'


def all_optimal(q, t, sigma, h):
    """Every optimal script of q against t as the tuple of its ops read from its end."""
    out = []

    def go(i, j, ops):
        if i == 0 and j == 0:
            out.append(tuple(ops))
            return
        if i and j:
            c = 0 if int(q[i - 1]) == int(t[j - 1]) and int(q[i - 1]) < sigma else 1
            if h[i - 1][j - 1] + c == h[i][j]:
                go(i - 1, j - 1, ops + [sn.OP_X if c else sn.OP_EQ])
        if j and h[i][j - 1] + 1 == h[i][j]:
            go(i, j - 1, ops + [sn.OP_D])
        if i and h[i - 1][j] + 1 == h[i][j]:
            go(i - 1, j, ops + [sn.OP_I])

    go(len(q), len(t), [])
    return out


def test_the_script_is_the_greatest_of_all_optimal_ones():
    """Tests the oracle: on tiny cases the walk's script, read from its end, is the lexicographically greatest of all optimal scripts
    under '=' / 'X' > 'D' > 'I' (and the only one with that key: whether a diagonal step is '=' or 'X' is fixed by the letters)."""
    n_cases = n_many = n_foreign = 0
    for i in range(600):
        z = synth.u64_stream(31_000 + i, 8).astype(np.int64) & 0x7FFFFFFF
        sigma = 2 + int(z[0] % 2)
        m, L = int(z[1] % 7), int(z[2] % 8)
        q = synth.ranks(41_000 + i, m, sigma)
        t = synth.ranks(51_000 + i, L, sigma)
        if z[3] % 3 == 0 and m and L:                            # related strings: more ties between the three moves
            q = np.resize(t, m).copy()
            q[int(z[4] % m)] = (int(q[int(z[4] % m)]) + 1) % sigma
        if z[5] % 5 == 0 and m:
            q[int(z[6] % m)] = sigma                              # a letter >= sigma now and then
            n_foreign += 1
        h = sn.full_h(q, t, sigma)
        every = all_optimal(q, t, sigma, h)
        ops = sn.walk(q, t, sigma, h)
        key = tuple(RANK[o] for o in ops[::-1])
        keys = [tuple(RANK[o] for o in s) for s in every]
        assert tuple(ops[::-1]) in every and key == max(keys) and keys.count(key) == 1, (i, q, t)
        edits, exact = sn.replay(q, t, sn.rle(ops), sigma)
        assert exact and edits == h[m][L]
        n_cases += 1
        n_many += len(every) > 1
    assert n_cases == 600 and n_many >= 200 and n_foreign >= 60


def random_aligned_loci(count):
    """(q, t, d, sigma) of loci that align_naive.align_one aligns: reads cut from a text of 4 letters with substitutions, insertions
    and deletions (some inside runs of one letter), some random, a letter >= sigma now and then, D within a few letters of the cut."""
    sigma = 4
    i = 0
    while count:
        z = synth.u64_stream(61_000 + i, 24).astype(np.int64) & 0x7FFFFFFF
        n = 60 + int(z[0] % 60)
        text = synth.ranks(71_000 + i, n, sigma)
        if z[1] % 2:
            a = int(z[2] % (n - 12))
            text[a:a + 3 + int(z[3] % 8)] = text[a]               # a run of one letter
        m = 1 + int(z[4] % 40)
        s = int(z[5] % (n - m + 1))
        q = list(text[s:s + m])
        for e in range(int(z[6] % 5)):
            at = int(z[7 + 3 * e] % (len(q) + 1))
            kind = int(z[8 + 3 * e] % 3)
            if kind == 0 and at < len(q):
                q[at] = (int(q[at]) + 1 + int(z[9 + 3 * e] % 3)) % sigma
            elif kind == 1:
                q.insert(at, int(z[9 + 3 * e] % sigma))
            elif at < len(q) and len(q) > 1:
                del q[at]
        if z[22] % 9 == 0:
            q[int(z[23] % len(q))] = sigma + int(z[23] % 2) * 200
        if z[22] % 13 == 1:
            q = list(synth.ranks(81_000 + i, len(q), sigma))
        q = np.asarray(q, np.uint8)
        E = 1 + int(z[21] % 8)
        D = s - 2 + int(z[20] % 5)
        d, a, b = align_one(text, q, D, int(z[19] % 3), E, sigma)
        i += 1
        if d <= E:
            count -= 1
            yield q, text[a:b], d, sigma


def test_consequences_on_random_aligned_loci():
    n = n_gap = n_sub = n_clean = n_band = 0
    for q, t, d, sigma in random_aligned_loci(2100):
        runs, mismatched = sn.script_one(q, t, d, sigma)
        assert not mismatched
        by = {op: sum(int(v) >> 4 for v in runs if int(v) & 15 == op) for op in (sn.OP_EQ, sn.OP_X, sn.OP_I, sn.OP_D)}
        assert by[sn.OP_X] + by[sn.OP_I] + by[sn.OP_D] == d
        assert by[sn.OP_EQ] + by[sn.OP_X] + by[sn.OP_I] == len(q) and by[sn.OP_EQ] + by[sn.OP_X] + by[sn.OP_D] == len(t)
        assert runs and int(runs[0]) & 15 != sn.OP_D and int(runs[-1]) & 15 != sn.OP_D        # start and end forbid it
        assert len(runs) <= 2 * d + 1
        assert all((int(a) & 15) != (int(b) & 15) for a, b in zip(runs, runs[1:])) and all(int(v) >> 4 for v in runs)
        assert sn.replay(q, t, runs, sigma) == (d, True)
        merged = sn.script_one(q, t, d, sigma, m=True)[0]
        assert sn.replay(q, t, merged, sigma) == (d, True) and all(int(v) & 15 in (sn.OP_M, sn.OP_I, sn.OP_D) for v in merged)
        # the band |j - i| <= d changes nothing: the walk stays inside it
        i, j = len(q), len(t)
        for v in runs[::-1]:
            for _ in range(int(v) >> 4):
                assert abs(j - i) <= d
                i -= int(v) & 15 != sn.OP_D
                j -= int(v) & 15 != sn.OP_I
        n += 1
        n_gap += by[sn.OP_I] + by[sn.OP_D] > 0
        n_sub += by[sn.OP_X] > 0
        n_clean += d == 0
        n_band += d > 0 and abs(len(q) - len(t)) == d
    assert n >= 2000 and n_gap >= 400 and n_sub >= 400 and n_clean >= 200 and n_band >= 100


def test_gaps_come_out_left_aligned():
    acgt = {"A": 0, "C": 1, "G": 2, "T": 3}
    t = np.asarray([acgt[c] for c in "ACGTTTTTACG"], np.uint8)
    shorter = np.asarray([acgt[c] for c in "ACGTTTTACG"], np.uint8)
    longer = np.asarray([acgt[c] for c in "ACGTTTTTTACG"], np.uint8)
    for q, want in ((shorter, "3=1D7="), (longer, "3=1I8="), (t, "11=")):
        runs, mismatched = sn.script_one(q, t, int(q.size != t.size), 4)
        assert not mismatched and sn.strings([0, len(runs)], runs) == [want]
    assert sn.strings([0, 1], sn.script_one(shorter, t, 1, 4, m=True)[0][:1]) == ["3M"]
    # dist == m with L = 0: the single run mI; a distance the DP does not end at, a read too far from L: mismatched
    assert sn.script_one(shorter, t[:0], 10, 4) == ([(10 << 4) | sn.OP_I], False)
    assert sn.script_one(shorter, t, 2, 4) == ([], True) and sn.script_one(shorter, t[:8], 1, 4) == ([], True)
    assert sn.script_one(np.zeros(0, np.uint8), t[:0], 0, 4) == ([], False)


def test_selection():
    off = np.asarray([0, 2, 2, 5], np.uint64)
    dist = np.asarray([3, 0, 255, 254, 7], np.uint8)
    best = np.asarray([1, 0xFFFFFFFF, 2], np.uint32)
    a, b = sn.select(off, dist, best)
    assert a.dtype == np.uint64 and b.dtype == np.uint32 and list(a) == [0, 1, 1, 2] and list(b) == [1, 4]
    a, b = sn.select(off, dist, best, all=True)
    assert list(a) == [0, 2, 2, 3] and list(b) == [0, 1, 4]


def _opts(engine, flags=0, size=None, scratch=0):
    return engine.ScriptOptions(C.sizeof(engine.ScriptOptions) if size is None else size, flags, scratch)


def test_scripts_refuse_bad_arguments_before_the_handles(engine):
    L = engine.lib()
    dummy = C.create_string_buffer(1 << 16)                  # stands for the index and the two handles: never looked into
    h = C.addressof(dummy)
    roff = (C.c_uint64 * 2)(0, 0)
    out = C.c_void_p()
    ok = _opts(engine)
    for fn, extra in ((L.kmx_alignments_scripts, ()), (L.kmx_alignments_scripts_device, (None,))):
        def call(index, loci, al, ro, o, inout):
            return fn(index, loci, al, None, ro, 1, o, *extra, inout)
        for args, word in (((None, h, h, roff, C.byref(ok), C.byref(out)), b"index"), ((h, None, h, roff, C.byref(ok), C.byref(out)), b"loci"),
                           ((h, h, None, roff, C.byref(ok), C.byref(out)), b"alignments"), ((h, h, h, roff, None, C.byref(out)), b"options"),
                           ((h, h, h, roff, C.byref(ok), None), b"inout"), ((h, h, h, None, C.byref(ok), C.byref(out)), b"roff")):
            assert call(*args) == INVALID
            assert word in L.kmx_last_error()
        assert call(h, h, h, roff, C.byref(_opts(engine, size=12)), C.byref(out)) == INVALID
        assert b"struct_size" in L.kmx_last_error()
        for flags in (4, 8, 1 << 31, 3 | 1 << 16):
            assert call(h, h, h, roff, C.byref(_opts(engine, flags=flags)), C.byref(out)) == INVALID
            assert b"flags" in L.kmx_last_error()
        assert not out.value
    assert L.kmx_scripts_counts(None, None, None, None, None) == INVALID
    assert L.kmx_scripts_view(None, None, None, None, None) == INVALID
    assert L.kmx_scripts_view_device(None, None, None, None, None) == INVALID
    L.kmx_scripts_free(None)
    assert C.sizeof(engine.ScriptOptions) == 16
    assert (engine.SCRIPT_ALL, engine.SCRIPT_M) == (1, 2)
    assert L.kmx_version() == 5


def test_header_with_script_declarations_is_c99(tmp_path):
    src = tmp_path / "script.c"
    src.write_text('#include "kmx.h"\n'
                   "#if KMX_ALIGN_SCRIPTS != 1 || KMX_VERSION != 5\n#error capability macro\n#endif\n"
                   "_Static_assert(sizeof(kmx_script_options) == 16, \"two words and a long one\");\n"
                   "_Static_assert(KMX_SCRIPT_ALL == 1u && KMX_SCRIPT_M == 2u, \"flags\");\n"
                   "int use(const kmx_index* ix, const kmx_loci* l, const kmx_alignments* a, const uint8_t* ranks, const uint64_t* roff, void* stream) {\n"
                   "  kmx_scripts* s = 0; kmx_script_options o; uint64_t nr, ns, no, nm;\n"
                   "  const uint64_t* rso; const uint32_t* sel; const uint64_t* co; const uint32_t* cigar;\n"
                   "  o.struct_size = (uint32_t)sizeof o; o.flags = KMX_SCRIPT_ALL | KMX_SCRIPT_M; o.scratch_bytes = 0;\n"
                   "  if (kmx_alignments_scripts(ix, l, a, ranks, roff, 1, &o, &s) != KMX_OK) return 1;\n"
                   "  if (kmx_alignments_scripts_device(ix, l, a, ranks, roff, 1, &o, stream, &s) != KMX_OK) return 2;\n"
                   "  if (kmx_scripts_counts(s, &nr, &ns, &no, &nm) != KMX_OK) return 3;\n"
                   "  if (kmx_scripts_view(s, &rso, &sel, &co, &cigar) != KMX_OK) return 4;\n"
                   "  if (kmx_scripts_view_device(s, &rso, &sel, &co, &cigar) != KMX_OK) return 5;\n"
                   "  kmx_scripts_free(s);\n"
                   "  return 0;\n}\n")
    res = subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Wextra", "-Werror", "-c", f"-I{os.path.join(ROOT, 'include')}",
                          str(src), "-o", str(tmp_path / "script.o")], capture_output=True, text=True)
    assert res.returncode == 0, res.stderr
