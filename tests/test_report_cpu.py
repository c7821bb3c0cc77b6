"""Reporting options of the approximate search (kmx_search_approx_opts), CPU part: properties of the independent checker on
tiny random cases, argument validation of the C-ABI (refused before any device is touched) and the header with the new names
as C99."""
import ctypes as C
import os
import subprocess

import numpy as np

from tests.report_naive import best, cap, hits_naive, loci, report_naive

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID = 1
COMP = {2: [1, 0], 4: [3, 2, 1, 0]}


def _cases():
    """About 200 tiny cases (text, q, e, edit, complement or None): repetitive texts, so that lists are long and loci close."""
    rng = np.random.default_rng(11)
    for trial in range(208):
        sigma = 2 if trial % 2 else 4
        n = int(rng.integers(12, 70))
        unit = rng.integers(0, sigma, int(rng.integers(1, 9))).astype(np.uint8)
        text = np.tile(unit, n // unit.size + 1)[:n].copy()
        noise = rng.integers(0, n, n // 6)
        text[noise] = rng.integers(0, sigma, noise.size).astype(np.uint8)
        m = int(rng.integers(4, 11))
        e = int(rng.integers(0, 4))
        s = int(rng.integers(0, n - m + 1))
        q = text[s:s + m].copy()
        if trial % 3 == 0:
            q[int(rng.integers(0, m))] = rng.integers(0, sigma)
        edit = trial % 4 < 2
        comp = COMP[sigma] if trial % 8 >= 4 else None
        yield text, q, e, edit, comp


def test_checker_properties():
    removed_loci = removed_best = cut = uncut = two_strata = 0
    for text, q, e, edit, comp in _cases():
        H = hits_naive(text, q, e, edit, comp)
        assert H == sorted(H, key=lambda h: (h[0], h[1])) and len({h[:2] for h in H}) == len(H)
        L1 = loci(H, e)
        both = best(L1)
        assert both == loci(best(H), e)                            # the two steps commute
        assert set(L1) <= set(H) and set(both) <= set(L1)          # subsets; d and L carried over (whole tuples compared)
        if e == 0:
            assert L1 == H
        if H:
            d0, p0, s0 = min((h[2], h[0], h[1]) for h in H)        # the leftmost least-distance hit always survives
            assert any(h[:3] == (p0, s0, d0) for h in both)
            assert {h[2] for h in both} == {d0}
        for s in (0, 1):                                           # different strands never suppress each other
            one = [h for h in H if h[1] == s]
            assert [h for h in L1 if h[1] == s] == loci(one, e)
        for use_loci, use_best in ((False, False), (True, False), (False, True), (True, True)):
            if use_loci and not edit:
                continue
            base = report_naive(H, e, use_loci, use_best, 0)
            assert base[0] == len(base[1])
            for max_hits in (1, 2, 3, 5):
                found, kept = report_naive(H, e, use_loci, use_best, max_hits)
                assert found == base[0] and len(kept) == min(found, max_hits)
                assert kept == sorted(kept, key=lambda h: (h[0], h[1])) and set(kept) <= set(base[1])
                order = sorted(base[1], key=lambda h: (h[2], h[0], h[1]))
                assert sorted(kept, key=lambda h: (h[2], h[0], h[1])) == order[:max_hits]      # a prefix of the (d, p, strand) order
                cut += found > max_hits
                uncut += found <= max_hits
        removed_loci += (len(H) - len(L1)) if edit else 0
        removed_best += len(L1) - len(both)
        two_strata += len({h[2] for h in L1}) > 1
    assert removed_loci > 100 and removed_best > 100 and cut > 100 and uncut > 100 and two_strata > 20


def test_loci_radius_and_ties():
    # equal distances e apart collapse onto the leftmost, e + 1 apart they do not; a worse hit between two better ones goes
    H = [(10, 0, 1, 8), (12, 0, 1, 8), (15, 0, 1, 8)]
    assert loci(H, 2) == [(10, 0, 1, 8), (15, 0, 1, 8)]
    H = [(10, 0, 0, 8), (11, 0, 1, 7), (12, 0, 2, 6), (13, 0, 1, 8), (14, 0, 0, 8)]
    assert loci(H, 2) == [(10, 0, 0, 8), (14, 0, 0, 8)]
    # the rule looks at H, not at the survivors: 12 is removed by 11 although 11 is removed by 10
    H = [(10, 0, 0, 8), (11, 0, 1, 8), (12, 0, 2, 8)]
    assert loci(H, 1) == [(10, 0, 0, 8)]
    # a forward and a reverse hit at one offset, and next to each other
    H = [(10, 0, 1, 8), (10, 1, 1, 8), (11, 1, 2, 8)]
    assert loci(H, 1) == [(10, 0, 1, 8), (10, 1, 1, 8)]
    assert cap(best([(4, 0, 1, 8), (9, 0, 0, 8), (9, 1, 0, 8), (20, 0, 0, 8)]), 2) == (3, [(9, 0, 0, 8), (9, 1, 0, 8)])
    assert cap([(4, 0, 1, 8), (9, 0, 0, 8), (30, 0, 1, 8)], 2) == (3, [(4, 0, 1, 8), (9, 0, 0, 8)])


def _options(engine, e, flags, max_hits=0, size=None, comp=None):
    return engine.ApproxOptions(C.sizeof(engine.ApproxOptions) if size is None else size, e, flags, max_hits, comp)


def test_opts_call_refuses_bad_arguments_without_a_device(engine):
    L = engine.lib()
    out = C.c_void_p()
    qoff = np.array([0, 4], np.uint64)
    qr = np.zeros(4, np.uint8)
    dummy = C.create_string_buffer(64)         # never dereferenced: the arguments are refused first
    ix = C.addressof(dummy)
    args = (qr.ctypes.data, qoff.ctypes.data, 1)
    good = _options(engine, 1, engine.APPROX_EDIT | engine.APPROX_LOCI | engine.APPROX_BEST, 3)
    assert C.sizeof(engine.ApproxOptions) == 24
    assert L.kmx_search_approx_opts(None, *args, C.byref(good), C.byref(out)) == INVALID
    assert L.kmx_search_approx_opts(ix, *args, C.byref(good), None) == INVALID
    assert L.kmx_search_approx_opts(ix, *args, None, C.byref(out)) == INVALID
    assert b"options" in L.kmx_last_error()
    for size in (0, 16, 23):
        o = _options(engine, 1, engine.APPROX_EDIT, size=size)
        assert L.kmx_search_approx_opts(ix, *args, C.byref(o), C.byref(out)) == INVALID
        assert b"struct_size" in L.kmx_last_error()
    for flags in (8, 9, 16, 1 << 31):
        o = _options(engine, 1, flags)
        assert L.kmx_search_approx_opts(ix, *args, C.byref(o), C.byref(out)) == INVALID
        assert b"flag" in L.kmx_last_error()
    for flags in (engine.APPROX_LOCI, engine.APPROX_LOCI | engine.APPROX_BEST):
        o = _options(engine, 1, flags)
        assert L.kmx_search_approx_opts(ix, *args, C.byref(o), C.byref(out)) == INVALID
        assert b"KMX_APPROX_LOCI needs KMX_APPROX_EDIT" in L.kmx_last_error()
    for flags in (0, engine.APPROX_EDIT | engine.APPROX_LOCI, engine.APPROX_BEST):
        o = _options(engine, 4, flags, 1)
        assert L.kmx_search_approx_opts(ix, *args, C.byref(o), C.byref(out)) == INVALID
        assert b"max_subst" in L.kmx_last_error()
    p = C.c_void_p()
    assert L.kmx_approx_found(None, C.byref(p)) == INVALID
    assert L.kmx_approx_found(None, None) == INVALID
    # the older entry points refuse the new bits as before
    for flags in (2, 3, 4):
        assert L.kmx_search_approx(ix, *args, 1, flags, C.byref(out)) == INVALID
        assert b"flag" in L.kmx_last_error()
    assert (engine.APPROX_EDIT, engine.APPROX_LOCI, engine.APPROX_BEST) == (1, 2, 4)
    assert L.kmx_version() == 5


def test_header_with_report_names_is_c99(tmp_path):
    src = tmp_path / "report.c"
    src.write_text('#include "kmx.h"\n'
                   "_Static_assert(KMX_APPROX_REPORT == 1, \"capability\");\n"
                   "_Static_assert(KMX_APPROX_LOCI == 2u && KMX_APPROX_BEST == 4u && KMX_APPROX_EDIT == 1u, \"flag bits\");\n"
                   "_Static_assert(KMX_VERSION == 5, \"version\");\n"
                   "int use(const kmx_index* ix, const uint8_t* q, const uint64_t* o) {\n"
                   "  static const uint8_t comp[4] = {3, 2, 1, 0};\n"
                   "  kmx_approx_options opt;\n"
                   "  kmx_approx_result* r = 0; const uint64_t* h; const uint32_t* p; const uint8_t* d; const uint8_t* st;\n"
                   "  const uint64_t* found;\n"
                   "  opt.struct_size = (uint32_t)sizeof opt; opt.max_subst = 2; opt.max_hits = 1; opt.complement = comp;\n"
                   "  opt.flags = KMX_APPROX_EDIT | KMX_APPROX_LOCI | KMX_APPROX_BEST;\n"
                   "  if (kmx_search_approx_opts(ix, q, o, 1, &opt, &r) != KMX_OK) return 1;\n"
                   "  kmx_approx_view(r, &h, &p, &d, &st);\n"
                   "  if (kmx_approx_found(r, &found) != KMX_OK) return 2;\n"
                   "  opt.max_hits = (uint32_t)(found[0] > h[1] - h[0]);\n"
                   "  kmx_approx_free(r);\n"
                   "  return (int)opt.max_hits;\n}\n")
    res = subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Wextra", "-Werror", "-c", f"-I{os.path.join(ROOT, 'include')}",
                          str(src), "-o", str(tmp_path / "report.o")], capture_output=True, text=True)
    assert res.returncode == 0, res.stderr
