"""kmx_windows_vote, CPU part: the contract in numpy (tests/vote_naive.py) against a plain loop, every refusal the header
promises before the result handle is looked at, and the header with the new declarations as C99."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from kmer_index_amd import synth
from tests.vote_naive import vote, vote_loop

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID = 1
NAMES = ("locus_off", "diag", "span", "votes", "skipped")


def assert_same(got, want):
    for name, g, x in zip(NAMES, got[:5], want[:5]):
        assert g.dtype == x.dtype and np.array_equal(g, x), name
    assert got[5] == want[5]


def windows_result(seed, n_windows_per_read, n_text=400, max_hits=9):
    """Host arrays shaped like a windows result: per window 0 .. max_hits ascending positions below n_text (about a third of the
    windows have none)."""
    win_off = np.zeros(len(n_windows_per_read) + 1, np.uint64)
    win_off[1:] = np.cumsum(n_windows_per_read)
    nq = int(win_off[-1])
    z = synth.u64_stream(seed, nq * (max_hits + 1) + 1).astype(np.int64) & 0x7FFFFFFF
    lists = []
    for q in range(nq):
        c = int(z[q * (max_hits + 1)] % (max_hits + 4)) - 3
        lists.append(np.unique(z[q * (max_hits + 1) + 1:q * (max_hits + 1) + 1 + max(c, 0)] % n_text))
    hit_off = np.zeros(nq + 1, np.uint64)
    hit_off[1:] = np.cumsum([x.size for x in lists]) if nq else []
    positions = np.concatenate(lists).astype(np.uint32) if nq and hit_off[-1] else np.zeros(0, np.uint32)
    return hit_off, positions, win_off


# reads without windows at the front, in the middle and at the end; one read with many windows
SHAPES = {"mixed": [0, 5, 0, 0, 17, 1, 40, 0], "one": [23], "no_windows": [0, 0, 0], "no_reads": []}


@pytest.mark.parametrize("shape", list(SHAPES))
@pytest.mark.parametrize("stride", [1, 3])
@pytest.mark.parametrize("band,min_votes,max_occ", [(0, 1, 0), (0, 2, 0), (5, 1, 0), (40, 3, 4), (2, 1, 1), (1000, 1, 0), (3, 1, 100)])
def test_vote_equals_the_loop(shape, stride, band, min_votes, max_occ):
    hit_off, positions, win_off = windows_result(11 + len(shape), SHAPES[shape])
    got = vote(hit_off, positions, win_off, stride, band, min_votes, max_occ)
    want = vote_loop(hit_off, positions, win_off, stride, band, min_votes, max_occ)
    assert_same(got, want)
    assert got[0].size == len(SHAPES[shape]) + 1 and got[4].size == len(SHAPES[shape])


def test_vote_inputs_are_not_vacuous():
    hit_off, positions, win_off = windows_result(11 + len("mixed"), SHAPES["mixed"])
    cnt = np.diff(hit_off.astype(np.int64))
    assert np.count_nonzero(cnt == 0) >= 10 and np.count_nonzero(cnt == 1) >= 3 and np.count_nonzero(cnt > 4) >= 5
    exact = vote(hit_off, positions, win_off, 1, 0, 1, 0)
    banded = vote(hit_off, positions, win_off, 1, 5, 1, 0)
    assert exact[5] == banded[5] == positions.size and exact[1].size > banded[1].size > 0
    assert np.count_nonzero(banded[2]) > 0 and np.all(exact[2] == 0)
    assert np.count_nonzero(exact[1] < 0) > 0                          # diagonals in front of the text
    some = vote(hit_off, positions, win_off, 1, 0, 1, 4)               # max_occ skips some windows ...
    assert 0 < some[5] < positions.size and 0 < int(some[4].sum()) < np.count_nonzero(cnt)
    only_single = vote(hit_off, positions, win_off, 1, 0, 1, 1)
    assert only_single[5] == np.count_nonzero(cnt == 1)
    # ... and all of them: every window with hits gets a second hit, max_occ = 1
    hit2 = (hit_off * np.uint64(2)).astype(np.uint64)
    pos2 = np.repeat(positions, 2)
    got = vote(hit2, pos2, win_off, 1, 0, 1, 1)
    assert_same(got, vote_loop(hit2, pos2, win_off, 1, 0, 1, 1))
    assert got[5] == 0 and got[1].size == 0 and not got[0].any() and int(got[4].sum()) == np.count_nonzero(cnt)


def _opts(engine, band=0, min_votes=1, max_occ=0, flags=0, size=None):
    return engine.VoteOptions(C.sizeof(engine.VoteOptions) if size is None else size, band, min_votes, max_occ, flags)


def test_vote_refuses_bad_arguments_before_the_handle(engine):
    L = engine.lib()
    dummy = C.create_string_buffer(1 << 16)                  # stands for a result handle: never looked into
    res = C.addressof(dummy)
    out = C.c_void_p()
    assert L.kmx_windows_vote(None, C.byref(_opts(engine)), C.byref(out)) == INVALID
    assert L.kmx_windows_vote(res, None, C.byref(out)) == INVALID
    assert L.kmx_windows_vote(res, C.byref(_opts(engine)), None) == INVALID
    assert L.kmx_windows_vote(res, C.byref(_opts(engine, size=16)), C.byref(out)) == INVALID
    assert b"struct_size" in L.kmx_last_error()
    for flags in (1, 2, 1 << 31):
        assert L.kmx_windows_vote(res, C.byref(_opts(engine, flags=flags)), C.byref(out)) == INVALID
        assert b"flags" in L.kmx_last_error()
    assert L.kmx_windows_vote(res, C.byref(_opts(engine, min_votes=0)), C.byref(out)) == INVALID
    assert b"min_votes" in L.kmx_last_error()
    assert not out.value
    assert L.kmx_loci_counts(None, None, None, None, None, None) == INVALID
    assert L.kmx_loci_view(None, None, None, None, None, None) == INVALID
    assert L.kmx_loci_view_device(None, None, None, None, None, None) == INVALID
    L.kmx_loci_free(None)
    assert L.kmx_version() == 5


def test_header_with_vote_declarations_is_c99(tmp_path):
    src = tmp_path / "vote.c"
    src.write_text('#include "kmx.h"\n'
                   "#if KMX_WINDOWS_VOTE != 1\n#error capability macro\n#endif\n"
                   "_Static_assert(sizeof(kmx_vote_options) == 20, \"five words\");\n"
                   "int use(kmx_result* windows) {\n"
                   "  kmx_loci* l = 0; kmx_vote_options o; uint64_t nr, nl, nv, ns, ng;\n"
                   "  const uint64_t* off; const int64_t* diag; const uint32_t* span; const uint32_t* votes; const uint32_t* skipped;\n"
                   "  o.struct_size = (uint32_t)sizeof o; o.band = 8; o.min_votes = 4; o.max_occ = 200; o.flags = 0;\n"
                   "  if (kmx_windows_vote(windows, &o, &l) != KMX_OK) return 1;\n"
                   "  if (kmx_loci_counts(l, &nr, &nl, &nv, &ns, &ng) != KMX_OK) return 2;\n"
                   "  if (kmx_loci_view(l, &off, &diag, &span, &votes, &skipped) != KMX_OK) return 3;\n"
                   "  if (kmx_loci_view_device(l, &off, &diag, &span, &votes, &skipped) != KMX_OK) return 4;\n"
                   "  kmx_loci_free(l);\n"
                   "  return 0;\n}\n")
    res = subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Wextra", "-Werror", "-c", f"-I{os.path.join(ROOT, 'include')}",
                          str(src), "-o", str(tmp_path / "vote.o")], capture_output=True, text=True)
    assert res.returncode == 0, res.stderr
