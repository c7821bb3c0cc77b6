"""kmx_search_windows, CPU part: the expander (tests/windows_naive.py) against a brute-force loop, every refusal the header
promises "before any device is touched", and the header with the new declarations as C99."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from kmer_index_amd import synth
from tests.helpers import pack
from tests.windows_naive import expand, expand_loop

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID = 1
W = 4


@pytest.mark.parametrize("stride", [1, 2, W, W + 3])
def test_expander_equals_brute_force(stride):
    # reads of length 0, w - 1, w, w + 1; a last window flush with the read's end (len = w + 2 * stride) and one letter short
    # of it (len = w + 2 * stride - 1: the third window does not fit), then some longer ones
    lens = [0, W - 1, W, W + 1, W + 2 * stride, W + 2 * stride - 1, 0, 23, W, 1, 40]
    reads = [synth.ranks(100 + i, n, 4) for i, n in enumerate(lens)]
    ranks, roff = pack(reads)
    q, off, win = expand(ranks, roff, W, stride)
    ql, offl, winl = expand_loop(ranks, roff, W, stride)
    assert np.array_equal(q, ql) and np.array_equal(off, offl) and np.array_equal(win, winl)
    c = np.diff(win.astype(np.int64))
    assert c[:4].tolist() == [0, 0, 1, 1 + (1 if stride == 1 else 0)]
    assert c[4] == 3 and c[5] == 2
    # the last window of read 4 ends with the read
    assert np.array_equal(q[(int(win[5]) - 1) * W:int(win[5]) * W], reads[4][-W:])


def test_expander_on_nothing():
    q, off, win = expand(np.zeros(0, np.uint8), np.zeros(1, np.uint64), W, 1)
    assert q.size == 0 and off.tolist() == [0] and win.tolist() == [0]
    q, off, win = expand(np.zeros(3, np.uint8), np.array([0, 3], np.uint64), W, 1)
    assert q.size == 0 and off.tolist() == [0] and win.tolist() == [0, 0]


def _opts(engine, w=10, stride=1, flags=0, size=None):
    return engine.WindowOptions(C.sizeof(engine.WindowOptions) if size is None else size, w, stride, flags)


def test_window_calls_refuse_bad_arguments_without_a_device(engine):
    L = engine.lib()
    ranks = np.zeros(12, np.uint8)
    roff = np.array([0, 12], np.uint64)
    # never looked into before the refusals that do not need it; zero-filled, it reads as an index without elements, which is
    # what the last refusal (w is no element's k) needs
    dummy = C.create_string_buffer(1 << 16)
    ix = C.addressof(dummy)
    for fn, extra in ((L.kmx_search_windows, ()), (L.kmx_search_windows_device, (None,))):
        def call(index, o, out):
            return fn(index, ranks.ctypes.data, roff.ctypes.data, 1, o, *extra, out)
        out = C.c_void_p()
        assert call(None, C.byref(_opts(engine)), C.byref(out)) == INVALID
        assert call(ix, None, C.byref(out)) == INVALID
        assert call(ix, C.byref(_opts(engine)), None) == INVALID
        assert call(ix, C.byref(_opts(engine, size=12)), C.byref(out)) == INVALID
        assert b"struct_size" in L.kmx_last_error()
        assert call(ix, C.byref(_opts(engine, stride=0)), C.byref(out)) == INVALID
        assert b"stride" in L.kmx_last_error()
        for flag in (engine.SEARCH_KEEP_MASKS, engine.SEARCH_ASYNC, engine.SEARCH_REFERENCE_PLAN, 16, 1 << 31,
                     engine.SEARCH_COUNT_ONLY | engine.SEARCH_ASYNC):
            assert call(ix, C.byref(_opts(engine, flags=flag)), C.byref(out)) == INVALID
            assert b"flags" in L.kmx_last_error()
        assert call(ix, C.byref(_opts(engine, w=10, flags=engine.SEARCH_COUNT_ONLY)), C.byref(out)) == INVALID
        assert b"is not the k of an element" in L.kmx_last_error()
        assert not out.value
    assert L.kmx_result_window_offsets(None, None, None, None) == INVALID
    assert L.kmx_version() == 5


def test_header_with_window_declarations_is_c99(tmp_path):
    src = tmp_path / "windows.c"
    src.write_text('#include "kmx.h"\n'
                   "#if KMX_SEARCH_WINDOWS != 1\n#error capability macro\n#endif\n"
                   "_Static_assert(sizeof(kmx_window_options) == 16, \"four words\");\n"
                   "int use(const kmx_index* ix, const uint8_t* ranks, const uint64_t* roff, void* stream) {\n"
                   "  kmx_result* r = 0; const uint64_t* wo; const uint64_t* dwo; uint64_t nr;\n"
                   "  kmx_window_options o;\n"
                   "  o.struct_size = (uint32_t)sizeof o; o.w = 10; o.stride = 1; o.flags = KMX_SEARCH_COUNT_ONLY;\n"
                   "  if (kmx_search_windows(ix, ranks, roff, 1, &o, &r) != KMX_OK) return 1;\n"
                   "  if (kmx_search_windows_device(ix, ranks, roff, 1, &o, stream, &r) != KMX_OK) return 2;\n"
                   "  return (int)kmx_result_window_offsets(r, &wo, &dwo, &nr);\n}\n")
    res = subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Wextra", "-Werror", "-c", f"-I{os.path.join(ROOT, 'include')}",
                          str(src), "-o", str(tmp_path / "windows.o")], capture_output=True, text=True)
    assert res.returncode == 0, res.stderr
