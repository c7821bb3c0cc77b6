"""kmx_search_windows / kmx_search_windows_device on the GPU.  The oracle throughout is the engine itself on the expanded batch
(tests/windows_naive.py writes every window out as a query of its own): hit_off, positions, status and kinds must be equal
array for array, win_off equal to the expander's."""
import functools

import numpy as np
import pytest

from kmer_index_amd import synth
from tests.chain_data import text_of
from tests.helpers import make_queries, pack
from tests.windows_naive import expand

pytestmark = pytest.mark.gpu

N_TEXT = 50_000
N_READS = 3_000


@functools.lru_cache(maxsize=None)
def window_reads(sigma, n=N_TEXT, n_reads=N_READS, seed=1):
    """About n_reads reads of 0 .. 300 letters: every second one cut from the text (every 25th of those ends with the text's
    last letter), the others random; every 50th read (2 %) carries a letter >= sigma — sigma or 255 in turn — at its first
    letter, its last letter or in its middle in turn, so that it enters and leaves rolling windows."""
    text = text_of(sigma, n)
    z = synth.u64_stream(seed * 7919 + sigma, 3 * n_reads).astype(np.int64) & 0x7FFFFFFF
    reads = []
    n_bad = 0
    for i in range(n_reads):
        m = int(z[3 * i] % 301)
        if i < 500:
            m = max(m, 60)                                   # the issue's floor: 500 planted reads of 60 letters or more
        if i % 2 == 0 or i < 500:
            s = n - m if (i // 2) % 25 == 0 else int(z[3 * i + 1] % (n - m + 1))
            q = text[s:s + m].copy()
        else:
            q = synth.ranks(seed * 1000003 + i, m, sigma)
        if i % 50 == 7 and m > 0:
            q[(0, m - 1, m // 2)[n_bad % 3]] = (sigma, 255)[(n_bad // 3) % 2]
            n_bad += 1
        reads.append(q)
    ranks, roff = pack(reads)
    ranks.setflags(write=False)
    roff.setflags(write=False)
    return ranks, roff


def reference(idx, ranks, roff, w, stride, flags=0):
    q, off, win = expand(ranks, roff, w, stride)
    return idx.search(q, off, flags=flags).host(), win


def assert_equal(got, want):
    for name, g, x in zip(("hit_off", "positions", "status", "kinds"), got, want):
        assert g.dtype == x.dtype and np.array_equal(g, x), name


def check(engine, idx, ranks, roff, w, stride, result=None):
    want, win = reference(idx, ranks, roff, w, stride)
    r = idx.search_windows(ranks, roff, w, stride, result=result)
    assert_equal(r.host(), want)
    assert np.array_equal(r.window_offsets(), win)
    p = r.paths()
    assert p["lookup_items"] == 0 and not p["lookup_pairs"] and not p["small"]
    assert p["prefix_plain"] + p["prefix_small"] + p["prefix_merge_small"] + p["prefix_mid"] + p["prefix_long"] == 0
    return want, r


def assert_not_vacuous(engine, want, every_key_occurs=False):
    hit_off, _, status, kinds = want
    cnt = np.diff(hit_off.astype(np.int64))
    assert int(np.count_nonzero(cnt)) >= 1000
    if not every_key_occurs:
        assert int(np.count_nonzero((cnt == 0) & (status == engine.Q_OK))) >= 1000
    assert int(np.count_nonzero(status == engine.Q_BAD_RANK)) >= 10
    assert set(np.unique(status).tolist()) <= {engine.Q_OK, engine.Q_BAD_RANK}
    assert set(np.unique(kinds).tolist()) <= {engine.KIND_NONE, engine.KIND_EXACT}


# ---- 1. every table layout probe() has -------------------------------------------------------------------------------------
# (sigma, k, text length, Index keywords, layout).  Protein k = 5 gets cells only once the key space (3.2e6 keys of 8 positions)
# is at most 8 times the positions, hence the longer text; protein at 50 000 letters is a plain dense table and runs as such.
LAYOUTS = {
    "dna4_k10_dense": (4, 10, N_TEXT, dict(table=2), "plain"),
    "dna4_k10_no_aligned_copy": (4, 10, N_TEXT, dict(table=2, aligned_copy=False), "plain"),
    "dna4_k5_atab": (4, 5, 100_000, dict(table=2), "atab"),
    "aa20_k5_cells": (20, 5, 3_500_000, dict(table=2), "cells"),
    "aa20_k5_short_text": (20, 5, N_TEXT, dict(table=2), "plain"),
    "dna4_k10_open": (4, 10, N_TEXT, dict(table=1), "open"),
}


@pytest.mark.parametrize("name", list(LAYOUTS))
def test_every_table_layout(engine, name):
    sigma, k, n, kw, layout = LAYOUTS[name]
    idx = engine.Index(text_of(sigma, n), sigma, [k], **kw)
    info, paths, mem = idx.info(), idx.paths(), idx.memory()
    assert info["tables"] == [engine.TABLE_OPEN if layout == "open" else engine.TABLE_DENSE]
    assert (paths["cell_shift"][0] != 0) == (layout == "cells") and (mem["cells"] != 0) == (layout == "cells")
    assert (mem["aligned_copy"] != 0) == (layout == "atab")
    ranks, roff = window_reads(sigma, n)
    for stride in (1, 3):
        want, _ = check(engine, idx, ranks, roff, k, stride)
        # DNA4 k = 5 has 1 024 keys for 100 000 letters: every key occurs, no valid window is without a hit
        assert_not_vacuous(engine, want, every_key_occurs=(name == "dna4_k5_atab"))
    idx.close()


# ---- 2. hash width: 62-bit hashes, the rolling update must neither wrap nor subtract after the multiply ---------------------
@pytest.mark.parametrize("sigma,k", [(4, 31), (5, 27)])
def test_wide_hashes(engine, sigma, k):
    idx = engine.Index(text_of(sigma), sigma, [k])
    assert idx.info()["tables"] == [engine.TABLE_OPEN]
    ranks, roff = window_reads(sigma)
    for stride in (1, 3):
        want, _ = check(engine, idx, ranks, roff, k, stride)
        assert_not_vacuous(engine, want)
    idx.close()


# ---- 3. multi-k ------------------------------------------------------------------------------------------------------------
def test_multi_k_index(engine):
    idx = engine.Index(text_of(4), 4, [8, 10, 12])
    ranks, roff = window_reads(4)
    for w in (8, 10, 12):
        want, _ = check(engine, idx, ranks, roff, w, 1)
        assert_not_vacuous(engine, want)
    with pytest.raises(engine.KmxError) as e:
        idx.search_windows(ranks, roff, 9)
    assert e.value.status == 1
    idx.close()


# ---- 4. strides ------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def dna10(engine):
    idx = engine.Index(text_of(4), 4, [10], table=2)
    yield idx
    idx.close()


@pytest.mark.parametrize("stride", [1, 2, 9, 10, 13, 301])
def test_strides(engine, dna10, stride):
    ranks, roff = window_reads(4)
    want, r = check(engine, dna10, ranks, roff, 10, stride)
    if stride == 301:                                        # larger than every read: one window per read of 10 letters or more
        lens = np.diff(roff.astype(np.int64))
        assert r.counts()["nq"] == int(np.count_nonzero(lens >= 10))
    else:
        assert_not_vacuous(engine, want)


def test_no_windows_at_all(engine, dna10):
    ranks, roff = pack([synth.ranks(i, i % 10, 4) for i in range(500)])      # only reads that are too short
    r = dna10.search_windows(ranks, roff, 10)
    hit_off, pos, st, kinds = r.host()
    assert r.counts()["nq"] == 0 and hit_off.tolist() == [0] and pos.size == 0 and st.size == 0 and kinds.size == 0
    assert np.array_equal(r.window_offsets(), np.zeros(501, np.uint64))
    r = dna10.search_windows(np.zeros(0, np.uint8), np.zeros(1, np.uint64), 10, result=r)      # nr == 0
    assert r.counts()["nq"] == 0 and r.host()[0].tolist() == [0] and r.window_offsets().tolist() == [0]
    # ... and the handle serves a real batch afterwards
    check(engine, dna10, *window_reads(4), 10, 1, result=r)


# ---- 5. tile edges ---------------------------------------------------------------------------------------------------------
def planted(text, m, at):
    return text[at:at + m].copy()


def test_tile_edges(engine, dna10):
    T, w = dna10.paths()["windows_tile"], 10
    assert T > 0 and dna10.paths()["scan_tile"] % T == 0
    text = text_of(4)
    for d in (-1, 0, 1):                                     # one read of exactly T windows, one fewer, one more
        check(engine, dna10, *pack([planted(text, T + w - 1 + d, 100)]), w, 1)
    check(engine, dna10, *pack([planted(text, 5 * T + w - 1, 300)]), w, 1)
    check(engine, dna10, *pack([planted(text, w, 37 * i) for i in range(T)]), w, 1)
    check(engine, dna10, *pack([planted(text, w, 37 * i) for i in range(T + 1)]), w, 1)
    # a read whose windows straddle the tile boundary, a letter outside the alphabet in the windows on either side of it:
    # the last letter of window T - 1, the first letter of window T, the last letter of window T; with reads in front so
    # that the boundary falls into the read's middle, and with stride 3
    for at in (T - 1 + w - 1, T, T + w - 1):
        long_read = planted(text, T + 200, 1000)
        long_read[at] = 4 if at % 2 else 255
        want, _ = check(engine, dna10, *pack([long_read]), w, 1)
        assert np.count_nonzero(want[2] == engine.Q_BAD_RANK) == w
        front = [planted(text, 57, 10), np.zeros(0, np.uint8), planted(text, 9, 5)]      # 48 windows, then reads without one
        shifted = planted(text, T + 200, 2000)
        shifted[at - 48] = 4
        check(engine, dna10, *pack(front + [shifted, planted(text, 30, 0)]), w, 1)
        strided = planted(text, 3 * T + 200, 3000)
        strided[3 * (at - w + 1) + w - 1] = 255
        check(engine, dna10, *pack([strided]), w, 3)


# ---- 6. count only ---------------------------------------------------------------------------------------------------------
def test_count_only(engine, dna10):
    ranks, roff = window_reads(4)
    want, win = reference(dna10, ranks, roff, 10, 1, flags=engine.SEARCH_COUNT_ONLY)
    r = dna10.search_windows(ranks, roff, 10, 1, flags=engine.SEARCH_COUNT_ONLY)
    got = r.host()
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[2], want[2]) and np.array_equal(got[3], want[3])
    assert r.counts() == dna10.search(*expand(ranks, roff, 10, 1)[:2], flags=engine.SEARCH_COUNT_ONLY).counts()
    assert np.array_equal(r.window_offsets(), win)
    full = dna10.search_windows(ranks, roff, 10, 1)
    assert np.array_equal(full.host()[0], got[0]) and full.counts() == r.counts()


# ---- 7. device form, one handle shared with kmx_search_batch_device ----------------------------------------------------------
def test_device_form_and_handle_reuse(engine):
    import torch
    idx = engine.Index(text_of(4), 4, [8, 10, 12])
    text = text_of(4)
    stream = torch.cuda.Stream()

    def up(a, dtype):
        a = np.array(a, dtype)                               # (a writable copy: the fixtures are read-only)
        return torch.from_numpy(a.view(np.int64) if dtype == np.uint64 else a).cuda() if a.size else torch.zeros(16, dtype=torch.uint8).cuda()

    def windows(reads, w, stride, res):
        ranks, roff = reads
        d_r, d_o = up(ranks, np.uint8), up(roff, np.uint64)
        torch.cuda.synchronize()
        r = idx.search_windows_device(d_r.data_ptr(), d_o.data_ptr(), roff.size - 1, w, stride, stream=stream.cuda_stream, result=res)
        want, win = reference(idx, ranks, roff, w, stride)
        assert_equal(r.host(), want)
        host_win, d_win, nr = r.window_offsets(device=True)
        assert nr == roff.size - 1 and np.array_equal(host_win, win)
        dev = torch.empty(nr + 1, dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()
        engine_copy(torch, dev, d_win, (nr + 1) * 8)
        assert np.array_equal(dev.cpu().numpy().view(np.uint64), win)
        return r

    ranks, roff = window_reads(4)
    some = pack([ranks[int(roff[i]):int(roff[i + 1])] for i in range(0, 1200)])
    few = pack([ranks[int(roff[i]):int(roff[i + 1])] for i in range(1200, 1500)])
    r = windows(some, 10, 1, None)
    # an unrelated mixed batch through kmx_search_batch_device on the same handle: sub-k, exact, stitch and multi-k lengths
    q, off = make_queries(text, 4, [3, 7, 8, 10, 12, 15, 20, 24, 31], 400, 5)
    d_q, d_o = up(q, np.uint8), up(off, np.uint64)
    torch.cuda.synchronize()
    r = idx.search_device(d_q.data_ptr(), d_o.data_ptr(), off.size - 1, stream=stream.cuda_stream, result=r)
    mixed = r.host()
    assert_equal(mixed, idx.search(q, off).host())
    assert {engine.KIND_STITCH, engine.KIND_PREFIX, engine.KIND_EXACT} <= set(np.unique(mixed[3]).tolist())
    with pytest.raises(engine.KmxError) as e:
        r.window_offsets()
    assert e.value.status == 1
    r = windows((ranks, roff), 12, 1, r)                      # larger
    r = windows(few, 8, 2, r)                                 # smaller
    r.close()
    idx.close()


def engine_copy(torch, dst, src_ptr, nbytes):
    """Device-to-device copy from a raw pointer into a torch tensor."""
    class _Arr:
        def __init__(self, ptr, n):
            self.__cuda_array_interface__ = {"shape": (int(n),), "typestr": "<i8", "data": (int(ptr), False), "version": 2}
    dst.copy_(torch.as_tensor(_Arr(src_ptr, nbytes // 8), device="cuda"))
    torch.cuda.synchronize()


# ---- 8. stats --------------------------------------------------------------------------------------------------------------
def test_stats_name(engine, dna10):
    ranks, roff = window_reads(4)
    dna10.stats_enable(True)
    dna10.stats_reset()
    dna10.search(*expand(ranks, roff, 10, 7)[:2])
    before = dna10.stats()
    assert before["k_lookup"]["launches"] >= 1 and before["k_lookup_windows"]["launches"] == 0
    dna10.search_windows(ranks, roff, 10, 7)
    after = dna10.stats()
    dna10.stats_enable(False)
    assert after["k_lookup_windows"]["launches"] >= 1
    assert after["k_lookup"]["launches"] == before["k_lookup"]["launches"]
