"""The front of the mapping chain (kmx_reads_strands, kmx_search_windows(_device), kmx_windows_vote) on indexes with cells and on
batches of more than one scan tile, and the whole chain with every scan per internal read in two blocks.

The oracle never goes through the engine: tests/front_naive.hits finds the hits from the text alone, tests/vote_naive.vote votes
on THOSE hits, and tests/chain_naive.py composes the naives of every later stage; for the tiled batches of (d) the reference is
chain_naive.tile of the base batch's result (tests/test_front_cpu.py licenses that).  Every comparison is exact equality of integer
arrays, dtypes included.  The inputs and their floors live in tests/front_data.py and are checked without a device by
tests/test_front_cpu.py; the GPU tests assert the same floors again, so that none of them passes vacuously.  Untested: an index with several replicas."""
import numpy as np
import pytest

from tests import chain_naive as chn
from tests.chain_checks import close_all, dev_array, same
from tests.chain_data import COMPLEMENT, HITS, LOCI
from tests.front_data import (C_DIRECT, C_LAYOUT, C_OPTS, C_PUBLIC, D_CHAIN, D_INSERT, D_LAYOUT, D_PAIR_STRIDE, D_PAIRS, D_TILES, LAYOUTS, LETTERS, OPTION_SETS,
                              SCAN_TILE, chain_d, floors_a, floors_b, floors_c, floors_d, internal_c, layout_text, naive_hits, naive_vote, pairs_d, public_c,
                              reads_a, reads_b, votes_per_read)

pytestmark = pytest.mark.gpu

@pytest.fixture(scope="module")
def indexes(engine):
    """every index with the default table argument, its layout asserted when it is made"""
    made = {}

    def get(name):
        if name not in made:
            sigma, k, n, shift, atab = LAYOUTS[name]
            idx = made[name] = engine.Index(layout_text(name), sigma, [k])
            paths, mem = idx.paths(), idx.memory()
            assert idx.info()["tables"] == [engine.TABLE_DENSE] and paths["scan_tile"] == SCAN_TILE
            assert paths["cell_shift"][0] == shift and (mem["cells"] != 0) == (shift != 0) and (mem["aligned_copy"] != 0) == atab
        return made[name]
    yield get
    for idx in made.values():
        idx.close()


class Uploaded:
    """a batch in device memory and a torch stream to search it on"""

    def __init__(self, ranks, roff):
        import torch

        self.nr = roff.size - 1
        self.ranks = torch.from_numpy(np.array(ranks) if ranks.size else np.zeros(16, np.uint8)).cuda()
        self.roff = torch.from_numpy(np.array(roff).view(np.int64)).cuda()
        self.stream = torch.cuda.Stream()
        torch.cuda.synchronize()

    def search(self, idx, w, stride, result=None):
        return idx.search_windows_device(self.ranks.data_ptr(), self.roff.data_ptr(), self.nr, w, stride, stream=self.stream.cuda_stream, result=result)


def check_hits(r, want):
    hit_off, positions, status, _ = r.host()
    same(HITS, (r.window_offsets(), hit_off, positions, status), want)


def check_vote(r, want_hits, stride, opts, want, loci=None):
    """kmx_windows_vote on a windows result against vote_naive on the NAIVE hits; returns (the Loci, its counts)"""
    loci = r.vote(*opts, loci=loci)
    same(LOCI, loci.host(), want[:5])
    c = loci.counts()
    assert (c["n_votes"], c["n_loci"], c["nr"]) == (want[5], want[1].size, want[4].size)
    assert c["n_small"] + c["n_large"] == int(np.count_nonzero(votes_per_read(want_hits[1], want_hits[0], opts[2])))
    return loci, c


# ---- (a) every layout, both forms ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("stride", [1, 3])
@pytest.mark.parametrize("name", list(LAYOUTS))
@pytest.mark.parametrize("form", ["host", "device"])
def test_layouts(indexes, form, name, stride):
    idx, k = indexes(name), LAYOUTS[name][1]
    floors_a(name, stride)
    want = naive_hits(name, "a", stride)
    if form == "host":
        r = idx.search_windows(*reads_a(name), k, stride)
    else:
        up = Uploaded(*reads_a(name))
        r = up.search(idx, k, stride)
    try:
        check_hits(r, want)
        for opts in OPTION_SETS:
            loci, c = check_vote(r, want, stride, opts, naive_vote(name, "a", stride, opts))
            loci.close()
            assert c["n_loci"] >= 100
    finally:
        r.close()


# ---- (b) both shapes of the small class and the large class at real vote counts, device form --------------------------------------------
@pytest.mark.parametrize("name,cap", [("dna4_k6_s4", None), ("dna4_k6_s5", None), ("dna4_k6_s4", 512)])
def test_vote_shapes_behind_the_device_form(indexes, monkeypatch, name, cap):
    idx, k = indexes(name), LAYOUTS[name][1]
    floors_b(name)
    want = naive_hits(name, "b")
    if cap is not None:
        monkeypatch.setenv("KMX_VOTE_SMALL_CAP", str(cap))
    up = Uploaded(*reads_b(name))
    r = up.search(idx, k, 1)
    try:
        check_hits(r, want)
        for opts in OPTION_SETS:
            loci, c = check_vote(r, want, 1, opts, naive_vote(name, "b", 1, opts))
            loci.close()
            v = votes_per_read(want[1], want[0], opts[2])
            if cap is None:
                assert c["n_large"] == 0 and c["n_small"] >= 500
            else:
                assert c["n_small"] == int(np.count_nonzero((v > 0) & (v <= cap))) and c["n_large"] == int(np.count_nonzero(v > cap)) >= 100
    finally:
        r.close()


# ---- (c) read counts around and beyond one scan tile ------------------------------------------------------------------------------------
class BatchC:
    """The windows search and the vote of the first nr2 internal reads, checked: an even number through kmx_reads_strands on the
    public reads and on the stream of its handle, an odd number as a device-form batch of its own.  `result` and `loci` reuse
    handles; the batch owns the stream they were filled on, so close() comes after theirs."""

    def __init__(self, idx, nr2, result=None, loci=None):
        floors_c(nr2)
        want = naive_hits(C_LAYOUT, ("c", nr2))
        self.reads = self.result = self.loci = None
        if nr2 % 2 == 0:
            ranks, roff = public_c()
            self.reads = idx.strand_reads(ranks[:int(roff[nr2 // 2])], roff[:nr2 // 2 + 1], np.asarray(COMPLEMENT[4], np.uint8))
            d_ranks2, d_roff2, n, stream = self.reads.device_ptrs()
            assert n == nr2
            want_reads = internal_c(nr2)
            same(("ranks2", "roff2"), (dev_array(d_ranks2, want_reads[0].size, np.uint8), dev_array(d_roff2, nr2 + 1, np.uint64)), want_reads)
            self.result = idx.search_windows_device(d_ranks2, d_roff2, nr2, 6, 1, stream=stream, result=result)
        else:
            self.up = Uploaded(*internal_c(nr2))
            self.result = self.up.search(idx, 6, 1, result=result)
        check_hits(self.result, want)
        self.loci, _ = check_vote(self.result, want, 1, C_OPTS, naive_vote(C_LAYOUT, ("c", nr2), 1, C_OPTS), loci=loci)

    def close(self):
        if self.reads is not None:
            self.reads.close()
            self.reads = None


@pytest.mark.parametrize("nr2", sorted(C_DIRECT + tuple(2 * x for x in C_PUBLIC)))
def test_read_counts_around_and_beyond_one_scan_tile(indexes, nr2):
    b = BatchC(indexes(C_LAYOUT), nr2)
    b.loci.close()
    b.result.close()
    b.close()


def test_one_result_and_one_loci_handle_through_small_large_small(indexes):
    r = loci = None
    done = []
    try:
        for nr2 in (4095, 8193, 4097, 4096):
            b = BatchC(indexes(C_LAYOUT), nr2, result=r, loci=loci)
            done.append(b)
            r, loci = b.result, b.loci
    finally:
        for h in (loci, r):
            if h is not None:
                h.close()
        for b in done:
            b.close()


# ---- (d) the whole chain on a tiled batch -------------------------------------------------------------------------------------------------
def host_of(h, kind):
    """the arrays of a handle in the form of a chain_naive.Stage"""
    if kind == "reads":
        d_ranks2, d_roff2, nr2, _ = h.device_ptrs()
        roff2 = dev_array(d_roff2, nr2 + 1, np.uint64)
        return dev_array(d_ranks2, int(roff2[-1]), np.uint8), roff2
    return (h.host(),) if kind == "mapq" else h.host()


def check_chain(out, want):
    """every handle of a chain call against the stages of the oracle: arrays, dtypes and totals"""
    assert len(out) == len(want)
    for h, w in zip(out, want):
        pairs = zip(h, w) if isinstance(w, chn.Tags) else [(h, w)]
        for hh, s in pairs:
            assert (hh is None) == (s is None)
            if s is None:
                continue
            got = host_of(hh, s.kind)
            assert len(got) == len(s.arrays), s.kind
            for i, (g, x) in enumerate(zip(got, s.arrays)):
                assert (g is None) == (x is None), (s.kind, i)
                if x is not None:
                    assert g.dtype == x.dtype and np.array_equal(g, x), (s.kind, i)
            if s.totals:
                c = hh.counts()
                assert {k: c[k] for k in s.totals} == s.totals, s.kind


@pytest.mark.parametrize("kind", ["strands", "pairs"])
def test_the_whole_chain_on_a_tiled_batch(engine, indexes, kind):
    idx = indexes(D_LAYOUT)
    floors_d()
    want = chn.tile(chain_d(kind), D_TILES)
    ranks, roff = chn.tile_reads(*pairs_d(), D_TILES)
    assert 2 * (roff.size - 1) == 4 * D_PAIRS * D_TILES > SCAN_TILE
    comp = np.asarray(COMPLEMENT[4], np.uint8)
    if kind == "strands":
        out = idx.map_reads_strands(ranks, roff, 6, comp, **D_CHAIN, scripts=True, tags=True, letters=LETTERS, secondaries=2, clip={})
    else:
        out = idx.map_pairs(ranks, roff, 6, comp, **D_INSERT, stride=D_PAIR_STRIDE, **D_CHAIN, rescue=True, tags=True, letters=LETTERS)
    try:
        check_chain(out, want)
    finally:
        close_all(list(out))
