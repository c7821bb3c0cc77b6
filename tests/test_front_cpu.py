"""The oracles of tests/test_front_gpu.py, checked without a device: front_naive.hits against the definition window by window,
chain_naive.tile against the chain on the tiled batch itself (what licenses the tiled reference of the GPU tests), and the floors
of every input of the GPU tests, so that none of them can pass vacuously."""
import numpy as np
import pytest

from kmer_index_amd import synth
from tests import chain_naive as chn
from tests import front_data as fd
from tests import front_naive as frn
from tests import vote_naive as vn
from tests import windows_naive as wn
from tests.chain_checks import same
from tests.chain_data import COMPLEMENT, HITS, LOCI
from tests.helpers import pack


# ---- 1. front_naive.hits against the definition -----------------------------------------------------------------------------------------
def tiny_case(seed):
    """(text, sigma, ranks, roff, w): a text of 5 .. 60 letters over 2 .. 5 letters, w = 1 .. 4, and a dozen reads: cut from the
    text, random, of no letter, of fewer than w letters, and with a letter equal to sigma or 255 at the first, the middle or the last
    letter"""
    z = synth.u64_stream(3000 + seed, 8).astype(np.int64) & 0x7FFFFFFF
    n, sigma, w = 5 + int(z[0] % 56), 2 + int(z[1] % 4), 1 + int(z[2] % 4)
    text = synth.ranks(4000 + seed, n, sigma)
    reads = [np.zeros(0, np.uint8), text[:max(w - 1, 0)].copy(), text.copy(), text[n - min(n, w):].copy()]
    for i in range(9):
        m = int((z[3] >> i) % 13)
        if i % 2 and m <= n:
            s = int((z[4] >> i) % (n - m + 1))
            q = text[s:s + m].copy()
        else:
            q = synth.ranks(5000 + 16 * seed + i, m, sigma)
        if i >= 3 and m:
            q[(0, m // 2, m - 1)[i % 3]] = (sigma, 255)[(i // 3) % 2]
        reads.append(q)
    return (text, sigma) + pack(reads) + (w,)


@pytest.mark.parametrize("block", range(6))
def test_hits_equal_the_definition_on_tiny_cases(block):
    n_bad = n_hits = n_short = 0
    for seed in range(50 * block, 50 * block + 50):
        text, sigma, ranks, roff, w = tiny_case(seed)
        for stride in sorted({1, 2, w, w + 1}):
            got = frn.hits(text, sigma, ranks, roff, w, stride)
            same(HITS, got, frn.hits_loop(text, sigma, ranks, roff, w, stride))
            assert np.array_equal(np.diff(got[0].astype(np.int64)), wn.window_counts(roff, w, stride))
            n_bad += int((got[3] == frn.Q_BAD_RANK).sum())
            n_hits += got[2].size
            n_short += int(np.count_nonzero(np.diff(roff.astype(np.int64)) < w))
    assert n_bad >= 100 and n_hits >= 1000 and n_short >= 100


def test_hits_on_a_text_with_a_letter_outside_the_alphabet_and_on_no_reads():
    text = np.asarray([0, 1, 4, 0, 1, 0, 1], np.uint8)
    ranks, roff = pack([np.asarray([0, 1, 0, 1], np.uint8)])
    got = frn.hits(text, 4, ranks, roff, 2, 1)
    same(HITS, got, frn.hits_loop(text, 4, ranks, roff, 2, 1))
    assert got[2].tolist() == [0, 3, 5, 4, 0, 3, 5]
    empty = frn.hits(text, 4, np.zeros(0, np.uint8), np.zeros(1, np.uint64), 2, 1)
    assert [a.tolist() for a in empty] == [[0], [0], [], []]
    same(HITS, empty, frn.hits_loop(text, 4, np.zeros(0, np.uint8), np.zeros(1, np.uint64), 2, 1))


def test_window_offsets_equal_windows_naive_on_the_inputs_of_the_gpu_tests():
    for name, batch, w in (("dna4_k6_s3", "a", 6), ("dna5_k5_s4", "a", 5), (fd.C_LAYOUT, ("c", 4097), 6)):
        ranks, roff = fd.BATCHES[batch](name)
        for stride in (1, 3):
            win_off = frn.window_starts(roff, w, stride)[0]
            assert np.array_equal(win_off, wn.expand_loop(ranks, roff, w, stride)[2].astype(np.int64))


# ---- 2. the licence of the tiled reference ------------------------------------------------------------------------------------------------
def check_tiled(base, tiled):
    assert len(base) == len(tiled)
    for b, t in zip(base, tiled):
        for sb, st in (zip(b, t) if isinstance(b, chn.Tags) else [(b, t)]):
            assert (sb is None) == (st is None)
            if sb is None:
                continue
            assert sb.kind == st.kind and sb.totals == st.totals, sb.kind
            assert len(sb.arrays) == len(st.arrays) == len(chn.SPEC[sb.kind]), sb.kind
            for i, (x, y) in enumerate(zip(sb.arrays, st.arrays)):
                assert (x is None) == (y is None)
                if x is not None:
                    assert x.dtype == y.dtype and np.array_equal(x, y), (sb.kind, i)


@pytest.fixture(scope="module")
def forty_pairs():
    ranks, roff = fd.pairs_d()
    return ranks[:int(roff[80])], roff[:81]


def test_tile_of_the_chain_equals_the_chain_of_the_tiled_batch(forty_pairs):
    text, comp = fd.layout_text(fd.D_LAYOUT), COMPLEMENT[4]
    twice = chn.tile_reads(*forty_pairs, 2)
    assert twice[1].size == 161 and np.array_equal(twice[0][:twice[0].size // 2], twice[0][twice[0].size // 2:])
    kw = dict(fd.D_CHAIN, secondaries=2, clip={})
    base = chn.strands(text, 4, *forty_pairs, 6, comp, fd.LETTERS, **kw)
    check_tiled(chn.tile(base, 2), chn.strands(text, 4, *twice, 6, comp, fd.LETTERS, **kw))
    assert base[3].totals["n_placed"] >= 50 and base[6].kind == "secondaries" and base[7].totals["n_sel"] >= 50
    kw = dict(fd.D_INSERT, stride=fd.D_PAIR_STRIDE, **fd.D_CHAIN)
    base = chn.pairs(text, 4, *forty_pairs, 6, comp, fd.LETTERS, **kw)
    check_tiled(chn.tile(base, 2), chn.pairs(text, 4, *twice, 6, comp, fd.LETTERS, **kw))
    # the tiling moved something in every kind of index: loci, internal reads and jobs
    assert base[6].totals["n_taken"] >= 2 and base[7].rescue_scripts.arrays[1].size >= 2 and base[5].arrays[1].size >= 50
    # and one copy is the base itself
    check_tiled(chn.tile(base, 1), base)


def test_the_front_of_the_chain_is_front_naive_and_vote_naive(forty_pairs):
    text = fd.layout_text(fd.D_LAYOUT)
    reads, loci, al = chn._front(text, 4, *forty_pairs, 6, COMPLEMENT[4], 1, 4, 10, 0, 6, 64)
    win_off, hit_off, positions, _ = frn.hits(text, 4, *reads.arrays, 6, 1)
    same(LOCI, loci.arrays, vn.vote(hit_off, positions, win_off, 1, 4, 10, 0)[:5])
    assert loci.totals["n_loci"] >= 50 and al.totals["n_aligned"] >= 50      # 80 reads, about nine in ten cut from the text


# ---- 3. the floors of the GPU tests' inputs -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("stride", [1, 3])
@pytest.mark.parametrize("name", list(fd.LAYOUTS))
def test_floors_of_the_layout_reads(name, stride):
    fd.floors_a(name, stride)
    sigma, k, n, shift, atab = fd.LAYOUTS[name]
    # the layout rules of the index, restated on the text's histogram (the GPU tests assert the layout the index reports)
    code, _ = frn._codes(fd.layout_text(name), sigma, k)
    npos, n_keys, present = code.size, sigma ** k, np.unique(code).size
    c = npos / n_keys
    assert n_keys <= 4 * npos                                  # the automatic table is the dense one
    assert atab == (npos >= 32 * present)
    assert shift == (0 if atab else 3 if c <= 3.5 else 4 if c <= 10.5 else 5 if c <= 24 else 0)
    assert not shift or (n_keys << shift) <= 8 * npos
    # every vote option set leaves loci to compare, and the max_occ of the third skips windows on the layouts with long buckets
    for opts in fd.OPTION_SETS:
        want = fd.naive_vote(name, "a", stride, opts)
        assert want[1].size >= 100


@pytest.mark.parametrize("name", ["dna4_k6_s4", "dna4_k6_s5"])
def test_floors_of_the_vote_shape_reads(name):
    fd.floors_b(name)


@pytest.mark.parametrize("nr2", sorted(fd.C_DIRECT + tuple(2 * x for x in fd.C_PUBLIC)))
def test_floors_of_the_scan_tile_batches(nr2):
    fd.floors_c(nr2)
    assert sorted(fd.C_DIRECT + tuple(2 * x for x in fd.C_PUBLIC)) == [4095, 4096, 4097, 4098, 8193]


def test_floors_of_the_chain_batch():
    fd.floors_d()
