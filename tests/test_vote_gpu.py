"""kmx_windows_vote on the GPU.  The oracle throughout is tests/vote_naive.vote applied to the host arrays of the engine's own
windows result: locus_off, diag, span, votes and skipped must be equal array for array, dtypes included, and n_votes equal."""
import functools

import numpy as np
import pytest

from kmer_index_amd import synth
from tests import chain_data
from tests.chain_checks import dev_array
from tests.chain_data import READ_WORKLOADS, text_of
from tests.helpers import pack
from tests.vote_naive import vote

pytestmark = pytest.mark.gpu

NAMES = ("locus_off", "diag", "span", "votes", "skipped")
WORKLOADS = READ_WORKLOADS              # name: (sigma, k, text length, reads)
reads_of = functools.partial(chain_data.reads_of, meta="plain")      # with (kind, s, m, plain) per read
OPTION_SETS = [(0, 1, 0), (0, 10, 0), (3, 8, 100), (0, 2, 1), (65_535, 1, 0)]      # (band, min_votes, max_occ)


@pytest.fixture(scope="module")
def indexes(engine):
    made = {}

    def get(name):
        if name not in made:
            sigma, k, n, _ = WORKLOADS[name]
            made[name] = engine.Index(text_of(sigma, n), sigma, [k], table=2)
        return made[name]
    yield get
    for idx in made.values():
        idx.close()


_windows = {}


def windows(indexes, name, stride):
    """(Result, host arrays, win_off) of the windows search of a workload, made once and shared (nothing changes them)."""
    if (name, stride) not in _windows:
        ranks, roff, _ = reads_of(name)
        r = indexes(name).search_windows(ranks, roff, WORKLOADS[name][1], stride)
        _windows[(name, stride)] = (r, r.host(), r.window_offsets())
    return _windows[(name, stride)]


@pytest.fixture(scope="module", autouse=True)
def _close_windows():
    yield
    for r, _, _ in _windows.values():
        r.close()
    _windows.clear()


def assert_same(loci, want):
    got = loci.host()
    for name, g, x in zip(NAMES, got, want[:5]):
        assert g.dtype == x.dtype and np.array_equal(g, x), name
    c = loci.counts()
    assert c["n_votes"] == want[5] and c["n_loci"] == want[1].size and c["nr"] == want[4].size
    return c


def votes_per_read(host, win, max_occ=0):
    cnt = np.diff(host[0].astype(np.int64))
    cnt = np.where((max_occ == 0) | (cnt <= max_occ), cnt, 0)
    return np.add.reduceat(np.append(cnt, 0), win[:-1].astype(np.int64)) * (np.diff(win.astype(np.int64)) > 0)


def check(r, host, win, stride, opts, loci=None):
    band, min_votes, max_occ = opts
    want = vote(host[0], host[1], win, stride, band, min_votes, max_occ)
    got = r.vote(band, min_votes, max_occ, loci=loci)
    c = assert_same(got, want)
    assert c["n_small"] + c["n_large"] == int(np.count_nonzero(votes_per_read(host, win, max_occ)))
    return got, want, c


# ---- 1. option sweeps ----------------------------------------------------------------------------------------------------------------
# floors: about half of what the generator gives (properties of the inputs, not of the code under test)
@pytest.mark.parametrize("opts", OPTION_SETS, ids=lambda o: "b%d_m%d_o%d" % o)
@pytest.mark.parametrize("stride", ["1", "3", "w", "w+3"])
@pytest.mark.parametrize("name", list(WORKLOADS))
def test_option_sweep(indexes, name, stride, opts):
    w = WORKLOADS[name][1]
    stride = {"1": 1, "3": 3, "w": w, "w+3": w + 3}[stride]
    r, host, win = windows(indexes, name, stride)
    loci, want, c = check(r, host, win, stride, opts)
    loci.close()
    off, diag, span, votes, skipped, n_votes = want
    if stride != 1:
        return
    per_read = np.diff(off.astype(np.int64))
    if opts == (0, 1, 0):
        assert host[1].size >= {"dna4_k10": 140_000, "aa20_k5": 150_000, "dna4_k5": 2_300_000}[name]
        assert diag.size >= {"dna4_k10": 9000, "aa20_k5": 4800, "dna4_k5": 1_500_000}[name]
        if name != "dna4_k5":
            assert int(np.count_nonzero((diag == -20) & (votes >= 10))) >= 30
        if name == "dna4_k10":
            assert int(np.count_nonzero((votes >= 10) & (diag + 300 > WORKLOADS[name][2]))) >= 60
        if name == "dna4_k5":
            v = votes_per_read(host, win)
            assert v.max() >= 14_000 and np.median(v) >= 7000
    if opts == (3, 8, 100):
        if name == "dna4_k5":
            assert diag.size >= 1600 and int(np.count_nonzero(skipped)) >= 148
        else:
            assert int(np.count_nonzero(span)) >= 290
    if opts == (0, 2, 1):
        if name == "dna4_k5":
            assert n_votes == 0 and diag.size == 0                          # no window has a single hit
        else:
            assert int(np.count_nonzero(skipped)) >= 850 and diag.size >= 1400
    if opts == (65_535, 1, 0):                                               # nearly every read has one locus
        assert int(np.count_nonzero(per_read == 1)) >= 0.9 * np.count_nonzero(per_read)


# ---- 2. class boundaries -------------------------------------------------------------------------------------------------------------
def test_class_boundaries_k5(indexes, monkeypatch):
    r, host, win = windows(indexes, "dna4_k5", 1)
    v_all = votes_per_read(host, win)
    voting = v_all[v_all > 0]
    v = int(np.sort(voting)[voting.size // 3])
    assert 2048 < v and np.count_nonzero(voting == v) >= 1
    assert np.count_nonzero(voting <= 2048) >= 5                             # both shapes of the small class have reads
    base = None
    for cap in (v, v - 1, 0, None):
        if cap is None:
            monkeypatch.delenv("KMX_VOTE_SMALL_CAP", raising=False)
        else:
            monkeypatch.setenv("KMX_VOTE_SMALL_CAP", str(cap))
        for opts in ((0, 1, 0), (3, 8, 100), (65_535, 2, 0)):
            loci, want, c = check(r, host, win, 1, opts)
            loci.close()
            vr = votes_per_read(host, win, opts[2])
            if cap is not None:
                assert c["n_small"] == int(np.count_nonzero((vr > 0) & (vr <= cap)))
                assert c["n_large"] == int(np.count_nonzero(vr > cap))
            elif opts[2] == 0:
                assert c["n_small"] >= 50 and c["n_large"] >= 50             # the built-in cap lies inside this workload
                base = c
    assert base is not None


def test_class_boundaries_k10(indexes, monkeypatch):
    r, host, win = windows(indexes, "dna4_k10", 1)
    vr = votes_per_read(host, win)
    monkeypatch.setenv("KMX_VOTE_SMALL_CAP", "64")
    for opts in ((0, 1, 0), (3, 8, 100), (0, 10, 0)):
        loci, want, c = check(r, host, win, 1, opts)
        loci.close()
        vo = votes_per_read(host, win, opts[2])
        assert c["n_small"] == int(np.count_nonzero((vo > 0) & (vo <= 64))) and c["n_large"] == int(np.count_nonzero(vo > 64))
        assert c["n_small"] >= 100 and c["n_large"] >= 100
    monkeypatch.delenv("KMX_VOTE_SMALL_CAP")
    loci, want, c = check(r, host, win, 1, (0, 1, 0))
    assert c["n_large"] == 0 and c["n_small"] == int(np.count_nonzero(vr))
    loci.close()


# ---- 3. against the text, not against the engine ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(WORKLOADS))
def test_reads_cut_from_the_text_find_their_place(indexes, name):
    w = WORKLOADS[name][1]
    ranks, roff, meta = reads_of(name)
    loci = indexes(name).vote_windows(ranks, roff, w)
    off, diag, span, votes, _ = loci.host()
    loci.close()
    n_checked = 0
    for i, (kind, s, m, plain) in enumerate(meta):
        if not plain or m < w:
            continue
        a, b = int(off[i]), int(off[i + 1])
        at = a + int(np.searchsorted(diag[a:b], s))
        assert at < b and diag[at] == s and span[at] == 0 and votes[at] == m - w + 1, i
        n_checked += 1
    assert n_checked >= len(meta) // 6


# ---- 4. empty and degenerate batches ---------------------------------------------------------------------------------------------------
def assert_no_loci(loci, nr, skipped=None):
    off, diag, span, votes, sk = loci.host()
    assert off.dtype == np.uint64 and off.size == nr + 1 and not off.any()
    assert diag.size == 0 and span.size == 0 and votes.size == 0 and diag.dtype == np.int64
    assert sk.dtype == np.uint32 and np.array_equal(sk, np.zeros(nr, np.uint32) if skipped is None else skipped)
    c = loci.counts()
    assert c["n_loci"] == 0 and c["nr"] == nr and c["n_small"] == 0 and c["n_large"] == 0
    return c


def test_empty_and_degenerate_batches(engine, indexes):
    idx = indexes("dna4_k10")
    loci = idx.vote_windows(np.zeros(0, np.uint8), np.zeros(1, np.uint64), 10)                  # nr = 0
    assert_no_loci(loci, 0)
    loci.close()
    ranks, roff = pack([synth.ranks(i, i % 10, 4) for i in range(500)])                         # every read shorter than w
    loci = idx.vote_windows(ranks, roff, 10)
    assert assert_no_loci(loci, 500)["n_votes"] == 0
    loci.close()
    # protein reads over the letters 10 .. 19 against a text over 0 .. 9: no 5-mer in common
    text = synth.ranks(3, 20_000, 10)
    aa = engine.Index(text, 20, [5], table=2)
    ranks, roff = pack([synth.ranks(50 + i, 30 + i % 100, 10) + 10 for i in range(400)])
    r = aa.search_windows(ranks, roff, 5)
    assert r.counts()["n_hits"] == 0 and r.counts()["nq"] > 10_000
    loci = r.vote()
    assert assert_no_loci(loci, 400)["n_votes"] == 0
    loci.close()
    r.close()
    aa.close()
    # max_occ that skips every window: DNA4 k = 5, where every window has about a hundred hits
    r, host, win = windows(indexes, "dna4_k5", 1)
    want = vote(host[0], host[1], win, 1, 0, 1, 1)
    loci = r.vote(0, 1, 1)
    assert want[5] == 0 and int(np.count_nonzero(want[4])) >= 250
    assert assert_no_loci(loci, win.size - 1, skipped=want[4])["n_votes"] == 0
    loci.close()


# ---- 5. handle reuse -----------------------------------------------------------------------------------------------------------------
def test_one_loci_handle_for_batches_of_different_sizes(indexes):
    idx = indexes("dna4_k10")
    ranks, roff, _ = reads_of("dna4_k10")
    few = pack([ranks[int(roff[i]):int(roff[i + 1])] for i in range(100, 160)])
    loci = None
    for reads in (few, (ranks, roff), few):
        r = idx.search_windows(*reads, 10)
        loci, _, _ = check(r, r.host(), r.window_offsets(), 1, (3, 2, 0), loci=loci)
        r.close()
    loci.close()


def test_voting_leaves_the_windows_result_as_it_was(indexes):
    r, host, win = windows(indexes, "dna4_k10", 3)
    for opts in ((0, 1, 0), (65_535, 1, 0), (3, 8, 1)):
        check(r, host, win, 3, opts)[0].close()
    for name, g, x in zip(("hit_off", "positions", "status", "kinds"), r.host(), host):
        assert g.dtype == x.dtype and np.array_equal(g, x), name
    assert np.array_equal(r.window_offsets(), win)


def test_vote_on_a_device_form_result_and_device_view(engine, indexes):
    import torch
    idx = indexes("dna4_k10")
    ranks, roff, _ = reads_of("dna4_k10")
    stream = torch.cuda.Stream()
    d_r = torch.from_numpy(np.array(ranks)).cuda()
    d_o = torch.from_numpy(np.array(roff).view(np.int64)).cuda()
    torch.cuda.synchronize()
    r = idx.search_windows_device(d_r.data_ptr(), d_o.data_ptr(), roff.size - 1, 10, 1, stream=stream.cuda_stream)
    loci, want, c = check(r, r.host(), r.window_offsets(), 1, (3, 2, 0))
    assert c["n_loci"] >= 5000
    # the device view, read back through torch, equals the host view
    stream.synchronize()
    ptrs = loci.device_ptrs()
    sizes = (c["nr"] + 1, c["n_loci"], c["n_loci"], c["n_loci"], c["nr"])
    for name, ptr, n, x in zip(NAMES, ptrs, sizes, want[:5]):
        got = dev_array(ptr, n, x.dtype)
        assert np.array_equal(got, x), name
    # search into the result again while the loci handle from it is alive, then read that handle
    few = pack([ranks[int(roff[i]):int(roff[i + 1])] for i in range(40)])
    r = idx.search_windows(*few, 10, result=r)
    other = r.vote(0, 1, 0)
    for name, g, x in zip(NAMES, loci.host(), want[:5]):
        assert np.array_equal(g, x), name
    assert other.counts()["nr"] == 40
    other.close()
    loci.close()
    r.close()


# ---- 6. refusals after looking at the handle -----------------------------------------------------------------------------------------------
def test_refusals_after_looking_at_the_handle(engine, indexes):
    idx = indexes("dna4_k10")
    ranks, roff, _ = reads_of("dna4_k10")
    q, off = pack([np.asarray(text_of(4, 50_000)[i * 7:i * 7 + 10]) for i in range(20_000)])   # (too many for the latency path)
    plain = idx.search(q, off)
    with pytest.raises(engine.KmxError) as e:
        plain.vote()
    assert e.value.status == 1 and "windows" in str(e.value)
    r = idx.search_windows(ranks, roff, 10, flags=engine.SEARCH_COUNT_ONLY)
    with pytest.raises(engine.KmxError) as e:
        r.vote()
    assert e.value.status == 1 and "COUNT_ONLY" in str(e.value)
    r = idx.search_windows(ranks, roff, 10, result=r)
    r.vote().close()
    for batch in ((q, off), (q[:50], off[:6])):                                # the device path and the latency path
        r = idx.search_windows(ranks, roff, 10, result=r)
        r = idx.search(*batch, result=r)
        with pytest.raises(engine.KmxError) as e:
            r.vote()
        assert e.value.status == 1
    plain.close()
    r.close()


# ---- 8. stats ----------------------------------------------------------------------------------------------------------------------
def test_stats_name(indexes):
    idx = indexes("dna4_k10")
    ranks, roff, _ = reads_of("dna4_k10")
    idx.stats_enable(True)
    idx.stats_reset()
    r = idx.search_windows(ranks, roff, 10, 7)
    before = idx.stats()
    assert before["k_vote"]["launches"] == 0 and before["k_lookup_windows"]["launches"] >= 1
    loci = r.vote(3, 2, 0)
    after = idx.stats()
    idx.stats_enable(False)
    assert after["k_vote"]["launches"] >= 1
    for name in before:
        if name != "k_vote":
            assert after[name]["launches"] == before[name]["launches"], name
    loci.close()
    r.close()
