"""kmx_loci_align on the GPU.  The oracle throughout is tests/align_naive.align applied to the host arrays of the engine's own loci:
dist, start, end, best and aligned must be equal array for array, dtypes included, and the counts equal."""
import functools

import numpy as np
import pytest

from kmer_index_amd import synth
from tests.align_naive import MAX_READ, NO_BEST, NONE, SKIPPED, align
from tests import chain_data
from tests.chain_checks import dev_array
from tests.chain_data import N_READS, READ_WORKLOADS, text_of
from tests.helpers import pack

pytestmark = pytest.mark.gpu

NAMES = ("dist", "start", "end", "best", "aligned")
WORKLOADS = {name: READ_WORKLOADS[name] for name in ("dna4_k10", "aa20_k5")}      # (sigma, k, text length, reads of the generator)
reads_of = functools.partial(chain_data.reads_of, n_reads=N_READS, meta="bad")      # the first N_READS, with (kind, s, m, plain, bad) per read
VOTE = (8, 2, 0)                  # (band, min_votes, max_occ)
MAX_SPAN = 64


class Work:
    """Indexes, windows results, loci and oracle results, made once and shared (nothing changes them)."""

    def __init__(self, engine):
        self.engine = engine
        self.indexes, self.results, self.loci_of, self.oracles, self.runs = {}, {}, {}, {}, {}

    def index(self, name):
        if name not in self.indexes:
            sigma, k, n, _ = WORKLOADS[name]
            self.indexes[name] = self.engine.Index(text_of(sigma, n), sigma, [k], table=2)
        return self.indexes[name]

    def windows(self, name):
        if name not in self.results:
            ranks, roff, _ = reads_of(name)
            self.results[name] = self.index(name).search_windows(ranks, roff, WORKLOADS[name][1], 1)
        return self.results[name]

    def loci(self, name, vote=VOTE):
        """(Loci, its host arrays)"""
        if (name, vote) not in self.loci_of:
            l = self.windows(name).vote(*vote)
            self.loci_of[(name, vote)] = (l, l.host())
        return self.loci_of[(name, vote)]

    def oracle(self, name, E, vote=VOTE, max_span=MAX_SPAN):
        key = (name, E, vote, max_span)
        if key not in self.oracles:
            sigma, _, n, _ = WORKLOADS[name]
            ranks, roff, _ = reads_of(name)
            off, diag, span, _, _ = self.loci(name, vote)[1]
            self.oracles[key] = align(text_of(sigma, n), ranks, roff, off, diag, span, E, max_span, sigma)
        return self.oracles[key]

    def run(self, name, E, vote=VOTE, max_span=MAX_SPAN):
        """(host arrays, counts) of the engine's alignment of the whole workload"""
        key = (name, E, vote, max_span)
        if key not in self.runs:
            ranks, roff, _ = reads_of(name)
            a = self.loci(name, vote)[0].align(self.index(name), ranks, roff, E, max_span)
            self.runs[key] = (a.host(), a.counts())
            a.close()
        return self.runs[key]

    def close(self):
        for l, _ in self.loci_of.values():
            l.close()
        for r in self.results.values():
            r.close()
        for idx in self.indexes.values():
            idx.close()


@pytest.fixture(scope="module")
def work(engine):
    w = Work(engine)
    yield w
    w.close()


def assert_same(got, counts, want, n_loci):
    for name, g, x in zip(NAMES, got, want):
        assert g.dtype == x.dtype and g.shape == x.shape, name
        bad = np.flatnonzero(g != x)
        assert bad.size == 0, (name, bad[:5], g[bad[:5]], x[bad[:5]])
    assert counts["n_loci"] == n_loci == want[0].size and counts["nr"] == want[3].size
    assert counts["n_aligned"] == int(want[4].sum()) and counts["n_skipped"] == int(np.count_nonzero(want[0] == SKIPPED))


# ---- 1. sweep ------------------------------------------------------------------------------------------------------------------------
# floors: half of what the generator gives (properties of the inputs, not of the code under test)
@pytest.mark.parametrize("E", [0, 1, 8, 24])
@pytest.mark.parametrize("name", list(WORKLOADS))
def test_sweep(work, name, E):
    sigma, k, n, _ = WORKLOADS[name]
    ranks, roff, meta = reads_of(name)
    off, diag, span, _, _ = work.loci(name)[1]
    got, counts = work.run(name, E)
    want = work.oracle(name, E)
    print(name, E, counts)
    assert_same(got, counts, want, diag.size)
    dist, start, end, best, aligned = want
    ok = dist <= E
    assert counts["n_skipped"] == 0
    if name == "dna4_k10":
        assert diag.size >= 651
        if E == 8:
            assert counts["n_aligned"] >= 186 and set(range(9)) <= set(dist[ok].tolist())
            assert int(np.count_nonzero(ok & (span > 0))) >= 58
            assert int(np.count_nonzero(ok & (end == n))) >= 7 and int(np.count_nonzero(ok & (start == 0))) >= 7
        if E == 24:
            assert counts["n_aligned"] >= 231 and int(np.count_nonzero(ok & (diag < 0))) >= 6
        if E == 0:
            assert counts["n_aligned"] >= 79
    elif E == 8:
        assert diag.size >= 275 and counts["n_aligned"] >= 187
    # unedited reads cut at s with at least two windows: the locus that holds s reports the place itself
    n_plain = 0
    for i, (kind, s, m, plain, _) in enumerate(meta):
        if not plain or m < k + 1:
            continue
        a, b = int(off[i]), int(off[i + 1])
        holds = [l for l in range(a, b) if diag[l] <= s <= diag[l] + span[l]]
        assert len(holds) == 1, i
        l = holds[0]
        assert (got[0][l], got[1][l], got[2][l]) == (0, s, s + m), i
        assert got[3][i] <= l - a and got[4][i] >= 1
        n_plain += 1
    assert n_plain >= 60


# ---- 2. max_span ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("max_span", [64, 0])
def test_max_span(work, max_span):
    vote = (65_535, 1, 0)
    off, diag, span, _, _ = work.loci("dna4_k10", vote)[1]
    got, counts = work.run("dna4_k10", 8, vote, max_span)
    want = work.oracle("dna4_k10", 8, vote, max_span)
    print(max_span, counts)
    assert_same(got, counts, want, diag.size)
    assert np.array_equal(got[0] == SKIPPED, span > max_span)
    assert not got[1][got[0] == SKIPPED].any() and not got[2][got[0] == SKIPPED].any()
    assert counts["n_skipped"] >= 250 and counts["n_aligned"] >= 20


# ---- 3. word and class boundaries ------------------------------------------------------------------------------------------------------
LENGTHS = (10, 11, 63, 64, 65, 127, 128, 129, 255, 256, 257, 511, 512, 513, 1023, 1024, 1025, 1500)


def boundary_reads():
    """Four reads per length, cut from the DNA4 text: unedited; a substitution at letter 0 and at letter m - 1; three letters
    inserted from letter 62 on (m > 70) and one deleted at letter 127 (m > 135); flush with the end of the text.  Per read
    (m, s, planted distance, read offsets that an edit touches or that a window must not straddle)."""
    sigma, k, n, _ = WORKLOADS["dna4_k10"]
    text = text_of(sigma, n)
    z = synth.u64_stream(77, 4 * len(LENGTHS)).astype(np.int64) & 0x7FFFFFFF
    reads, meta = [], []
    for li, m in enumerate(LENGTHS):
        s = [int(z[4 * li + j] % (n - m - 16)) for j in range(3)] + [n - m]
        q = text[s[0]:s[0] + m].copy()
        reads.append(q); meta.append((m, s[0], 0, [], []))
        q = text[s[1]:s[1] + m].copy()
        q[0] = (q[0] + 1) % sigma
        q[m - 1] = (q[m - 1] + 2) % sigma
        reads.append(q); meta.append((m, s[1], 2, [0, m - 1], []))
        q = text[s[2]:s[2] + m + 8].copy()
        planted, touched, seams = 0, [], []
        if m > 70:
            q = np.insert(q, 62, synth.ranks(5000 + m, 3, sigma))
            planted, touched = 3, [62, 63, 64]
        if m > 135:
            q = np.delete(q, 127)
            planted, seams = 4, [127]                          # a window over letters 126 and 127 straddles the deletion
        reads.append(q[:m]); meta.append((m, s[2], planted, touched, seams))
        reads.append(text[n - m:].copy()); meta.append((m, n - m, 0, [], []))
    return pack(reads), meta


def clean_windows(m, k, touched, seams):
    c = 0
    for j in range(max(m - k + 1, 0)):
        if any(j <= t < j + k for t in touched) or any(j < t < j + k for t in seams):
            continue
        c += 1
    return c


def test_word_and_class_boundaries(work):
    sigma, k, n, _ = WORKLOADS["dna4_k10"]
    (ranks, roff), meta = boundary_reads()
    idx = work.index("dna4_k10")
    E = 8
    loci, al = idx.map_reads(ranks, roff, k, 1, *VOTE, max_edits=E, max_span=MAX_SPAN)
    off, diag, span, _, _ = loci.host()
    want = align(text_of(sigma, n), ranks, roff, off, diag, span, E, MAX_SPAN, sigma)
    got, counts = al.host(), al.counts()
    loci.close()
    al.close()
    assert_same(got, counts, want, diag.size)
    dist = got[0]
    n_required = 0
    for i, (m, s, planted, touched, seams) in enumerate(meta):
        a, b = int(off[i]), int(off[i + 1])
        if m > MAX_READ:
            assert b > a and np.all(dist[a:b] == SKIPPED) and got[3][i] == NO_BEST and got[4][i] == 0, i
        # "at least two windows" is read here as two windows that no planted edit touches: only those vote on the read's own
        # diagonal, and min_votes = 2 (m = 11 with a substitution at both ends has two windows and no vote)
        elif clean_windows(m, k, touched, seams) >= 2:
            assert b > a and int(dist[a:b].min()) <= planted, (i, m, planted, dist[a:b])
            assert dist[a + got[3][i]] == dist[a:b].min()
            n_required += 1
    assert n_required >= 4 * 15 - 2 and counts["n_skipped"] >= 8


# ---- 4. the largest E ------------------------------------------------------------------------------------------------------------------
def test_250_edits(work):
    sigma, k, n, _ = WORKLOADS["dna4_k10"]
    ranks, roff, _ = reads_of("dna4_k10")
    nr = 100
    few = (ranks[:int(roff[nr])], roff[:nr + 1])
    idx = work.index("dna4_k10")
    E = 250
    loci, al = idx.map_reads(*few, k, 1, *VOTE, max_edits=E, max_span=MAX_SPAN)
    off, diag, span, _, _ = loci.host()
    want = align(text_of(sigma, n), few[0], few[1], off, diag, span, E, MAX_SPAN, sigma)
    got, counts = al.host(), al.counts()
    loci.close()
    al.close()
    print(counts)
    assert_same(got, counts, want, diag.size)
    m = np.repeat(np.diff(few[1].astype(np.int64)), np.diff(off.astype(np.int64)))
    assert diag.size >= 100 and counts["n_aligned"] >= 0.9 * diag.size
    assert int(np.count_nonzero(diag - E < 0)) >= 3 and int(np.count_nonzero(diag + span + m + E > n)) >= 3


# ---- 5. against the text, not the oracle --------------------------------------------------------------------------------------------------
def lev(a, b, sigma):
    prev = list(range(len(b) + 1))
    for i, x in enumerate(a):
        cur = [i + 1] * (len(b) + 1)
        known = x < sigma
        for j, y in enumerate(b):
            c = prev[j] if known and x == y else prev[j] + 1
            up, left = prev[j + 1] + 1, cur[j] + 1
            cur[j + 1] = c if c <= up and c <= left else up if up <= left else left
        prev = cur
    return prev[-1]


def test_distance_of_the_reported_substring(work):
    picked = []
    for name in WORKLOADS:
        sigma, _, n, _ = WORKLOADS[name]
        ranks, roff, _ = reads_of(name)
        off = work.loci(name)[1][0].astype(np.int64)
        read_of = np.repeat(np.arange(N_READS), np.diff(off))
        for E in (1, 8, 24):
            got, _ = work.run(name, E)
            m = np.diff(roff.astype(np.int64))[read_of]
            ls = np.flatnonzero((got[0] <= E) & (m <= 160))
            for l in ls[::max(ls.size // 34, 1)][:34]:
                picked.append((name, E, int(l), int(read_of[l])))
                q = [int(x) for x in ranks[int(roff[read_of[l]]):int(roff[read_of[l] + 1])]]
                t = [int(x) for x in text_of(sigma, n)[int(got[1][l]):int(got[2][l])]]
                assert got[1][l] <= got[2][l] <= n
                assert lev(q, t, sigma) == got[0][l], (name, E, l)
    assert len(picked) >= 200


# ---- 6. letters >= sigma -----------------------------------------------------------------------------------------------------------------
def test_letters_outside_the_alphabet_cost_an_edit(work):
    n_reads = 0
    for name in WORKLOADS:
        _, _, meta = reads_of(name)
        off = work.loci(name)[1][0].astype(np.int64)
        got, _ = work.run(name, 24)
        for i, (_, _, _, _, bad) in enumerate(meta):
            if not bad:
                continue
            d = got[0][off[i]:off[i + 1]]
            assert not np.any(d == 0), i                               # the letter equals no text letter
            n_reads += int(np.any((d >= 1) & (d <= 24)))
    assert n_reads >= 5


# ---- 7. degenerate batches and plumbing ----------------------------------------------------------------------------------------------------
def assert_empty(al, nr, n_loci=0):
    dist, start, end, best, aligned = al.host()
    assert dist.dtype == np.uint8 and start.dtype == np.uint32 and end.dtype == np.uint32
    assert dist.size == start.size == end.size == n_loci
    assert best.dtype == np.uint32 and np.array_equal(best, np.full(nr, NO_BEST, np.uint32))
    assert aligned.dtype == np.uint32 and np.array_equal(aligned, np.zeros(nr, np.uint32))
    assert al.counts() == {"nr": nr, "n_loci": n_loci, "n_aligned": 0, "n_skipped": 0}


def test_degenerate_batches(work):
    engine, idx = work.engine, work.index("dna4_k10")
    loci, al = idx.map_reads(np.zeros(0, np.uint8), np.zeros(1, np.uint64), 10, max_edits=3)                 # nr = 0
    assert_empty(al, 0)
    ranks, roff = pack([synth.ranks(i, i % 10, 4) for i in range(300)])                                      # no read has a window
    loci2 = idx.vote_windows(ranks, roff, 10)
    al = loci2.align(idx, ranks, roff, 3, alignments=al)
    assert loci2.counts()["n_loci"] == 0
    assert_empty(al, 300)
    # nr differs from the loci's: refused, and the handle holds an empty result
    with pytest.raises(engine.KmxError) as e:
        loci2.align(idx, ranks[:int(roff[299])], roff[:300], 3, alignments=al)
    assert e.value.status == 1 and "nr" in str(e.value)
    assert_empty(al, 0)
    # host reads that do not hold together: refused as well, and the filled handle holds an empty result
    from_one, decreasing = np.array(roff), np.array(roff)
    from_one[0] = 1
    decreasing[3] = decreasing[5]
    for bad_ranks, bad_roff, word in ((ranks, from_one, "roff[0]"), (ranks, decreasing, "non-decreasing"), (np.zeros(0, np.uint8), roff, "ranks")):
        loci2.align(idx, ranks, roff, 3, alignments=al)
        assert al.counts()["nr"] == 300
        with pytest.raises(engine.KmxError) as e:
            loci2.align(idx, bad_ranks, bad_roff, 3, alignments=al)
        assert e.value.status == 1 and word in str(e.value)
        assert_empty(al, 0)
    for h in (loci, loci2, al):
        h.close()


def test_one_handle_for_batches_of_different_sizes(work):
    sigma, k, n, _ = WORKLOADS["dna4_k10"]
    idx = work.index("dna4_k10")
    ranks, roff, _ = reads_of("dna4_k10")
    few = pack([ranks[int(roff[i]):int(roff[i + 1])] for i in range(100, 130)])
    al = None
    for reads, E in ((few, 8), ((ranks, roff), 1), (few, 8)):
        loci = idx.vote_windows(*reads, k, 1, *VOTE)
        al = loci.align(idx, *reads, E, MAX_SPAN, alignments=al)
        off, diag, span, _, _ = loci.host()
        want = work.oracle("dna4_k10", E) if reads is not few else align(text_of(sigma, n), *reads, off, diag, span, E, MAX_SPAN, sigma)
        assert_same(al.host(), al.counts(), want, diag.size)
        loci.close()
    al.close()


def test_device_form_on_a_callers_stream_and_device_view(work):
    import torch
    idx = work.index("dna4_k10")
    ranks, roff, _ = reads_of("dna4_k10")
    stream = torch.cuda.Stream()
    d_r = torch.from_numpy(np.array(ranks)).cuda()
    d_o = torch.from_numpy(np.array(roff).view(np.int64)).cuda()
    torch.cuda.synchronize()
    r = idx.search_windows_device(d_r.data_ptr(), d_o.data_ptr(), N_READS, 10, 1, stream=stream.cuda_stream)
    loci = r.vote(*VOTE)
    before = loci.host()
    al = loci.align_device(idx, d_r.data_ptr(), d_o.data_ptr(), N_READS, 8, MAX_SPAN, stream=stream.cuda_stream)
    stream.synchronize()
    want = work.oracle("dna4_k10", 8)
    c = al.counts()
    sizes = (c["n_loci"], c["n_loci"], c["n_loci"], c["nr"], c["nr"])
    for name, ptr, n, x in zip(NAMES, al.device_ptrs(), sizes, want):
        assert np.array_equal(dev_array(ptr, n, x.dtype), x), name
    assert_same(al.host(), c, want, before[1].size)
    for g, x in zip(loci.host(), before):                                  # the call only reads the loci handle
        assert np.array_equal(g, x)
    for h in (al, loci, r):
        h.close()


def test_aligning_leaves_the_loci_and_the_windows_result_as_they_were(work):
    r = work.windows("dna4_k10")
    host, win = r.host(), r.window_offsets()
    loci, before = work.loci("dna4_k10")
    ptrs = loci.device_ptrs()
    for E in (0, 24):
        work.run("dna4_k10", E)
    assert loci.device_ptrs() == ptrs
    for name, g, x in zip(("locus_off", "diag", "span", "votes", "skipped"), loci.host(), before):
        assert g.dtype == x.dtype and np.array_equal(g, x), name
    for name, g, x in zip(("hit_off", "positions", "status", "kinds"), r.host(), host):
        assert g.dtype == x.dtype and np.array_equal(g, x), name
    assert np.array_equal(r.window_offsets(), win)


def test_map_reads_equals_the_three_calls(work):
    idx = work.index("aa20_k5")
    ranks, roff, _ = reads_of("aa20_k5")
    loci, al = idx.map_reads(ranks, roff, 5, 1, *VOTE, max_edits=8, max_span=MAX_SPAN)
    for g, x in zip(loci.host(), work.loci("aa20_k5")[1]):
        assert g.dtype == x.dtype and np.array_equal(g, x)
    got, counts = work.run("aa20_k5", 8)
    for g, x in zip(al.host(), got):
        assert g.dtype == x.dtype and np.array_equal(g, x)
    assert al.counts() == counts
    loci.close()
    al.close()
