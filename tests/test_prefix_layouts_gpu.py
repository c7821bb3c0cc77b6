"""The sub-k mergers on the planted slices of tests/prefix_layouts.py: every slice on a size-class boundary of the dispatcher
(len 512 | 513, 2048 | 2049, 8192 | 8193, 32768 | 32769; R 4 | 5, 32 | 33, 64 | 65; len 8 R - 1 | 8 R; a band of exactly 8192 | 8193
positions; chunks + merge passes with a partial last chunk and tile; cnt and len on two sides of a threshold) in every
interleaving of its runs.  The reference is the plant table (Slice.expected), element for element; the class every slice went
to is asserted through kmx_result_paths against the dispatcher's conditions restated in Python (prefix_layouts.classify).

Whether a slice beyond one chunk was cut into bands, spread by value or left to chunks + merge passes is decided on the device
and not read back: kmx_result_paths reports such slices in prefix_long / prefix_large_chunks / prefix_large_elems only, and the
host launches k_prefix_bands, k_prefix_split and the merge passes for any batch that holds one.  Batches that hold slices of
ONE of the three classes alone are run as well, with the launches asserted; which of the three took a slice is pinned on the CPU
(test_prefix_layouts_cpu.py: bands_fit restates k_prefix_bands) and here by the list each of them has to return.

k_small (the latency path): batches of at most 256 queries on a handle of their own, on either side of each of its limits."""
import numpy as np
import pytest

from tests import prefix_layouts as pl

pytestmark = pytest.mark.gpu

N_FILL = 8200                      # more queries than the latency path takes (KMX_SMALL_BLOCKS * KMX_SMALL_NQ = 8192)
LAYOUTS = pl.all_layouts()
LARGE = ("banded", "split", "chunked")


def build_index(engine, lay, levels=-1):
    # an open table and no prefix levels: the runs of a slice are the k-mers planted behind its query, nothing else
    return engine.Index(lay.text, pl.SIGMA, [pl.K], table=engine.TABLE_OPEN, prefix_levels=levels)


def check_lists(engine, out, sl, n_fill):
    """Status, kind, hit_off and positions of the slices in front of a batch against the plant table; the fillers hit nothing."""
    ho, pos, st, kd = out
    ns = len(sl)
    assert ho.size == ns + n_fill + 1
    assert (st == engine.Q_OK).all() and (kd[:ns] == engine.KIND_PREFIX).all()
    assert np.array_equal(np.diff(ho.astype(np.int64))[:ns], [s.cnt for s in sl])
    assert int(ho[ns]) == int(ho[-1])
    for i, s in enumerate(sl):
        got = pos[int(ho[i]):int(ho[i + 1])]
        assert np.array_equal(got, s.expected), (s, int(np.argmax(got != s.expected)) if got.size == s.expected.size else got.size)
        if s.tail_pos is not None:
            assert got[-1] == s.tail_pos and got[-2] < s.tail_pos


def expected_counts(lay, sl):
    cc = lay.class_counts(sl)
    large = [s.length for s in sl if s.length > pl.PSORT_BLOCK_CAP]
    chunks = max((-(-l // pl.PSORT_BLOCK_CAP) for l in large), default=0)
    return cc, {"prefix_plain": cc["plain"], "prefix_small": cc["small"], "prefix_merge_small": cc["merge_small"], "prefix_mid": cc["mid"],
                "prefix_long": cc["one_chunk"] + cc["banded"] + cc["split"] + cc["chunked"],
                "prefix_large_chunks": chunks, "prefix_large_elems": sum(large)}, chunks


def check_general(engine, idx, res, lay, names, label):
    """One batch through the general pipeline into `res`: the lists, the classes as reported, the kernels as launched."""
    q, off, sl = lay.batch(names, fillers=N_FILL)
    idx.stats_reset()
    idx.search(q, off, result=res)
    k, p = idx.stats(), res.paths()
    cc, want, chunks = expected_counts(lay, sl)
    got = {name: p[name] for name in want}
    print(f"{label}: " + " ".join(f"{c}={n}" for c, n in cc.items() if n) + f" | reported {got}")
    check_lists(engine, res.host(), sl, N_FILL)
    assert p["small"] is False and k["k_small"]["launches"] == 0 and k["k_lookup"]["launches"] >= 1
    assert got == want
    assert res.counts()["n_prefix"] == len(sl)
    n_long = want["prefix_long"]
    assert bool(k["k_prefix_sort_small"]["launches"]) == bool(cc["small"])
    assert bool(k["k_prefix_merge_small"]["launches"]) == bool(cc["merge_small"])
    assert k["k_prefix_sort_block"]["launches"] == (1 if cc["mid"] + n_long else 0)
    # beyond one chunk: the cut into bands and the spread by value are tried, and ceil(log2(chunks)) merge passes run over the rest
    passes = int(np.ceil(np.log2(chunks))) if chunks else 0
    assert k["k_prefix_bands"]["launches"] == (1 if chunks else 0)
    assert k["k_prefix_split"]["launches"] == (1 if chunks else 0)
    assert k["k_prefix_merge_pass"]["launches"] == passes
    return cc


@pytest.mark.parametrize("name,make,expect", LAYOUTS, ids=[t[0] for t in LAYOUTS])
def test_planted_slices_through_the_general_pipeline(engine, name, make, expect):
    lay = make()
    idx = build_index(engine, lay)
    idx.stats_enable(True)
    res = engine.Result()
    for s in lay.slices:
        print(f"{name}: {s!r}")
        assert expect is None or s.cls == expect[s.name]
    for rep in range(2):                                   # the same handle again: grown buffers, counters reset
        check_general(engine, idx, res, lay, None, f"{name} run {rep}")
    # slices beyond one chunk, one class at a time
    for cls in LARGE:
        names = [s.name for s in lay.slices if s.cls == cls]
        if names:
            cc = check_general(engine, idx, res, lay, names, f"{name} {cls} only")
            assert cc[cls] == len(names) == res.paths()["prefix_long"]
    res.close()
    idx.close()


@pytest.mark.parametrize("T", sorted(pl.TAIL_CASES))
def test_prefix_levels_do_not_change_the_lists(engine, T):
    """The tail layouts on an index with the default prefix levels (open table): the same lists, the tail position in its place."""
    lay = pl.tail_layout(T)
    idx = build_index(engine, lay, levels=0)
    q, off, sl = lay.batch(None, fillers=N_FILL)
    res = idx.search(q, off)
    check_lists(engine, res.host(), sl, N_FILL)
    assert res.paths()["small"] is False
    if min(idx.levels()) >= pl.K - pl.M:                   # a level answers the query outright: one list, copied as it lies
        assert res.paths()["prefix_plain"] == len(sl)
    idx.close()


@pytest.fixture(scope="module")
def latency(engine):
    lay = pl.latency_layout()
    idx = build_index(engine, lay)
    idx.stats_enable(True)
    yield lay, idx
    idx.close()


@pytest.mark.parametrize("name,names,answers", pl.LATENCY_BATCHES, ids=[t[0] for t in pl.LATENCY_BATCHES])
def test_latency_path_answers_up_to_its_limits(engine, latency, name, names, answers):
    lay, idx = latency
    q, off, sl = lay.batch(names)
    assert pl.small_answers(sl) == answers and len(sl) <= pl.SMALL_WSLOW + pl.SMALL_BSLOW      # (the host sends up to 40 sub-k queries)
    res = engine.Result()
    for rep in range(2):
        idx.stats_reset()
        idx.search(q, off, result=res)
        k, p = idx.stats(), res.paths()
        print(f"{name} run {rep}: small={p['small']} k_small={k['k_small']['launches']} k_lookup={k['k_lookup']['launches']}")
        check_lists(engine, res.host(), sl, 0)
        assert k["k_small"]["launches"] == 1                 # answered or declined by the kernel itself, not by the host in front of it
        if answers:
            assert p["small"] is True and k["k_lookup"]["launches"] == 0
        else:
            assert p["small"] is False and k["k_lookup"]["launches"] >= 1
            _, want, _ = expected_counts(lay, sl)
            assert {c: p[c] for c in want} == want
    res.close()
