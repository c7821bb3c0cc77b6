"""The planted texts of tests/prefix_layouts.py hold what their plant tables say: every slice's len, R and run lengths counted
from the text by a numpy k-mer scan, its expected list against a naive scan of the text, and the merger the dispatcher's
conditions give it against the one the case was built for.  The texts put a slice on every size-class boundary of the sub-k
mergers (Layout.batch() packs the queries, Slice.expected is the list a search must return): a change to the builder that moves
a case fails here, without a GPU."""
import numpy as np
import pytest

from tests import prefix_layouts as pl

LAYOUTS = pl.all_layouts()


@pytest.mark.parametrize("name,make,expect", LAYOUTS, ids=[t[0] for t in LAYOUTS])
def test_text_holds_the_planted_slices(orc, name, make, expect):
    lay = make()
    assert lay.n <= 5_000_000 and not (lay.text[1:] == 0)[lay.text[:-1] == 0].any()           # a few million letters; no two 0s side by side
    found = pl.scan(lay)
    assert int((lay.text == 0).sum()) == sum(s.cnt for s in lay.slices)                      # letter 0 only where planted
    for s, (length, run_lens, pos, tails) in zip(lay.slices, found):
        print(f"{name}: {s!r}")
        assert length == s.length and run_lens.size == s.runs and np.array_equal(run_lens, s.run_lens), s
        assert np.array_equal(np.concatenate([pos, tails]), s.expected), s
        assert tails.size == (s.tail_pos is not None) and s.cnt == s.length + tails.size, s
        assert (np.diff(s.expected.astype(np.int64)) >= pl.K).all() or tails.size, s         # occurrences at least k apart
        assert np.array_equal(orc.naive_scan(lay.text, s.query), s.expected), s
        if s.length > pl.PSORT_BLOCK_CAP and s.runs <= pl.BAND_RUNS:                          # the arithmetic of k_prefix_bands, from the scan
            assert pl.classify(length, run_lens.size, pl.bands_fit(pos, lay.n)) == s.cls, s
        else:
            assert pl.classify(length, run_lens.size) == s.cls, s
        if expect is not None:
            assert s.cls == expect[s.name], (s, expect[s.name])
    if expect is not None:
        assert {s.name for s in lay.slices} == set(expect)


def test_interleavings_are_what_they_are_called():
    """Run r wholly below / above run r + 1, element by element, and the giant run with its singles before, behind and inside it."""
    for inter in pl.INTERLEAVINGS:
        lay = pl.boundary_layout(inter)
        for s in (lay.by_name["len513_R4"], lay.by_name["len2049_R33"], lay.by_name["len8193_R64"]):
            # the run of every position, in text order: the rank of its k-mer among the slice's k-mers
            codes = np.zeros(s.length, np.int64)
            for t in range(pl.K):
                codes = codes * pl.SIGMA + lay.text[s.expected.astype(np.int64) + t]
            run = np.searchsorted(np.unique(codes), codes)
            if inter == "below":
                assert (np.diff(run) >= 0).all()
            elif inter == "above":
                assert (np.diff(run) <= 0).all()
            elif inter == "round_robin":
                assert np.array_equal(run[:s.runs], np.arange(s.runs))                       # (every run has a first element)
                assert (np.bincount(run[:2 * s.runs]) <= 2).all()
            elif inter == "random":
                assert (np.diff(run) < 0).any() and (np.diff(run) > 0).any()
            else:
                g = s.runs // 2
                singles = np.nonzero(run != g)[0]
                assert singles.size == s.runs - 1 and np.array_equal(np.sort(run[singles]), np.delete(np.arange(s.runs), g))
                if inter == "giant_singles_before":
                    assert singles.max() == s.runs - 2
                elif inter == "giant_singles_behind":
                    assert singles.min() == s.length - (s.runs - 1)
                else:
                    assert singles.min() > 0 and singles.max() < s.length - 1 and (np.diff(singles) > 1).all()


def test_band_edges_are_exact():
    """The band cases hold exactly 8192 / 8193 positions in the band they were built around, at the text's own length."""
    lay = pl.bands_layout()
    pos = lambda name: lay.by_name[name].expected.astype(np.int64)
    assert pl.band_sizes(pos("band_of_8192"), lay.n, pl.BAND_FULL).tolist() == [6912, 8192, 6912, 6912, 6912]
    at_full, at_band = pl.band_sizes(pos("band_of_8193"), lay.n, pl.BAND_FULL), pl.band_sizes(pos("band_of_8193"), lay.n, pl.BAND)
    assert at_full.tolist() == [6912, 8193, 6912, 6912, 6911] and at_band.size == 6 and at_band.max() > pl.PSORT_MID_CAP
    for name, below in (("half_8192", 8192), ("half_8193", 8193)):
        assert int((pos(name) < lay.n // 2).sum()) == below and pos(name).size == 2 * 8192
    assert pos("first_tenth").max() < lay.n // 10 and pos("empty_first_fifth").min() >= lay.n // 5
    sizes = pl.band_sizes(pos("empty_first_fifth"), lay.n, pl.BAND_FULL)
    assert sizes[0] == 0 and sizes.max() <= pl.PSORT_MID_CAP
    passes = pl.passes_layout()
    for s in passes.slices:                                                                   # bands and split decline: chunks + merge passes
        assert s.runs <= pl.BAND_RUNS and not pl.bands_fit(s.expected.astype(np.int64), passes.n) and s.cls == "chunked"


def test_latency_batches_sit_on_the_limits():
    """The batches for the limits of k_small hold what their names say: 32 | 33 wave-sized and 8 | 9 block-sized slow queries, a slice of
    4096 | 4097 positions, nine of 1024 | 1025, a hit total of exactly 49152 | 49153 in one workgroup — and the kernel's conditions,
    restated, answer the first of each pair and decline the second."""
    lay = pl.latency_layout()
    by = {name: [lay.by_name[n] for n in names] for name, names, _ in pl.LATENCY_BATCHES}
    assert sum(s.cnt for s in by["total_49152"]) == pl.SMALL_POS and sum(s.cnt for s in by["total_49153"]) == pl.SMALL_POS + 1
    for name, sl in by.items():
        assert all(s.runs > 1 for s in sl if s.name != "one")
    assert [s.length for s in by["nine_of_1024"]] == [pl.SMALL_WCAP] * 9 and [s.length for s in by["nine_of_1025"]] == [pl.SMALL_WCAP + 1] * 9
    assert by["one_of_4096"][0].length == pl.SMALL_SORT and by["one_of_4097"][0].length == pl.SMALL_SORT + 1
    assert len(by["wave_sized_32"]) == pl.SMALL_WSLOW and len(by["block_sized_8"]) == pl.SMALL_BSLOW
    assert all(s.length <= pl.SMALL_WCAP for s in by["wave_sized_33"]) and all(pl.SMALL_WCAP < s.length <= pl.SMALL_SORT for s in by["block_sized_9"])
    for name, sl in by.items():
        print(f"latency batch {name}: {len(sl)} slices, {sum(s.cnt for s in sl)} positions")
        assert len(sl) <= pl.SMALL_WSLOW + pl.SMALL_BSLOW and pl.small_answers(sl) == dict((n, a) for n, _, a in pl.LATENCY_BATCHES)[name]
    assert [a for _, _, a in pl.LATENCY_BATCHES] == [True, True] + [True, False] * 5
