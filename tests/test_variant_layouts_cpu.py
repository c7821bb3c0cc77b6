"""The batch builder of tests/variant_layouts.py puts every requested event on the requested slot — judged by the oracle's
hit_off, for all four k_fill tile sizes.  tests/test_variants_gpu.py relies on these batches to reach the tile edges of every
k_fill variant: a change to synth or to the builder that moves an event fails here instead of quietly testing less."""
import numpy as np
import pytest

from tests import variant_layouts as vl

K = 6


@pytest.fixture(scope="module")
def setup(orc):
    text = vl.make_text()
    return text, vl.LayoutBuilder(text, K), orc.Index(text, vl.SIGMA, [K])


def test_text_has_the_planted_buckets(setup):
    text, lb, _ = setup
    assert 55_000 <= text.size <= 65_000
    assert lb.hist[lb.giant] > 2 * 4096
    assert len(lb.ones) + len(lb.twos) >= 300 and len(lb.absent) >= 300
    assert lb.prefix_counts(lb.p_long)[1] == 1 and lb.prefix_counts(lb.p_runs)[1] == 2


@pytest.mark.parametrize("T", vl.TILES)
def test_every_event_lies_on_its_slot(setup, orc, T):
    text, lb, oidx = setup
    batch = vl.main_batch(lb, T)
    o_off, o_pos, o_st, _ = oidx.search_batch(batch.qranks, batch.qoff, mode=orc.MODE_INTENDED, n_threads=4)
    assert (o_st == 0).all()
    seen = vl.check_events(batch, o_off)
    assert seen == set(vl.EVENT_LAYOUTS) | {"total"}
    assert len(batch.qs) <= 20_000 and int(o_off[-1]) % T == 0
    # the planted queries against the text itself
    for ev in batch.events:
        if "q" in ev:
            q = ev["q"]
            assert np.array_equal(o_pos[int(o_off[q]):int(o_off[q + 1])], orc.naive_scan(text, batch.qs[q])), ev["layout"]


@pytest.mark.parametrize("T", vl.TILES)
def test_totals_and_the_stitch_query(setup, orc, T):
    text, lb, oidx = setup
    for total in (T - 1, T, T + 1, 3 * T, 3 * T + 1):
        batch = lb.build(T, [("total", total)])
        o_off = oidx.search_batch(batch.qranks, batch.qoff, mode=orc.MODE_INTENDED, n_threads=4)[0]
        assert vl.check_events(batch, o_off) == {"total"} and int(o_off[-1]) == total
    batch = lb.build(T, ["stitch_straddles", ("total", None)])
    o_off, o_pos, o_st, _ = oidx.search_batch(batch.qranks, batch.qoff, mode=orc.MODE_INTENDED, n_threads=4)
    assert (o_st == 0).all()
    assert vl.check_events(batch, o_off) == {"stitch_straddles", "total"}
    q = batch.events[0]["q"]
    assert np.array_equal(o_pos[int(o_off[q]):int(o_off[q + 1])], orc.naive_scan(text, batch.qs[q]))
