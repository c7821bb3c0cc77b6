"""Reporting options of the approximate search on the GPU (kmx_search_approx_opts: KMX_APPROX_LOCI, KMX_APPROX_BEST, max_hits;
kmx_approx_found) against the independent checker tests/report_naive.py: positions, strands, distances, lengths, found,
statuses and n_hits."""
import os
import subprocess
import sys

import numpy as np
import pytest

from kmer_index_amd import synth
from tests.helpers import pack
from tests.report_fixtures import DNA4, NQ, fixture_batch, fixture_text, opts_search
from tests.report_naive import best, compare_batch, reference

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# (loci, best, max_hits): each flag alone, both, each cap alone and combined with the flags
COMBOS = [(1, 0, 0), (0, 1, 0), (1, 1, 0), (0, 0, 1), (0, 0, 3), (1, 0, 1), (1, 0, 3), (0, 1, 1), (0, 1, 3), (1, 1, 1), (1, 1, 3)]


def check(text, q, off, e, got, edit, comp, loci, best_, max_hits, ref=None):
    assert got["counts"]["n_hits"] == got["pos"].size == int(got["ho"][-1]) and got["counts"]["nq"] == off.size - 1
    return compare_batch(text, q, off, e, got["ho"], got["pos"], got["strands"], got["dist"], got["lens"], got["st"], got["found"], edit=edit,
                         complement=comp, use_loci=bool(loci), use_best=bool(best_), max_hits=max_hits, ref=ref)


@pytest.fixture(scope="module")
def indexes(engine):
    text = fixture_text()
    out = {"open": engine.Index(text, 4, [5], table=engine.TABLE_OPEN), "dense": engine.Index(text, 4, [5], table=engine.TABLE_DENSE)}
    yield out
    for idx in out.values():
        idx.close()


# ---- 1. parity with the checker over the grid --------------------------------------------------------------------------------

def assert_fixture_has_work(ref, e, edit):
    """On the checker's output alone: every rule has something to do on this batch (a degenerate input would make the parity
    test vacuous).  e = 0: LOCI is a no-op and there is one stratum, only the caps can cut."""
    H1 = [HL if edit else H for H, HL in ref]
    kept = [len(best(h)) for h in H1]
    if e:
        assert sum(len(h) - k for h, k in zip(H1, kept)) > 0                        # BEST removes hits
        assert sum(len({x[2] for x in h}) > 1 for h in H1) > 0                       # survivors in more than one stratum
        if edit:
            assert sum(len(H) - len(HL) for H, HL in ref) > 0                        # LOCI removes hits
    for lists in ([len(H) for H, _ in ref], [len(h) for h in H1], kept):            # each cap cuts some queries and not others
        for cap in (1, 3):
            assert 0 < sum(n > cap for n in lists) < len(lists), (cap, lists)


@pytest.mark.parametrize("e", [0, 1, 2, 3])
@pytest.mark.parametrize("strands", [False, True], ids=["one_strand", "both_strands"])
@pytest.mark.parametrize("edit", [False, True], ids=["hamming", "edit"])
@pytest.mark.parametrize("table", ["open", "dense"])
def test_parity_with_checker(engine, indexes, table, edit, strands, e):
    text, q, off, comp, ref = fixture_batch(edit, strands, e)
    assert_fixture_has_work(ref, e, edit)
    for loci, best_, max_hits in COMBOS:
        if loci and not edit:
            continue
        got = opts_search(engine, indexes[table], q, off, e, edit, comp, loci, best_, max_hits)
        assert np.all(got["st"] == engine.Q_OK)
        checked, by_loci, by_best, cut = check(text, q, off, e, got, edit, comp, loci, best_, max_hits, ref)
        assert checked == NQ
        if e:
            assert (by_loci > 0) == bool(loci) and (by_best > 0) == bool(best_)
        assert (0 < cut < NQ) == bool(max_hits), (loci, best_, max_hits, cut)


@pytest.mark.parametrize("edit", [False, True], ids=["hamming", "edit"])
def test_hits_on_both_strands_of_one_query(engine, edit):
    # every other copy of the unit reverse-complemented: a read has loci on both strands, BEST and the cap choose across them
    e = 2
    text, q, off, comp, ref = fixture_batch(edit, True, e, rc_copies=True)
    assert sum(len({h[1] for h in best(HL)}) == 2 for _, HL in ref) > 5
    idx = engine.Index(text, 4, [5])
    for loci, best_, max_hits in COMBOS:
        if loci and not edit:
            continue
        got = opts_search(engine, idx, q, off, e, edit, comp, loci, best_, max_hits)
        assert check(text, q, off, e, got, edit, comp, loci, best_, max_hits, ref)[0] == NQ
    idx.close()


def test_engine_keywords_route_to_the_new_call(engine, indexes):
    text, q, off, comp, ref = fixture_batch(True, True, 2)
    r = indexes["open"].search_approx(q, off, 2, edit=True, strands=True, loci=True, best=True, max_hits=3)
    ho, pos, dist, st = r.host()
    got = {"ho": ho, "pos": pos, "strands": r.strands(), "dist": dist, "lens": r.lengths(), "st": st, "found": r.found(), "counts": r.counts()}
    r.close()
    assert check(text, q, off, 2, got, True, comp, 1, 1, 3, ref)[3] > 0
    r = indexes["open"].search_approx(q, off, 2, max_hits=1)                       # Hamming, one strand, the cap alone
    assert int(np.diff(r.host()[0].astype(np.int64)).max()) == 1 and int(r.found().max()) > 1
    r.close()
    with pytest.raises(engine.KmxError) as ex:
        indexes["open"].search_approx(q, off, 2, loci=True)
    assert ex.value.status == 1 and "KMX_APPROX_LOCI" in str(ex.value)


# ---- 2. edge shapes ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("e", [1, 3])
def test_poly_a_lists_across_block_and_tile_boundaries(engine, e):
    # three lists of about 4400 hits each: every one straddles 256-thread blocks and the 1024- and 4096-hit tiles of the scans
    n = 4400
    text = np.zeros(n, np.uint8)
    idx = engine.Index(text, 4, [5])
    qs = [np.zeros(m, np.uint8) for m in (20, 24, 30)]
    q, off = pack(qs)
    ref = []
    for m in (20, 24, 30):
        H = [(p, 0, max(0, m - (n - p)), min(m, n - p)) for p in range(n - (m - e) + 1)]       # every start with m - e letters behind it
        ref.append((H, [H[0]]))                                # LOCI keeps exactly the leftmost: each start has its left
    plain = opts_search(engine, idx, q, off, e, edit=True)     # neighbour at no greater distance (the literal double loop
    check(text, q, off, e, plain, True, None, 0, 0, 0, ref)    # over 4400 hits is left out; H itself is checked here)
    assert np.array_equal(np.diff(plain["ho"].astype(np.int64)), [len(H) for H, _ in ref]) and plain["pos"].size > 3 * 4096
    for loci, best_, max_hits in COMBOS + [(0, 0, 1023), (0, 1, 4096), (0, 0, 4381), (0, 1, 4380)]:
        got = opts_search(engine, idx, q, off, e, True, None, loci, best_, max_hits)
        check(text, q, off, e, got, True, None, loci, best_, max_hits, ref)
        if loci:
            assert got["pos"].tolist() == [0, 0, 0] and got["found"].tolist() == [1, 1, 1] and got["lens"].tolist() == [20, 24, 30]
    idx.close()


@pytest.mark.parametrize("period", [2, 3])
def test_hits_e_and_e_plus_one_apart(engine, period):
    # exact hits every `period` letters: LOCI collapses them onto the leftmost when period <= e and keeps them all when
    # period == e + 1 (the shadows between them go either way)
    text = np.tile(np.array([0, 1, 3][:period], np.uint8), 600 // period)
    idx = engine.Index(text, 4, [5])
    q, off = pack([text[:24].copy(), text[1:22].copy()])
    for e in (1, 2, 3):
        ref = reference(text, q, off, e, True, None)
        for loci, best_, max_hits in ((1, 0, 0), (1, 1, 0), (1, 0, 3), (0, 1, 3)):
            got = opts_search(engine, idx, q, off, e, True, None, loci, best_, max_hits)
            check(text, q, off, e, got, True, None, loci, best_, max_hits, ref)
        got = opts_search(engine, idx, q, off, e, True, None, True, False, 0)
        first = got["pos"][:int(got["ho"][1])]
        if period <= e:
            assert first.tolist() == [0]
        elif period == e + 1:
            assert np.array_equal(first, np.arange(0, text.size - 24 + 1, period)) and not got["dist"][:first.size].any()
    idx.close()


def test_forward_and_reverse_hit_at_one_offset(engine):
    text = np.tile(np.array([0, 3], np.uint8), 200)            # ATAT...: every even-length window is its own reverse complement
    idx = engine.Index(text, 4, [5])
    q, off = pack([np.tile(np.array([0, 3], np.uint8), 10), np.tile(np.array([3, 0], np.uint8), 8)])
    for edit in (False, True):
        for e in (1, 2):
            ref = reference(text, q, off, e, edit, DNA4)
            for loci, best_, max_hits in COMBOS + [(0, 1, 2), (1 if edit else 0, 1, 2)]:
                if loci and not edit:
                    continue
                got = opts_search(engine, idx, q, off, e, edit, DNA4, loci, best_, max_hits)
                check(text, q, off, e, got, edit, DNA4, loci, best_, max_hits, ref)
                a, b = int(got["ho"][0]), int(got["ho"][1])
                if best_ and max_hits == 2:                    # the two strands of the leftmost exact hit, forward first
                    assert got["pos"][a:b].tolist() == [0, 0] and got["strands"][a:b].tolist() == [0, 1]
                if loci and best_ and not max_hits and e == 2:  # neither strand suppresses the other; each collapses onto its leftmost
                    assert got["pos"][a:b].tolist() == [0, 0] and got["strands"][a:b].tolist() == [0, 1] and got["found"][0] == 2
    idx.close()


@pytest.mark.parametrize("strands", [False, True], ids=["one_strand", "both_strands"])
def test_caps_around_found_and_inside_a_stratum(engine, indexes, strands):
    e = 2
    text, q, off, comp, ref = fixture_batch(True, strands, e)
    # a query whose LOCI survivors have at least two hits in their best stratum and a further stratum behind it
    pick = next(i for i, (_, HL) in enumerate(ref) if 2 <= len(best(HL)) < len(HL))
    n_best, n_all = len(best(ref[pick][1])), len(ref[pick][1])
    for max_hits in sorted({n_best - 1, n_best, n_best + 1, n_all - 1, n_all, n_all + 1}):
        got = opts_search(engine, indexes["open"], q, off, e, True, comp, True, False, max_hits)
        check(text, q, off, e, got, True, comp, 1, 0, max_hits, ref)
        a, b = int(got["ho"][pick]), int(got["ho"][pick + 1])
        assert b - a == min(max_hits, n_all) and got["found"][pick] == n_all
        if max_hits < n_best:                                  # the cut falls among ties on d: the leftmost of them stay
            assert got["pos"][a:b].tolist() == [h[0] for h in best(ref[pick][1])][:max_hits]
    for max_hits in (n_best - 1, n_best, n_best + 1):          # ... and with BEST, found is the size of the best stratum
        got = opts_search(engine, indexes["open"], q, off, e, True, comp, True, True, max_hits)
        check(text, q, off, e, got, True, comp, 1, 1, max_hits, ref)
        assert got["found"][pick] == n_best and int(got["ho"][pick + 1] - got["ho"][pick]) == min(max_hits, n_best)


@pytest.mark.parametrize("strands", [False, True], ids=["one_strand", "both_strands"])
def test_statuses_empty_lists_and_an_empty_batch(engine, strands):
    text = fixture_text()
    idx = engine.Index(text, 4, [5], query_size_range=20)
    comp = DNA4 if strands else None
    e = 2
    qs = [text[600:630].copy(),                       # served, in the repeat
          np.zeros(0, np.uint8),                      # empty
          np.array([0, 1, 7, 2, 3, 0, 1, 2, 3, 1], np.uint8),   # a letter outside the alphabet
          synth.ranks(9, 30, 4),                      # served, no hit
          np.array([1, 2], np.uint8),                 # m <= e
          text[100:160].copy(),                       # longest piece == range
          text[2000:2024].copy()]                     # served
    q, off = pack(qs)
    OK = engine.Q_OK
    for edit in (False, True):
        for loci, best_, max_hits in ((0, 1, 0), (0, 0, 2), (1 if edit else 0, 1, 1)):
            got = opts_search(engine, idx, q, off, e, edit, comp, loci, best_, max_hits)
            assert got["st"].tolist() == [OK, engine.Q_EMPTY_QUERY, engine.Q_BAD_RANK, OK, engine.Q_TOO_SHORT, engine.Q_TOO_LONG, OK]
            assert check(text, q, off, e, got, edit, comp, loci, best_, max_hits)[0] == 3
            assert got["found"][3] == 0 and got["found"][0] >= 1 and got["found"][6] >= 1
            plain = idx.search_approx(q, off, e, edit=edit, strands=strands)
            assert plain.host()[3].tolist() == got["st"].tolist() and plain.counts()["n_candidates"] == got["counts"]["n_candidates"]
            plain.close()
        none = opts_search(engine, idx, np.zeros(0, np.uint8), np.zeros(1, np.uint64), e, edit, comp, bool(edit), True, 2)
        assert none["ho"].tolist() == [0] and none["pos"].size == 0 and none["found"].size == 0 and none["counts"]["n_hits"] == 0
        miss = opts_search(engine, idx, qs[3], np.array([0, 30], np.uint64), e, edit, comp, bool(edit), True, 2)     # a chunk without hits
        assert miss["ho"].tolist() == [0, 0] and miss["found"].tolist() == [0] and miss["st"].tolist() == [OK]
    idx.close()


# ---- 3. chunking -----------------------------------------------------------------------------------------------------------------

CHILD = r"""
import sys
sys.path.insert(0, %(root)r)
import numpy as np
from kmer_index_amd import engine
from tests.report_fixtures import fixture_text, fixture_batch, opts_search
out = {}
idx = engine.Index(fixture_text(), 4, [5])
for strands in (False, True):
    for edit, loci, best, max_hits in ((True, 1, 1, 0), (True, 1, 0, 3), (False, 0, 1, 1)):
        text, q, off, comp, _ = fixture_batch(edit, strands, 2)
        got = opts_search(engine, idx, q, off, 2, edit, comp, loci, best, max_hits)
        tag = "%%d%%d%%d%%d%%d_" %% (strands, edit, loci, best, max_hits)
        for k in ("ho", "pos", "dist", "st", "found", "strands", "lens"):
            if got[k] is not None:
                out[tag + k] = got[k]
        out[tag + "chunks"] = got["counts"]["n_chunks"]
        out[tag + "cand"] = got["counts"]["n_candidates"]
np.savez(%(out)r, **out)
print("report child ok")
"""


@pytest.mark.parametrize("knobs", [{"KMX_APPROX_CHUNK_CANDIDATES": "8"}, {"KMX_APPROX_CHUNK_PIECES": "24"},
                                   {"KMX_APPROX_CHUNK_CANDIDATES": "300", "KMX_APPROX_CHUNK_PIECES": "60"}],
                         ids=["candidates", "pieces", "both"])
def test_chunked_batch_equals_one_chunk(engine, indexes, tmp_path, knobs):
    out = str(tmp_path / "chunked.npz")
    env = dict(os.environ)
    env.update(knobs)
    res = subprocess.run([sys.executable, "-c", CHILD % {"root": ROOT, "out": out}], capture_output=True, text=True, timeout=600, env=env)
    assert res.returncode == 0 and "report child ok" in res.stdout, res.stdout[-2000:] + res.stderr[-4000:]
    child = np.load(out)
    for strands in (False, True):
        for edit, loci, best_, max_hits in ((True, 1, 1, 0), (True, 1, 0, 3), (False, 0, 1, 1)):
            text, q, off, comp, ref = fixture_batch(edit, strands, 2)
            one = opts_search(engine, indexes["open"], q, off, 2, edit, comp, loci, best_, max_hits)
            tag = "%d%d%d%d%d_" % (strands, edit, loci, best_, max_hits)
            assert one["counts"]["n_chunks"] == 1 and int(child[tag + "chunks"]) > 1
            assert int(child[tag + "cand"]) == one["counts"]["n_candidates"]
            for k in ("ho", "pos", "dist", "st", "found", "strands", "lens"):
                if one[k] is not None:
                    assert child[tag + k].dtype == one[k].dtype and child[tag + k].tobytes() == one[k].tobytes(), (tag, k)
            check(text, q, off, 2, one, edit, comp, loci, best_, max_hits, ref)


# ---- 4. no option set: the older entry points, array for array -----------------------------------------------------------------

@pytest.mark.parametrize("strands", [False, True], ids=["one_strand", "both_strands"])
@pytest.mark.parametrize("edit", [False, True], ids=["hamming", "edit"])
def test_no_option_equals_the_older_entry_points(engine, indexes, edit, strands):
    idx = indexes["dense"]
    for e in (0, 2, 3):
        text, q, off, comp, ref = fixture_batch(edit, strands, e)
        got = opts_search(engine, idx, q, off, e, edit, comp)
        old = idx.search_approx(q, off, e, edit=edit, strands=strands, complement=comp)
        ho, pos, dist, st = old.host()
        for name, arr in (("ho", ho), ("pos", pos), ("dist", dist), ("st", st), ("strands", old.strands() if strands else None),
                          ("lens", old.lengths() if edit else None)):
            assert (arr is None and got[name] is None) or (got[name].dtype == arr.dtype and got[name].tobytes() == arr.tobytes()), name
        assert got["counts"] == old.counts()
        assert np.array_equal(got["found"], np.diff(ho)) and got["found"].dtype == np.uint64
        with pytest.raises(engine.KmxError) as ex:
            old.found()
        assert ex.value.status == 1 and "kmx_approx_found" in str(ex.value)
        old.close()
        check(text, q, off, e, got, edit, comp, 0, 0, 0, ref)


# ---- 5. loaded and replicated indexes ----------------------------------------------------------------------------------------------

def test_loaded_and_replicated_indexes(engine, indexes, tmp_path):
    e = 2
    text, q, off, comp, ref = fixture_batch(True, True, e)
    want = opts_search(engine, indexes["open"], q, off, e, True, comp, True, True, 3)
    check(text, q, off, e, want, True, comp, 1, 1, 3, ref)
    path = str(tmp_path / "ix.kmx")
    indexes["open"].save(path)
    loaded = engine.Index.load(path)
    rep = engine.Index(text, 4, [5], devices=[0, 0])
    for other in (loaded, rep):
        got = opts_search(engine, other, q, off, e, True, comp, True, True, 3)
        for k in ("ho", "pos", "dist", "st", "found", "strands", "lens"):
            assert np.array_equal(want[k], got[k]), k
        other.close()
