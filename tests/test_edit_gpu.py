"""Edit-distance search on the GPU (kmx_search_approx with KMX_APPROX_EDIT, kmx_approx_lengths) against the independent
numpy checker: positions, distances and lengths equal."""
import os
import subprocess
import sys
import threading

import numpy as np
import pytest

from kmer_index_amd import synth
from tests.edit_naive import compare_batch, edit_naive
from tests.helpers import CASES, mutate, pack

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_PARITY = 60_000          # letters of text per parity case (the checker is O(n m) per query)


def _edit_search(idx, qranks, qoff, e):
    r = idx.search_approx(qranks, qoff, e, edit=True)
    ho, pos, dist, st = r.host()
    return ho, pos, dist, r.lengths(), st, r


def _queries(text, sigma, ks, e, seed):
    """The length ladder of the Hamming parity test (pieces below k, equal to k, above k, a sum of two ks); per length a
    uniform random read, two reads planted with 0 .. e edits of mixed kinds, one with e + 1 edits, one planted within the last
    14 letters and one at offset 0 .. e (windows cut by either end of the text)."""
    k0, k1 = min(ks), max(ks)
    piece_lengths = sorted({max(1, k0 - 2), k0, k1 + 3} | ({ks[0] + ks[1]} if len(ks) > 1 else set()))
    lengths = [pl * (e + 1) + (j % (e + 1)) for j, pl in enumerate(piece_lengths)]
    n = text.size
    rng = np.random.default_rng(seed)
    qs = []
    for m in lengths:
        for kind in range(6):
            if kind == 0:
                qs.append(rng.integers(0, sigma, m).astype(np.uint8))
                continue
            if kind == 4:
                s = n - m - int(rng.integers(0, 15))
            elif kind == 5:
                s = int(rng.integers(0, e + 1))
            else:
                s = int(rng.integers(0, n - m - e))
            d = e + 1 if kind == 3 else int(rng.integers(0, e + 1))
            qs.append(mutate(text[s:s + m + e + 1], m, d, sigma, rng))
    return pack(qs)


# ---- 1. parity with the checker -----------------------------------------------------------------------------------------

@pytest.mark.parametrize("table", ["open", "dense"])
@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_parity_with_checker(engine, case, table):
    name, sigma, _, ks, _ = case
    text = synth.ranks(1000 + len(name), N_PARITY, sigma)
    idx = engine.Index(text, sigma, ks, table=engine.TABLE_OPEN if table == "open" else engine.TABLE_DENSE)
    for e in range(4):
        qranks, qoff = _queries(text, sigma, ks, e, seed=191 + e)
        ho, pos, dist, lens, st, r = _edit_search(idx, qranks, qoff, e)
        assert set(np.unique(st).tolist()) <= {engine.Q_OK, engine.Q_SUBK_FANOUT}
        checked = compare_batch(text, qranks, qoff, e, ho, pos, dist, lens, st)
        assert checked >= (qoff.size - 1) // 2, (e, checked)
        c = r.counts()
        assert c["n_hits"] == pos.size and c["n_chunks"] == 1
        r.close()
    idx.close()


# ---- 2. reads with one inserted or deleted letter -----------------------------------------------------------------------

def test_indel_reads_are_found_where_hamming_loses_them(engine):
    text = synth.ranks(1234, 60_000, 4)
    rng = np.random.default_rng(1234)
    starts = rng.integers(0, text.size - 30, 80)
    qs = []
    for t, s in enumerate(starts):
        w = text[s:s + 30]
        if t < 40:
            qs.append(np.delete(w, 15))
        else:
            qs.append(np.insert(w, 15, rng.integers(0, 4)).astype(np.uint8))
    qranks, qoff = pack(qs)
    idx = engine.Index(text, 4, [10])
    ho, pos, dist, lens, st, r = _edit_search(idx, qranks, qoff, 2)
    assert compare_batch(text, qranks, qoff, 2, ho, pos, dist, lens, st) == 80
    hh, hpos, hmm, hst = idx.search_approx(qranks, qoff, 2).host()
    other_length = 0
    for i, s in enumerate(starts):
        a, b = int(ho[i]), int(ho[i + 1])
        at = np.nonzero(pos[a:b] == s)[0]
        assert at.size == 1 and dist[a + at[0]] == 1 and lens[a + at[0]] == 30, i
        other_length += int(np.sum(lens[a:b] != qs[i].size))
        ha, hb = int(hh[i]), int(hh[i + 1])
        assert not np.any((hpos[ha:hb] == s) & (hmm[ha:hb] <= 1)), i
    assert other_length >= 80
    r.close()
    idx.close()


# ---- 3. periodic text: nearly every start is named by many (piece, displacement) pairs ----------------------------------

@pytest.mark.parametrize("ks", [[5], [8, 10, 12]])
def test_periodic_text_many_overlapping_windows(engine, ks):
    rng = np.random.default_rng(5)
    text = np.tile(np.array([0, 1], np.uint8), 50_000)
    noise = rng.integers(0, text.size, 300)
    text[noise] = rng.integers(0, 4, noise.size).astype(np.uint8)
    idx = engine.Index(text, 4, ks)
    qs = []
    for m in (16, 24, 31):
        q = np.tile(np.array([0, 1], np.uint8), m)[:m].copy()
        qs.append(q.copy())
        q[m // 3] = 3
        qs.append(q.copy())
        q[2 * m // 3] = 2
        qs.append(q)
    qranks, qoff = pack(qs)
    for e in range(4):
        ho, pos, dist, lens, st, r = _edit_search(idx, qranks, qoff, e)
        compare_batch(text, qranks, qoff, e, ho, pos, dist, lens, st)
        assert int(np.diff(ho.astype(np.int64)).max()) > 1000
        r.close()
    idx.close()


# ---- 4. the Hamming hits are a subset, 5. e = 0 ------------------------------------------------------------------------

def _keys(ho, pos):
    qi = np.repeat(np.arange(ho.size - 1, dtype=np.uint64), np.diff(ho).astype(np.int64))
    return (qi << np.uint64(32)) | pos.astype(np.uint64)


def test_hamming_hits_are_a_subset(engine):
    text = synth.ranks(77, 300_000, 4)
    idx = engine.Index(text, 4, [8, 10, 12])
    for e in (1, 2, 3):
        q, off = synth.planted_reads(178 + e, text, 2000, 32, 4, e)
        hh, hpos, hmm, hst = idx.search_approx(q, off, e).host()
        ho, pos, dist, lens, st, r = _edit_search(idx, q, off, e)
        assert np.array_equal(st, hst) and np.all(st == engine.Q_OK)
        hk, ek = _keys(hh, hpos), _keys(ho, pos)
        assert hk.size >= 2000 and np.all(np.diff(ek.astype(np.int64)) > 0)
        at = np.searchsorted(ek, hk)
        assert np.all(at < ek.size) and np.array_equal(ek[at], hk)
        assert np.all(dist[at] <= hmm)
        assert np.all(dist <= e) and np.all(np.abs(lens.astype(np.int64) - 32) <= e)
        r.close()
    idx.close()


def test_zero_edits_equal_zero_substitutions(engine):
    text = synth.ranks(77, 300_000, 4)
    idx = engine.Index(text, 4, [8, 10, 12])
    qranks, qoff = synth.mixed_queries(78, text, 3000, list(range(3, 40)), 4)
    hh, hpos, hmm, hst = idx.search_approx(qranks, qoff, 0).host()
    ho, pos, dist, lens, st, r = _edit_search(idx, qranks, qoff, 0)
    assert np.array_equal(st, hst) and np.array_equal(ho, hh) and np.array_equal(pos, hpos)
    assert pos.size > 2000 and not dist.any()
    m = np.diff(qoff.astype(np.int64))
    assert np.array_equal(lens, np.repeat(m, np.diff(ho.astype(np.int64))).astype(np.uint32))
    r.close()
    with pytest.raises(engine.KmxError):
        idx.search_approx(qranks, qoff, 0).lengths()          # not a result of a call with the flag
    idx.close()


# ---- 6. statuses --------------------------------------------------------------------------------------------------------

def test_statuses(engine):
    text = synth.ranks(81, 5000, 4)
    idx = engine.Index(text, 4, [14], query_size_range=60)
    e = 2
    qs = [np.zeros(0, np.uint8),                       # empty
          np.array([0, 1, 7, 2, 3, 0, 1], np.uint8),  # a letter outside the alphabet
          np.array([1, 2], np.uint8),                 # m <= e
          text[100:100 + 3 * 60].copy(),              # longest piece == range
          np.array([1, 2, 3, 0, 1, 2], np.uint8),     # pieces of two letters: 4^12 buckets > the sub-k fan-out limit
          text[:150].copy(),                          # served (pieces of 50 letters)
          text[4000:4000 + 177].copy()]               # served (pieces of 59 letters)
    qranks, qoff = pack(qs)
    ho, pos, dist, lens, st, r = _edit_search(idx, qranks, qoff, e)
    assert st.tolist() == [engine.Q_EMPTY_QUERY, engine.Q_BAD_RANK, engine.Q_TOO_SHORT, engine.Q_TOO_LONG, engine.Q_SUBK_FANOUT,
                           engine.Q_OK, engine.Q_OK]
    assert st.tolist() == idx.search_approx(qranks, qoff, e).host()[3].tolist()
    assert compare_batch(text, qranks, qoff, e, ho, pos, dist, lens, st) == 2
    r.close()
    idx.close()
    # n < m <= n + e: served, the whole text is within e deletions of the query
    small = synth.ranks(83, 40, 4)
    idx = engine.Index(small, 4, [5])
    for extra in (1, 2, 3):
        q = np.concatenate([small[:20], synth.ranks(84, extra, 4), small[20:]])
        off = np.array([0, q.size], np.uint64)
        ho, pos, dist, lens, st, r = _edit_search(idx, q, off, 3)
        assert st[0] == engine.Q_OK and compare_batch(small, q, off, 3, ho, pos, dist, lens, st) == 1
        assert pos[0] == 0 and dist[0] == extra and lens[0] == 40
        r.close()
    idx.close()


# ---- 7. chunking ---------------------------------------------------------------------------------------------------------

CHILD = r"""
import sys
sys.path.insert(0, %(root)r)
import numpy as np
from kmer_index_amd import engine, synth
text = synth.ranks(91, 200_000, 4)
idx = engine.Index(text, 4, [8, 10, 12])
q, off, _ = synth.planted_reads_edit(92, text, 3000, 28, 4, 3)
r = idx.search_approx(q, off, 3, edit=True)
ho, pos, dist, st = r.host()
np.savez(%(out)r, ho=ho, pos=pos, dist=dist, lens=r.lengths(), st=st, chunks=r.counts()["n_chunks"])
print("edit child ok")
"""


@pytest.mark.parametrize("knobs", [{"KMX_APPROX_CHUNK_CANDIDATES": "4096"},          # candidate budget: inner chunks
                                   {"KMX_APPROX_CHUNK_PIECES": "1000"},              # piece bound: outer chunks of 250 queries
                                   {"KMX_APPROX_CHUNK_CANDIDATES": "20000", "KMX_APPROX_CHUNK_PIECES": "2000"}],
                         ids=["candidates", "pieces", "both"])
def test_chunked_batch_equals_one_chunk(engine, tmp_path, knobs):
    out = str(tmp_path / "chunked.npz")
    env = dict(os.environ)
    env.update(knobs)
    res = subprocess.run([sys.executable, "-c", CHILD % {"root": ROOT, "out": out}], capture_output=True, text=True, timeout=600, env=env)
    assert res.returncode == 0 and "edit child ok" in res.stdout, res.stdout[-2000:] + res.stderr[-4000:]
    got = np.load(out)
    assert int(got["chunks"]) > 1
    text = synth.ranks(91, 200_000, 4)
    idx = engine.Index(text, 4, [8, 10, 12])
    q, off, start = synth.planted_reads_edit(92, text, 3000, 28, 4, 3)
    ho, pos, dist, lens, st, r = _edit_search(idx, q, off, 3)
    assert r.counts()["n_chunks"] == 1
    for name, arr in (("ho", ho), ("pos", pos), ("dist", dist), ("lens", lens), ("st", st)):
        assert np.array_equal(got[name], arr), name
    n_hits = int(ho[40])
    assert compare_batch(text, q[:40 * 28], off[:41], 3, ho[:41], pos[:n_hits], dist[:n_hits], lens[:n_hits], st[:40]) == 40
    ek = _keys(ho, pos)
    want = (np.arange(3000, dtype=np.uint64) << np.uint64(32)) | start.astype(np.uint64)
    at = np.searchsorted(ek, want)
    assert np.all(at < ek.size) and np.array_equal(ek[at], want)         # every read's source start is a hit
    r.close()
    idx.close()


# ---- 8. concurrent calls, 9. prefix levels, 10. loaded and replicated indexes --------------------------------------------

def test_two_threads_with_and_without_the_flag(engine):
    text = synth.ranks(95, 300_000, 4)
    idx = engine.Index(text, 4, [10])
    q0, o0, _ = synth.planted_reads_edit(96, text, 4000, 30, 4, 2)
    q1, o1 = synth.planted_reads(97, text, 4000, 30, 4, 2)

    def call(t):
        if t == 0:
            r = idx.search_approx(q0, o0, 2, edit=True)
            out = r.host() + (r.lengths(),)
        else:
            r = idx.search_approx(q1, o1, 2)
            out = r.host()
        r.close()
        return out

    want = [call(0), call(1)]
    got = [None, None]
    errors = []

    def run(t):
        try:
            for _ in range(3):
                got[t] = call(t)
        except Exception as ex:          # noqa: BLE001 - reported below
            errors.append(ex)

    threads = [threading.Thread(target=run, args=(t,)) for t in range(2)]
    for th in threads:
        th.start()
    for th in threads:
        th.join()
    assert not errors, errors
    for t in range(2):
        assert len(want[t]) == len(got[t]) == 5 - t
        for a, b in zip(want[t], got[t]):
            assert np.array_equal(a, b)
    idx.close()


def test_prefix_levels_do_not_change_results(engine):
    text = synth.ranks(97, 200_000, 4)
    q, off, _ = synth.planted_reads_edit(98, text, 2000, 27, 4, 3)    # pieces of 6 and 7 letters: sub-k on k = 10
    a = engine.Index(text, 4, [10])
    b = engine.Index(text, 4, [10], prefix_levels=-1)
    ra = _edit_search(a, q, off, 3)
    rb = _edit_search(b, q, off, 3)
    for x, y in zip(ra[:5], rb[:5]):
        assert np.array_equal(x, y)
    ho, pos, dist, lens, st, _ = ra
    n_hits = int(ho[30])
    assert compare_batch(text, q[:30 * 27], off[:31], 3, ho[:31], pos[:n_hits], dist[:n_hits], lens[:n_hits], st[:30]) == 30
    a.close()
    b.close()


def test_loaded_and_replicated_indexes(engine, tmp_path):
    text = synth.ranks(42, 50_000, 5)
    q, off, _ = synth.planted_reads_edit(43, text, 60, 30, 5, 2)
    idx = engine.Index(text, 5, [10])
    want = _edit_search(idx, q, off, 2)[:5]
    assert compare_batch(text, q, off, 2, *want) == 60
    path = str(tmp_path / "ix.kmx")
    idx.save(path)
    idx.close()
    loaded = engine.Index.load(path)
    rep = engine.Index(text, 5, [10], devices=[0, 0])
    for other in (loaded, rep):
        got = _edit_search(other, q, off, 2)[:5]
        for x, y in zip(want, got):
            assert np.array_equal(x, y)
        other.close()
