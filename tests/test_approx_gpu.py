"""Approximate search on the GPU (kmx_search_approx, kmx_index_text) against the independent numpy checker."""
import os
import subprocess
import sys
import threading

import numpy as np
import pytest

from kmer_index_amd import synth
from tests.approx_naive import compare_batch
from tests.helpers import CASES, pack

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- 1. the text reconstructed from the index -------------------------------------------------------------------------

TEXT_CASES = [("dna4_k5", 4, [5]), ("dna4_k10", 4, [10]), ("dna5_k10", 5, [10]), ("aa20_k5", 20, [5]),
              ("s15_k345", 15, [3, 4, 5]), ("s15_k81012", 15, [8, 10, 12])]
# both tables where a dense table can exist (sigma^k <= 2^30 keys for every k)
TEXT_PARAMS = [(c, t) for c in TEXT_CASES for t in ("open", "dense") if t == "open" or c[1] ** max(c[2]) <= 1 << 30]


@pytest.mark.parametrize("case,table", TEXT_PARAMS, ids=[f"{c[0]}-{t}" for c, t in TEXT_PARAMS])
def test_index_text_equals_input(engine, case, table):
    name, sigma, ks = case
    text = synth.ranks(300 + len(name), 60_000, sigma)
    idx = engine.Index(text, sigma, ks, table=engine.TABLE_OPEN if table == "open" else engine.TABLE_DENSE)
    assert np.array_equal(idx.text(), text)
    w = 2 if sigma <= 4 else 4 if sigma <= 16 else 8
    assert idx.text_packed_bytes() >= (text.size * w + 63) // 64 * 8
    idx.close()


def test_index_text_short_loaded_and_replicated(engine, tmp_path):
    text = synth.ranks(41, 12, 4)                                   # n == kmax
    idx = engine.Index(text, 4, [8, 10, 12])
    assert np.array_equal(idx.text(), text)
    idx.close()
    text = synth.ranks(42, 50_000, 5)
    idx = engine.Index(text, 5, [10])
    path = str(tmp_path / "ix.kmx")
    idx.save(path)
    idx.close()
    loaded = engine.Index.load(path)
    assert np.array_equal(loaded.text(), text)
    loaded.close()
    rep = engine.Index(text, 5, [10], devices=[0, 0])
    assert np.array_equal(rep.text(), text)
    q, off = synth.planted_reads(43, text, 50, 30, 5, 2)
    ho, pos, mm, st = rep.search_approx(q, off, 2).host()
    assert compare_batch(text, q, off, 2, ho, pos, mm, st) == 50
    rep.close()


# ---- 2. parity with the checker -----------------------------------------------------------------------------------------

def _queries(text, sigma, ks, e, seed):
    """Lengths whose pieces fall below k, equal k, exceed k and (several ks) hit sums of two ks; per length uniform random
    reads, reads planted with 0..e and with e + 1 substitutions, and reads planted within the last 14 letters."""
    k0, k1 = min(ks), max(ks)
    piece_lengths = sorted({max(1, k0 - 2), k0, k1 + 3} | ({ks[0] + ks[1]} if len(ks) > 1 else set()))
    lengths = [pl * (e + 1) + (j % (e + 1)) for j, pl in enumerate(piece_lengths)]
    n = text.size
    z = synth.u64_stream(seed, 4096)
    zi = 0
    qs = []
    for m in lengths:
        for t in range(8):
            kind = t % 4
            if kind == 0:
                q = synth.ranks(seed * 7919 + m * 31 + t, m, sigma)
            else:
                if kind == 3:
                    s = n - m - int(z[zi] % np.uint64(15))
                else:
                    s = int(z[zi] % np.uint64(n - m + 1))
                zi += 1
                q = text[s:s + m].copy()
                d = (e + 1) if kind == 2 else int(z[zi] % np.uint64(e + 1))
                zi += 1
                cols = np.linspace(0, m - 1, num=max(d, 1), dtype=np.int64)[:d] if d else []
                for c in cols:
                    q[c] = (int(q[c]) + 1 + int(z[zi] % np.uint64(sigma - 1))) % sigma
                    zi += 1
            qs.append(q)
    return pack(qs)


@pytest.mark.parametrize("table", ["open", "dense"])
@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_parity_with_checker(engine, case, table):
    name, sigma, n, ks, _ = case
    text = synth.ranks(1000 + len(name), n, sigma)
    idx = engine.Index(text, sigma, ks, table=engine.TABLE_OPEN if table == "open" else engine.TABLE_DENSE)
    for e in range(4):
        qranks, qoff = _queries(text, sigma, ks, e, seed=91 + e)
        r = idx.search_approx(qranks, qoff, e)
        ho, pos, mm, st = r.host()
        assert set(np.unique(st).tolist()) <= {engine.Q_OK, engine.Q_SUBK_FANOUT}
        checked = compare_batch(text, qranks, qoff, e, ho, pos, mm, st)
        assert checked >= (qoff.size - 1) // 2, (e, checked)
        c = r.counts()
        assert c["n_hits"] == pos.size and c["n_chunks"] == 1 and c["n_candidates"] >= pos.size
        r.close()
    idx.close()


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
        ho, pos, mm, st = idx.search_approx(qranks, qoff, e).host()
        compare_batch(text, qranks, qoff, e, ho, pos, mm, st)
        assert int(np.diff(ho.astype(np.int64)).max()) > 1000
    idx.close()


# ---- 3. e = 0 is the exact search ---------------------------------------------------------------------------------------

def test_zero_substitutions_equal_exact_search(engine):
    text = synth.ranks(77, 300_000, 4)
    idx = engine.Index(text, 4, [8, 10, 12])
    qranks, qoff = synth.mixed_queries(78, text, 3000, list(range(3, 40)), 4)
    ho, pos, mm, st = idx.search_approx(qranks, qoff, 0).host()
    eh, epos, est, _ = idx.search(qranks, qoff).host()
    ok = np.nonzero(est == engine.Q_OK)[0]
    assert ok.size > 2000
    assert np.array_equal(st[ok], est[ok])
    assert not mm.any()
    for i in ok:
        assert np.array_equal(pos[int(ho[i]):int(ho[i + 1])], epos[int(eh[i]):int(eh[i + 1])]), i
    idx.close()


# ---- 4. statuses --------------------------------------------------------------------------------------------------------

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
    ho, pos, mm, st = idx.search_approx(qranks, qoff, e).host()
    assert st.tolist() == [engine.Q_EMPTY_QUERY, engine.Q_BAD_RANK, engine.Q_TOO_SHORT, engine.Q_TOO_LONG, engine.Q_SUBK_FANOUT,
                           engine.Q_OK, engine.Q_OK]
    assert ho[5] == 0 and pos[int(ho[5]):int(ho[6])].tolist() == [0] and pos[int(ho[6]):int(ho[7])].tolist() == [4000]
    compare_batch(text, qranks, qoff, e, ho, pos, mm, st)
    idx.close()
    # m > n: served, no hits
    small = synth.ranks(83, 40, 4)
    idx = engine.Index(small, 4, [5])
    q = np.concatenate([small, small[:6]])
    ho, pos, mm, st = idx.search_approx(q, np.array([0, q.size], np.uint64), 3).host()
    assert st[0] == engine.Q_OK and ho[1] == 0
    idx.close()


# ---- 5. chunking ---------------------------------------------------------------------------------------------------------

CHILD = r"""
import sys
sys.path.insert(0, %(root)r)
import numpy as np
from kmer_index_amd import engine, synth
text = synth.ranks(91, 200_000, 4)
idx = engine.Index(text, 4, [8, 10, 12])
q, off = synth.planted_reads(92, text, 3000, 28, 4, 3)
r = idx.search_approx(q, off, 3)
ho, pos, mm, st = r.host()
np.savez(%(out)r, ho=ho, pos=pos, mm=mm, st=st, chunks=r.counts()["n_chunks"])
print("approx child ok")
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
    assert res.returncode == 0 and "approx child ok" in res.stdout, res.stdout[-2000:] + res.stderr[-4000:]
    got = np.load(out)
    assert int(got["chunks"]) > 1
    text = synth.ranks(91, 200_000, 4)
    idx = engine.Index(text, 4, [8, 10, 12])
    q, off = synth.planted_reads(92, text, 3000, 28, 4, 3)
    r = idx.search_approx(q, off, 3)
    assert r.counts()["n_chunks"] == 1
    ho, pos, mm, st = r.host()
    for name, arr in (("ho", ho), ("pos", pos), ("mm", mm), ("st", st)):
        assert np.array_equal(got[name], arr), name
    assert compare_batch(text, q[:40 * 28], off[:41], 3, ho[:41], pos, mm, st[:40]) == 40
    idx.close()


# ---- 6. concurrent calls, 7. prefix levels ------------------------------------------------------------------------------

def test_two_threads_on_one_index(engine):
    text = synth.ranks(95, 300_000, 4)
    idx = engine.Index(text, 4, [10])
    batches = [synth.planted_reads(96 + t, text, 4000, 20 + 10 * t, 4, 1 + t) for t in range(2)]
    want = [idx.search_approx(q, o, 1 + t).host() for t, (q, o) in enumerate(batches)]
    got = [None, None]
    errors = []

    def run(t):
        try:
            for _ in range(3):
                got[t] = idx.search_approx(*batches[t], 1 + t).host()
        except Exception as ex:          # noqa: BLE001 - reported below
            errors.append(ex)

    threads = [threading.Thread(target=run, args=(t,)) for t in range(2)]
    for th in threads:
        th.start()
    for th in threads:
        th.join()
    assert not errors, errors
    for t in range(2):
        for a, b in zip(want[t], got[t]):
            assert np.array_equal(a, b)
    idx.close()


def test_prefix_levels_do_not_change_results(engine):
    text = synth.ranks(97, 200_000, 4)
    q, off = synth.planted_reads(98, text, 2000, 27, 4, 3)    # pieces of 6 and 7 letters: sub-k on k = 10
    a = engine.Index(text, 4, [10])
    b = engine.Index(text, 4, [10], prefix_levels=-1)
    ra = a.search_approx(q, off, 3).host()
    rb = b.search_approx(q, off, 3).host()
    for x, y in zip(ra, rb):
        assert np.array_equal(x, y)
    assert compare_batch(text, q[:30 * 27], off[:31], 3, ra[0][:31], ra[1], ra[2], ra[3][:30]) == 30
    a.close()
    b.close()
