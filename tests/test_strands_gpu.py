"""Both-strand approximate search on the GPU (kmx_search_approx_strands, kmx_approx_strands) against the independent numpy
checker: positions, strands, distances and (edit) lengths equal, hits ordered by (position, strand)."""
import os
import subprocess
import sys
import threading

import numpy as np
import pytest

from kmer_index_amd import synth
from tests.helpers import CASES, pack, random_involution
from tests.strand_naive import compare_batch, revcomp, strand_naive

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_PARITY = 60_000          # letters of text per parity case (the checker is O(n m) per query and strand)
DNA4 = np.array([3, 2, 1, 0], np.uint8)


def table_for(engine, sigma, seed):
    """The natural complement where the alphabet has one, a seeded random involution elsewhere."""
    return engine.complement_table(sigma) if sigma in (4, 5, 15) else random_involution(sigma, seed)


def strand_search(idx, qranks, qoff, e, edit, comp):
    """(hit_off, positions, strands, distances, lengths or None, status, counts)"""
    r = idx.search_approx(qranks, qoff, e, edit=edit, strands=True, complement=comp)
    ho, pos, dist, st = r.host()
    out = (ho, pos, r.strands(), dist, r.lengths() if edit else None, st, r.counts())
    r.close()
    return out


def check(text, qranks, qoff, e, comp, got, edit):
    ho, pos, strands, dist, lens, st, _ = got
    return compare_batch(text, qranks, qoff, e, comp, ho, pos, strands, dist, lens, st, edit=edit)


def _queries(text, sigma, ks, e, seed, comp):
    """The length ladder of tests/test_approx_gpu.py (pieces below k, equal to k, above k, a sum of two ks); per length
    uniform random reads, reads planted with 0 .. e and with e + 1 substitutions and reads planted within the last 14
    letters; a seeded half of the planted reads is reverse-complemented."""
    k0, k1 = min(ks), max(ks)
    piece_lengths = sorted({max(1, k0 - 2), k0, k1 + 3} | ({ks[0] + ks[1]} if len(ks) > 1 else set()))
    lengths = [pl * (e + 1) + (j % (e + 1)) for j, pl in enumerate(piece_lengths)]
    n = text.size
    z = synth.u64_stream(seed, 4096)
    zi = 0
    qs = []
    flipped = 0
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
                if (int(z[zi]) >> 20) & 1:
                    q = revcomp(q, comp)
                    flipped += 1
                zi += 1
            qs.append(q)
    assert 0 < flipped < len(qs)
    return pack(qs)


# ---- 1. parity with the checker -----------------------------------------------------------------------------------------

# both tables where a dense table can exist (sigma^k <= 2^30 keys for every k)
PARITY_PARAMS = [(c, t) for c in CASES for t in ("open", "dense") if t == "open" or c[1] ** max(c[3]) <= 1 << 30]


@pytest.mark.parametrize("edit", [False, True], ids=["hamming", "edit"])
@pytest.mark.parametrize("case,table", PARITY_PARAMS, ids=[f"{c[0]}-{t}" for c, t in PARITY_PARAMS])
def test_parity_with_checker(engine, case, table, edit):
    name, sigma, _, ks, _ = case
    text = synth.ranks(1000 + len(name), N_PARITY, sigma)
    comp = table_for(engine, sigma, 77)
    idx = engine.Index(text, sigma, ks, table=engine.TABLE_OPEN if table == "open" else engine.TABLE_DENSE)
    for e in range(4):
        qranks, qoff = _queries(text, sigma, ks, e, 291 + e, comp)
        got = strand_search(idx, qranks, qoff, e, edit, comp)
        ho, pos, strands, dist, lens, st, c = got
        assert set(np.unique(st).tolist()) <= {engine.Q_OK, engine.Q_SUBK_FANOUT}
        checked = check(text, qranks, qoff, e, comp, got, edit)
        assert checked >= (qoff.size - 1) // 2, (e, checked)
        assert c["n_hits"] == pos.size and c["n_chunks"] == 1 and c["nq"] == qoff.size - 1
        assert (strands == 0).any() and (strands == 1).any()
    idx.close()


@pytest.mark.parametrize("edit", [False, True], ids=["hamming", "edit"])
def test_planted_strand_reads_all_served_and_found(engine, edit):
    text = synth.ranks(1234, 60_000, 4)
    idx = engine.Index(text, 4, [10])
    nq, m, e = 64, 30, 2
    gen = synth.planted_reads_edit_strands if edit else synth.planted_reads_strands
    q, off, strand, start = gen(55, text, nq, m, 4, e, DNA4)
    got = strand_search(idx, q, off, e, edit, DNA4)
    ho, pos, strands, dist, lens, st, _ = got
    assert np.all(st == engine.Q_OK)
    assert check(text, q, off, e, DNA4, got, edit) == nq
    for i in range(nq):
        a, b = int(ho[i]), int(ho[i + 1])
        assert np.any((pos[a:b] == start[i]) & (strands[a:b] == strand[i])), i
    assert 0 < int(strand.sum()) < nq
    idx.close()


# ---- 2. queries that are their own reverse complement: every hit twice, forward first -------------------------------------

@pytest.mark.parametrize("ks", [[5], [8, 10, 12]])
def test_self_reverse_complementary_queries_on_a_periodic_text(engine, ks):
    rng = np.random.default_rng(5)
    text = np.tile(np.array([0, 3], np.uint8), 30_000)        # ATAT...: every even-length window of it is its own rc
    noise = rng.integers(0, text.size, 200)
    text[noise] = rng.integers(0, 4, noise.size).astype(np.uint8)
    idx = engine.Index(text, 4, ks)
    qs = [np.tile(np.array([0, 3], np.uint8), m // 2) for m in (16, 24, 30)]
    half = np.array([0, 3, 0, 1, 0, 3, 0, 3, 0, 3], np.uint8)
    qs.append(np.concatenate([half, revcomp(half, DNA4)]))     # one substitution off the period, still its own rc
    for q in qs:
        assert np.array_equal(revcomp(q, DNA4), q)
    qranks, qoff = pack(qs)
    for edit in (False, True):
        for e in range(4):
            got = strand_search(idx, qranks, qoff, e, edit, DNA4)
            ho, pos, strands, dist, lens, st, _ = got
            assert check(text, qranks, qoff, e, DNA4, got, edit) == len(qs)
            assert pos.size % 2 == 0 and int(np.diff(ho.astype(np.int64)).max()) > 2000
            assert np.array_equal(pos[0::2], pos[1::2]) and np.array_equal(dist[0::2], dist[1::2])
            assert not strands[0::2].any() and strands[1::2].all()
            if edit:
                assert np.array_equal(lens[0::2], lens[1::2])
    idx.close()


# ---- 3. e = 0 is the exact search of q and of rc(q) ------------------------------------------------------------------------

def test_zero_distance_equals_exact_search_of_both_strands(engine):
    text = synth.ranks(77, 300_000, 4)
    idx = engine.Index(text, 4, [8, 10, 12])
    qranks, qoff = synth.mixed_queries(78, text, 3000, list(range(3, 40)), 4)
    flip = (synth.u64_stream(79, 3000) & np.uint64(1)).astype(bool)
    rc_all = synth.revcomp(qranks, qoff, DNA4)
    qranks = np.where(np.repeat(flip, np.diff(qoff.astype(np.int64))), rc_all, qranks).astype(np.uint8)
    rc = synth.revcomp(qranks, qoff, DNA4)                     # made on the host
    ho, pos, strands, dist, _, st, _ = strand_search(idx, qranks, qoff, 0, False, DNA4)
    fh, fpos, fst, _ = idx.search(qranks, qoff).host()
    rh, rpos, rst, _ = idx.search(rc, qoff).host()
    ok = np.nonzero((fst == engine.Q_OK) & (rst == engine.Q_OK))[0]
    assert ok.size > 2000 and not dist.any()
    assert np.all(st[ok] == engine.Q_OK)
    both = 0
    for i in ok:
        a, b = int(ho[i]), int(ho[i + 1])
        p, s = pos[a:b], strands[a:b]
        assert np.array_equal(p[s == 0], fpos[int(fh[i]):int(fh[i + 1])]), i
        assert np.array_equal(p[s == 1], rpos[int(rh[i]):int(rh[i + 1])]), i
        both += int((s == 0).any() and (s == 1).any())
    assert (strands == 1).sum() > 1000 and (strands == 0).sum() > 1000 and both > 0
    idx.close()


# ---- 4. the table is honoured, not assumed -----------------------------------------------------------------------------------

def test_identity_and_an_involution_on_aa20_differ(engine):
    sigma = 20
    text = synth.ranks(31, 60_000, sigma)
    idx = engine.Index(text, sigma, [5])
    ident = np.arange(sigma, dtype=np.uint8)
    inv = random_involution(sigma, 5)
    assert not np.array_equal(inv, ident) and np.array_equal(inv[inv], ident)
    rng = np.random.default_rng(32)
    qs = []
    for t in range(24):
        s = int(rng.integers(0, text.size - 21))
        q = text[s:s + 21].copy()
        qs.append(q if t % 3 == 0 else revcomp(q, ident if t % 3 == 1 else inv))    # forward, reversed, rc under inv
    qranks, qoff = pack(qs)
    for edit in (False, True):
        a = strand_search(idx, qranks, qoff, 2, edit, ident)
        b = strand_search(idx, qranks, qoff, 2, edit, inv)
        assert check(text, qranks, qoff, 2, ident, a, edit) == 24
        assert check(text, qranks, qoff, 2, inv, b, edit) == 24
        assert not (np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2]))
        for t in range(24):                                    # a read turned under one table is found under that table only
            na, nb = int(a[0][t + 1] - a[0][t]), int(b[0][t + 1] - b[0][t])
            assert (na >= 1) == (t % 3 != 2) and (nb >= 1) == (t % 3 != 1), t
    idx.close()


# ---- 5. one call equals two plain calls merged on the host --------------------------------------------------------------------

@pytest.mark.parametrize("edit", [False, True], ids=["hamming", "edit"])
def test_equals_two_plain_calls_merged_on_the_host(engine, edit):
    text = synth.ranks(77, 300_000, 4)
    idx = engine.Index(text, 4, [8, 10, 12])
    nq, e = 2000, 3
    gen = synth.planted_reads_edit_strands if edit else synth.planted_reads_strands
    q, off, _, _ = gen(181, text, nq, 32, 4, e, DNA4)
    rc = synth.revcomp(q, off, DNA4)
    plain_before = []
    parts = []
    for strand, batch in enumerate((q, rc)):
        r = idx.search_approx(batch, off, e, edit=edit)
        ho, pos, dist, st = r.host()
        lens = r.lengths() if edit else np.zeros(pos.size, np.uint32)
        plain_before.append((ho, pos, dist, st, lens))
        assert np.all(st == engine.Q_OK)
        qi = np.repeat(np.arange(nq), np.diff(ho.astype(np.int64)))
        parts.append((qi, pos, np.full(pos.size, strand, np.uint8), dist, lens))
        r.close()
    qi, pos, strand, dist, lens = (np.concatenate([p[k] for p in parts]) for k in range(5))
    order = np.lexsort((strand, pos, qi))
    want_ho = np.zeros(nq + 1, np.uint64)
    np.cumsum(np.bincount(qi, minlength=nq), out=want_ho[1:])
    got = strand_search(idx, q, off, e, edit, DNA4)
    ho, gpos, gstrands, gdist, glens, st, c = got
    assert np.all(st == engine.Q_OK) and np.array_equal(ho, want_ho)
    assert np.array_equal(gpos, pos[order]) and np.array_equal(gstrands, strand[order]) and np.array_equal(gdist, dist[order])
    if edit:
        assert np.array_equal(glens, lens[order])
    assert gpos.size >= nq and (gstrands == 1).sum() >= nq // 4 and c["n_hits"] == gpos.size
    # plain results on the same index are what they were before the strand call
    for batch, before in zip((q, rc), plain_before):
        r = idx.search_approx(batch, off, e, edit=edit)
        after = r.host() + ((r.lengths(),) if edit else (before[4],))
        for x, y in zip(before, after):
            assert np.array_equal(x, y)
        r.close()
    idx.close()


# ---- 6. chunking ---------------------------------------------------------------------------------------------------------

CHILD = r"""
import sys
sys.path.insert(0, %(root)r)
import numpy as np
from kmer_index_amd import engine, synth
edit = %(edit)r
comp = np.array([3, 2, 1, 0], np.uint8)
text = synth.ranks(91, 200_000, 4)
idx = engine.Index(text, 4, [8, 10, 12])
gen = synth.planted_reads_edit_strands if edit else synth.planted_reads_strands
q, off, _, _ = gen(92, text, 1500, 28, 4, 3, comp)
r = idx.search_approx(q, off, 3, edit=edit, strands=True, complement=comp)
ho, pos, dist, st = r.host()
c = r.counts()
np.savez(%(out)r, ho=ho, pos=pos, dist=dist, st=st, strands=r.strands(), lens=r.lengths() if edit else np.zeros(0, np.uint32),
         chunks=c["n_chunks"], cand=c["n_candidates"])
print("strands child ok")
"""


@pytest.mark.parametrize("edit", [False, True], ids=["hamming", "edit"])
@pytest.mark.parametrize("knobs", [{"KMX_APPROX_CHUNK_CANDIDATES": "4096"},          # candidate budget: inner chunks
                                   {"KMX_APPROX_CHUNK_CANDIDATES": "8"},             # less than one pair's candidates
                                   {"KMX_APPROX_CHUNK_PIECES": "1000"},              # piece bound: outer chunks of 125 pairs
                                   {"KMX_APPROX_CHUNK_CANDIDATES": "20000", "KMX_APPROX_CHUNK_PIECES": "2000"}],
                         ids=["candidates", "below_one_pair", "pieces", "both"])
def test_chunked_batch_equals_one_chunk(engine, tmp_path, knobs, edit):
    out = str(tmp_path / "chunked.npz")
    env = dict(os.environ)
    env.update(knobs)
    res = subprocess.run([sys.executable, "-c", CHILD % {"root": ROOT, "out": out, "edit": edit}], capture_output=True, text=True, timeout=900,
                         env=env)
    assert res.returncode == 0 and "strands child ok" in res.stdout, res.stdout[-2000:] + res.stderr[-4000:]
    got = np.load(out)
    assert int(got["chunks"]) > 1
    text = synth.ranks(91, 200_000, 4)
    idx = engine.Index(text, 4, [8, 10, 12])
    gen = synth.planted_reads_edit_strands if edit else synth.planted_reads_strands
    q, off, strand, start = gen(92, text, 1500, 28, 4, 3, DNA4)
    one = strand_search(idx, q, off, 3, edit, DNA4)
    ho, pos, strands, dist, lens, st, c = one
    assert c["n_chunks"] == 1 and c["n_candidates"] == int(got["cand"])
    if knobs.get("KMX_APPROX_CHUNK_CANDIDATES") == "8":
        per_pair = c["n_candidates"] / 1500
        assert per_pair > 8 and int(got["chunks"]) == 1500, per_pair        # one pair per chunk, each over the budget
    for name, arr in (("ho", ho), ("pos", pos), ("dist", dist), ("st", st), ("strands", strands)):
        assert got[name].dtype == arr.dtype and got[name].tobytes() == arr.tobytes(), name
    if edit:
        assert got["lens"].tobytes() == lens.tobytes()
    n_hits = int(ho[30])
    head = (ho[:31], pos[:n_hits], strands[:n_hits], dist[:n_hits], lens[:n_hits] if edit else None, st[:30], None)
    assert check(text, q[:30 * 28], off[:31], 3, DNA4, head, edit) == 30
    for i in range(1500):                                                   # every read's source start, on its strand
        a, b = int(ho[i]), int(ho[i + 1])
        assert np.any((pos[a:b] == start[i]) & (strands[a:b] == strand[i])), i
    idx.close()


# ---- 7. statuses, 8. refused arguments ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("edit", [False, True], ids=["hamming", "edit"])
def test_statuses(engine, edit):
    text = synth.ranks(81, 5000, 4)
    idx = engine.Index(text, 4, [14], query_size_range=60)
    e = 2
    qs = [text[300:450].copy(),                       # served
          np.zeros(0, np.uint8),                      # empty
          revcomp(text[1000:1150], DNA4),             # served, on the reverse strand
          np.array([0, 1, 7, 2, 3, 0, 1], np.uint8),  # a letter outside the alphabet
          np.concatenate([text[2000:2075], [9], text[2076:2150]]).astype(np.uint8),    # ... in the middle of a read
          text[:150].copy(),                          # served
          np.array([1, 2], np.uint8),                 # m <= e
          text[100:100 + 3 * 60].copy(),              # longest piece == range
          np.array([1, 2, 3, 0, 1, 2], np.uint8),     # pieces of two letters: over the sub-k fan-out limit
          revcomp(text[4000:4000 + 177], DNA4)]       # served (pieces of 59 letters), on the reverse strand
    qranks, qoff = pack(qs)
    got = strand_search(idx, qranks, qoff, e, edit, DNA4)
    ho, pos, strands, dist, lens, st, _ = got
    OK = engine.Q_OK
    assert st.tolist() == [OK, engine.Q_EMPTY_QUERY, OK, engine.Q_BAD_RANK, engine.Q_BAD_RANK, OK, engine.Q_TOO_SHORT, engine.Q_TOO_LONG,
                           engine.Q_SUBK_FANOUT, OK]
    r = idx.search_approx(qranks, qoff, e, edit=edit)
    assert st.tolist() == r.host()[3].tolist()
    r.close()
    assert check(text, qranks, qoff, e, DNA4, got, edit) == 4               # ... and every other query without hits
    for i, (p, s) in {0: (300, 0), 2: (1000, 1), 5: (0, 0), 9: (4000, 1)}.items():
        a, b = int(ho[i]), int(ho[i + 1])
        assert np.any((pos[a:b] == p) & (strands[a:b] == s) & (dist[a:b] == 0)), i
    idx.close()


def test_invalid_tables_and_wrong_accessors_are_refused(engine):
    text = synth.ranks(83, 4000, 4)
    idx = engine.Index(text, 4, [5])
    q, off = synth.planted_reads(84, text, 10, 20, 4, 1)
    for bad, word in (([1, 2, 0, 3], "involution"), ([3, 2, 1, 4], "outside"), ([0, 0, 2, 3], "involution")):
        with pytest.raises(engine.KmxError) as ex:
            idx.search_approx(q, off, 1, strands=True, complement=np.array(bad, np.uint8))
        assert ex.value.status == 1 and word in str(ex.value) and "kmx_search_approx_strands" in str(ex.value)
    with pytest.raises(ValueError):
        idx.search_approx(q, off, 1, strands=True, complement=np.array([1, 0], np.uint8))
    plain = idx.search_approx(q, off, 1)
    with pytest.raises(engine.KmxError) as ex:
        plain.strands()
    assert ex.value.status == 1 and "kmx_approx_strands" in str(ex.value)
    plain.close()
    r = idx.search_approx(q, off, 1, strands=True)
    assert r.strands().size == r.counts()["n_hits"] >= 10
    with pytest.raises(engine.KmxError):
        r.lengths()                                                         # not a result of a call with KMX_APPROX_EDIT
    r.close()
    r = idx.search_approx(q, off, 1, edit=True, strands=True)
    assert r.lengths().size == r.strands().size == r.counts()["n_hits"]
    r.close()
    aa = engine.Index(synth.ranks(85, 4000, 20), 20, [3])
    with pytest.raises(ValueError):
        aa.search_approx(q, off, 1, strands=True)                           # no natural complement: a table is needed
    aa.close()
    idx.close()


# ---- 9. concurrent calls, 10. loaded and replicated indexes ---------------------------------------------------------------

def test_two_threads_with_and_without_strands(engine):
    text = synth.ranks(95, 300_000, 4)
    idx = engine.Index(text, 4, [10])
    q0, o0, _, _ = synth.planted_reads_strands(96, text, 4000, 30, 4, 2, DNA4)
    q1, o1 = synth.planted_reads(97, text, 4000, 30, 4, 2)

    def call(t):
        if t == 0:
            return strand_search(idx, q0, o0, 2, False, DNA4)[:4]
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
        assert len(want[t]) == len(got[t]) == 4
        for a, b in zip(want[t], got[t]):
            assert np.array_equal(a, b)
    idx.close()


def test_loaded_and_replicated_indexes(engine, tmp_path):
    text = synth.ranks(42, 50_000, 5)
    comp = engine.complement_table(5)
    q, off, _, _ = synth.planted_reads_edit_strands(43, text, 60, 30, 5, 2, comp)
    idx = engine.Index(text, 5, [10])
    want = {edit: strand_search(idx, q, off, 2, edit, None) for edit in (False, True)}      # the default table of sigma 5
    for edit in (False, True):
        assert check(text, q, off, 2, comp, want[edit], edit) == 60
    path = str(tmp_path / "ix.kmx")
    idx.save(path)
    idx.close()
    loaded = engine.Index.load(path)
    rep = engine.Index(text, 5, [10], devices=[0, 0])
    for other in (loaded, rep):
        for edit in (False, True):
            got = strand_search(other, q, off, 2, edit, comp)
            for x, y in zip(want[edit][:6], got[:6]):
                assert (x is None and y is None) or np.array_equal(x, y)
        other.close()
