"""What the tests of tests/test_variants_gpu.py share with the child processes they start (a tuning variable is read once per
process, so a test of one runs a child): the device-buffer search, the comparison with the oracle's answer, and the batches of the
k_lookup, cell and latency-path cases."""
import numpy as np

from kmer_index_amd import synth
from tests import variant_layouts as vl

K = 6


def dev_search(idx, qranks, qoff, res, flags=0):
    """kmx_search_batch_device on queries uploaded with torch: ((hit_off, positions, status, kinds), paths)."""
    import torch
    d_q = torch.from_numpy(np.ascontiguousarray(qranks, np.uint8)).cuda()
    d_o = torch.from_numpy(np.ascontiguousarray(qoff, np.uint64).view(np.int64)).cuda()
    torch.cuda.synchronize()
    idx.search_device(d_q.data_ptr(), d_o.data_ptr(), qoff.size - 1, flags=flags, result=res)
    out = res.host()
    return out, res.paths()


def same_answers(got, want, what):
    ho, pos, st, _ = got
    o_off, o_pos, o_st = want
    assert np.array_equal(st, o_st.astype(np.uint8)), ("status", what)
    assert np.array_equal(ho, o_off), ("hit_off", what)
    assert np.array_equal(pos, o_pos), ("positions", what)


def lookup_text_and_batch(nq):
    """50 000 letters of DNA4, k = 7: as a dense table the index has cells of 8 and at most four positions per key (tiny_cells).
    Queries: exact (planted and random: some absent), sub-k (4, 5 letters), two-part (14, and 10 = 7 + a rest)."""
    text = synth.ranks(77, 50_000, 4)
    q, off = synth.mixed_queries(78, text, nq, [7, 7, 7, 7, 5, 14, 10, 4, 7, 7], 4, planted_frac=0.6)
    return text, q, off


def cells_case(n):
    """DNA4, k = 6 (4096 keys, dense): n letters give c = n / 4096 positions per key.  Every key once as an exact query (the
    histogram names the ones whose buckets hold 2^shift - 1, 2^shift and 2^shift + 1 positions), then sub-k queries and the tail."""
    text = synth.ranks(500 + n, n, 4)
    hist = np.bincount(vl.kmer_codes(text, K), minlength=4 ** K)
    qs = [vl.decode(c, K) for c in range(4 ** K)]
    qs += [text[s:s + m].copy() for m in (5, 4, 3) for s in (0, 777, n // 2)] + [text[n - m:].copy() for m in (5, 4, 3)]
    off = np.zeros(len(qs) + 1, np.uint64)
    off[1:] = np.cumsum([len(x) for x in qs])
    return text, hist, np.concatenate(qs).astype(np.uint8), off


def small_batches():
    """Host-buffer searches of 1 .. 40 queries on the index of cells of 16: ('small' | 'general', digest of every answer)."""
    from kmer_index_amd import engine
    import hashlib
    from oracle import orc
    from tests.helpers import digest
    text, hist, q, off = cells_case(42_900)
    idx = engine.Index(text, 4, [K], table=engine.TABLE_DENSE)
    assert idx.paths()["cell_shift"] == [4], idx.paths()
    oidx = orc.Index(text, 4, [K])
    edge = np.nonzero((hist >= 15) & (hist <= 17))[0]
    digests, small = [], set()
    res = engine.Result()
    for nq in range(1, 41):
        ids = [int(edge[(7 * nq + j) % edge.size]) if j % 2 else 4 ** K + (nq + j) % 12 for j in range(nq)]     # edge buckets and sub-k queries
        qs = [q[int(off[i]):int(off[i + 1])] for i in ids]
        o = np.zeros(nq + 1, np.uint64)
        o[1:] = np.cumsum([len(x) for x in qs])
        r = idx.search(np.concatenate(qs), o, result=res)
        ho, pos, st, kd = r.host()
        same_answers((ho, pos, st, kd), oidx.search_batch(np.concatenate(qs), o, mode=orc.MODE_INTENDED)[:3], nq)
        small.add(r.paths()["small"])
        digests.append(digest(ho, pos) ^ int(st.sum()))
    res.close()
    idx.close()
    return ("small" if True in small else "general"), hashlib.sha1(np.array(digests, np.uint64).tobytes()).hexdigest()
