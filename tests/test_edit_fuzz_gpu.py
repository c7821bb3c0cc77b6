"""Edit-distance search fuzz: 32 seeds, each drawing sigma, ks, table, text length, e, query lengths and reads that are random
or planted with edits of mixed kinds; every served query is compared in full (positions, distances, lengths) with the
independent numpy checker."""
import numpy as np
import pytest

from kmer_index_amd import synth
from tests.edit_naive import compare_batch
from tests.helpers import mutate, pack

pytestmark = pytest.mark.gpu

KS = {4: [[5], [10], [8, 10, 12], [7, 11]], 5: [[6], [10]], 15: [[3, 4, 5], [8]], 20: [[5], [3, 4]]}


@pytest.mark.parametrize("seed", range(32))
def test_edit_fuzz(engine, seed):
    rng = np.random.default_rng(9000 + seed)
    sigma = int(rng.choice(list(KS)))
    ks = KS[sigma][int(rng.integers(len(KS[sigma])))]
    n = int(rng.integers(max(ks) + 50, 20_000))
    text = synth.ranks(9500 + seed, n, sigma)
    table = [0, 1, 2][int(rng.integers(3))]
    idx = engine.Index(text, sigma, ks, table=table)
    e = int(rng.integers(4))
    qs = []
    for _ in range(24):
        m = int(rng.integers(e + 1, min(n, 4 * max(ks) * (e + 1)) + 1))
        if rng.random() < 0.3:
            q = rng.integers(0, sigma, m).astype(np.uint8)
        else:
            r = rng.random()
            s = int(rng.integers(0, n - m + 1)) if r < 0.7 else n - m - int(rng.integers(0, min(14, n - m) + 1)) if r < 0.85 else \
                int(rng.integers(0, min(e, n - m) + 1))
            q = mutate(text[s:s + m + e + 1], m, int(rng.integers(0, e + 2)), sigma, rng)
        qs.append(q)
    qranks, qoff = pack(qs)
    r = idx.search_approx(qranks, qoff, e, edit=True)
    ho, pos, dist, st = r.host()
    assert set(np.unique(st).tolist()) <= {engine.Q_OK, engine.Q_SUBK_FANOUT}, (seed, st)
    compare_batch(text, qranks, qoff, e, ho, pos, dist, r.lengths(), st)
    r.close()
    idx.close()
