"""Both-strand search fuzz: 32 seeds, each drawing sigma, ks, table kind, text kind (uniform or periodic with noise) and length,
e, mode (Hamming or edit), the complement table (natural, identity or a random involution) and reads that are random or
planted on either strand; every served query is compared in full with the independent numpy checker."""
import numpy as np
import pytest

from kmer_index_amd import synth
from tests.helpers import mutate, pack, random_involution
from tests.strand_naive import compare_batch, revcomp

pytestmark = pytest.mark.gpu

KS = {4: [[5], [10], [8, 10, 12], [7, 11]], 5: [[6], [10]], 15: [[3, 4, 5], [8]], 20: [[5], [3, 4]]}


@pytest.mark.parametrize("seed", range(32))
def test_strands_fuzz(engine, seed):
    rng = np.random.default_rng(19000 + seed)
    sigma = int(rng.choice(list(KS)))
    ks = KS[sigma][int(rng.integers(len(KS[sigma])))]
    n = int(rng.integers(max(ks) + 50, 20_000))
    if rng.random() < 0.3:                                      # periodic with noise: long hit lists on both strands
        period = rng.integers(0, sigma, int(rng.integers(2, 7))).astype(np.uint8)
        text = np.tile(period, n // period.size + 1)[:n].copy()
        noise = rng.integers(0, n, max(n // 200, 1))
        text[noise] = rng.integers(0, sigma, noise.size).astype(np.uint8)
    else:
        text = synth.ranks(19500 + seed, n, sigma)
    kind = int(rng.integers(3))
    if kind == 0 and sigma in (4, 5, 15):
        comp = engine.complement_table(sigma)
    elif kind == 1:
        comp = np.arange(sigma, dtype=np.uint8)
    else:
        comp = random_involution(sigma, 19900 + seed)
    table = [0, 1, 2][int(rng.integers(3))]
    idx = engine.Index(text, sigma, ks, table=table)
    e = int(rng.integers(4))
    edit = bool(rng.integers(2))
    qs = []
    for _ in range(24):
        m = int(rng.integers(e + 1, min(n, 4 * max(ks) * (e + 1)) + 1))
        if rng.random() < 0.3:
            q = rng.integers(0, sigma, m).astype(np.uint8)
        else:
            r = rng.random()
            s = int(rng.integers(0, n - m + 1)) if r < 0.7 else n - m - int(rng.integers(0, min(14, n - m) + 1)) if r < 0.85 else \
                int(rng.integers(0, min(e, n - m) + 1))
            if edit:
                q = mutate(text[s:s + m + e + 1], m, int(rng.integers(0, e + 2)), sigma, rng)
            else:
                q = text[s:s + m].copy()
                for c in rng.integers(0, m, int(rng.integers(0, e + 2))):
                    q[c] = (int(q[c]) + 1 + int(rng.integers(sigma - 1))) % sigma
            if rng.random() < 0.5:
                q = revcomp(q, comp)
        qs.append(q)
    qranks, qoff = pack(qs)
    r = idx.search_approx(qranks, qoff, e, edit=edit, strands=True, complement=comp)
    ho, pos, dist, st = r.host()
    assert set(np.unique(st).tolist()) <= {engine.Q_OK, engine.Q_SUBK_FANOUT}, (seed, st)
    compare_batch(text, qranks, qoff, e, comp, ho, pos, r.strands(), dist, r.lengths() if edit else None, st, edit=edit)
    r.close()
    idx.close()
