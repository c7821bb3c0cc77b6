"""tests/fold_naive.py against itself: the two statements of the fold agree, the doubled batch undoes itself, and the hand-made
cases of the contract come out as it says.  No device is needed."""
import numpy as np
import pytest

from tests import fold_naive as fn
from tests.chain_checks import same_mixed
from tests.helpers import pack

NAMES = ("locus", "strand", "dist", "start", "end", "second", "best2", "n_placed", "n_reverse", "n_ambiguous")
NO = fn.NO_BEST


def best_of(locus_off, dist):
    """best[] as kmx_loci_align defines it: the aligned locus of the read with the least (dist, index), relative to locus_off[r]."""
    best = np.full(len(locus_off) - 1, NO, np.uint32)
    for r in range(len(locus_off) - 1):
        a, b = int(locus_off[r]), int(locus_off[r + 1])
        keys = [(int(dist[l]), l - a) for l in range(a, b) if int(dist[l]) < fn.SKIPPED]
        if keys:
            best[r] = min(keys)[1]
    return best


def case(per_strand):
    """per_strand: for every internal read a list of (dist, start, end).  Returns the five arrays of the fold."""
    off = np.zeros(len(per_strand) + 1, np.uint64)
    off[1:] = np.cumsum([len(x) for x in per_strand])
    flat = [t for x in per_strand for t in x]
    dist = np.asarray([t[0] for t in flat], np.uint8)
    start = np.asarray([t[1] for t in flat], np.uint32)
    end = np.asarray([t[2] for t in flat], np.uint32)
    return off, dist, start, end, best_of(off, dist)


def random_case(seed):
    rng = np.random.default_rng(seed)
    per = []
    for _ in range(2 * int(rng.integers(0, 12))):
        loci = []
        for _ in range(int(rng.integers(0, 6)) if rng.random() < 0.9 else int(rng.integers(60, 140))):
            d = int(rng.choice([0, 1, 1, 2, 3, fn.SKIPPED, fn.NONE]))
            s = int(rng.integers(0, 60)) if d < fn.SKIPPED else 0
            e = s + int(rng.integers(0, 12)) if d < fn.SKIPPED else 0
            loci.append((d, s, e))
        per.append(loci)
    return case(per)


@pytest.mark.parametrize("seed", range(40))
def test_fold_equals_fold_loop(seed):
    args = random_case(seed)
    same_mixed(NAMES, fn.fold(*args), fn.fold_loop(*args))


@pytest.mark.parametrize("sigma,complement", [(4, [3, 2, 1, 0]), (5, [4, 2, 1, 3, 0]), (20, list(range(20)))])
def test_double_reads_of_rc_reads_gives_the_reads_back(sigma, complement):
    rng = np.random.default_rng(sigma)
    reads = [rng.integers(0, sigma, m).astype(np.uint8) for m in (0, 1, 2, 7, 64, 65, 150)]
    reads[3][0] = sigma                                       # letters outside the alphabet stay where the reversal puts them
    reads[4][-1] = 255
    ranks, roff = pack(reads)
    ranks2, roff2 = fn.double_reads(ranks, roff, complement, sigma)
    assert ranks2.dtype == np.uint8 and roff2.dtype == np.uint64
    assert roff2.size == 2 * len(reads) + 1 and int(roff2[-1]) == 2 * ranks.size
    rc = [ranks2[int(roff2[2 * i + 1]):int(roff2[2 * i + 2])] for i in range(len(reads))]
    for i, q in enumerate(reads):
        assert np.array_equal(ranks2[int(roff2[2 * i]):int(roff2[2 * i + 1])], q)
        assert np.array_equal(rc[i], fn.revcomp(q, complement, sigma))
    again, roff4 = fn.double_reads(*pack(rc), complement, sigma)
    for i, q in enumerate(reads):                             # the odd slots of the doubled rc reads are the reads
        assert np.array_equal(again[int(roff4[2 * i + 1]):int(roff4[2 * i + 2])], q)
    assert rc[3][-1] == sigma and rc[4][0] == 255


def both(args):
    got = fn.fold(*args)
    same_mixed(NAMES, got, fn.fold_loop(*args))
    return dict(zip(NAMES, got))


def test_tie_between_the_strands_goes_forward():
    r = both(case([[(2, 100, 150)], [(2, 400, 450)]]))
    assert r["locus"].tolist() == [0] and r["strand"].tolist() == [0] and r["dist"].tolist() == [2]
    assert r["second"].tolist() == [2] and r["best2"].tolist() == [0, NO]
    assert (r["n_placed"], r["n_reverse"], r["n_ambiguous"]) == (1, 0, 1)
    r = both(case([[(3, 100, 150)], [(2, 400, 450)]]))        # ... and the better strand wins where there is none
    assert r["locus"].tolist() == [1] and r["strand"].tolist() == [1] and r["second"].tolist() == [3]
    assert r["best2"].tolist() == [NO, 0] and (r["n_placed"], r["n_reverse"], r["n_ambiguous"]) == (1, 1, 0)


def test_overlapping_second_locus_is_no_runner_up():
    r = both(case([[(1, 100, 150), (3, 149, 190)], []]))
    assert r["locus"].tolist() == [0] and r["second"].tolist() == [255] and r["n_ambiguous"] == 0
    r = both(case([[(1, 100, 150), (3, 150, 190)], []]))      # touching intervals share no letter
    assert r["second"].tolist() == [3]
    r = both(case([[(1, 100, 150)], [(3, 120, 170)]]))        # the same letters on the other strand are another placement
    assert r["second"].tolist() == [3]


def test_disjoint_locus_at_the_same_distance_is_ambiguous():
    r = both(case([[(1, 100, 150), (1, 900, 950)], []]))
    assert r["locus"].tolist() == [0] and r["second"].tolist() == [1] and r["n_ambiguous"] == 1


def test_empty_winner_interval_overlaps_nothing():
    r = both(case([[(0, 70, 70), (0, 60, 80)], []]))           # (the empty read: every locus aligns with nothing at distance 0)
    assert r["locus"].tolist() == [0] and r["start"].tolist() == [70] and r["end"].tolist() == [70]
    assert r["second"].tolist() == [0] and r["n_ambiguous"] == 1


def test_read_with_loci_but_none_aligned_and_read_without_loci():
    r = both(case([[(fn.SKIPPED, 0, 0), (fn.NONE, 0, 0)], [(fn.NONE, 0, 0)], [], [], [], [(0, 5, 9)]]))
    assert r["locus"].tolist() == [NO, NO, 3] and r["strand"].tolist() == [255, 255, 1]
    assert r["dist"].tolist() == [fn.NONE, fn.NONE, 0] and r["start"].tolist() == [0, 0, 5] and r["end"].tolist() == [0, 0, 9]
    assert r["second"].tolist() == [255, 255, 255] and r["best2"].tolist() == [NO, NO, NO, NO, NO, 0]
    assert (r["n_placed"], r["n_reverse"], r["n_ambiguous"]) == (1, 1, 0)


def test_no_reads():
    r = both(case([]))
    assert all(r[k].size == 0 for k in NAMES[:7]) and (r["n_placed"], r["n_reverse"], r["n_ambiguous"]) == (0, 0, 0)
