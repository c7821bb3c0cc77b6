"""tests/pair_naive.py against itself: the two statements of the pair fold agree, the hand-made cases of the contract come out as
it says, every read of a non-concordant pair is what fold_naive.fold makes of it, and engine.sam_pair_fields on a hand-made table.
No device is needed."""
import numpy as np
import pytest

from tests import fold_naive as fn
from tests import pair_naive as pn
from tests.chain_checks import same

NAMES = pn.PLACEMENTS + pn.PAIRS
NO = pn.NO_BEST
NONE16 = pn.NO_SCORE


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
    """per_strand: for every internal read (four to a pair) a list of (dist, start, end).  Returns the five arrays of the fold."""
    off = np.zeros(len(per_strand) + 1, np.uint64)
    off[1:] = np.cumsum([len(x) for x in per_strand])
    flat = [t for x in per_strand for t in x]
    dist = np.asarray([t[0] for t in flat], np.uint8)
    start = np.asarray([t[1] for t in flat], np.uint32)
    end = np.asarray([t[2] for t in flat], np.uint32)
    return off, dist, start, end, best_of(off, dist)


def same_result(got, want):
    same(NAMES, got, want)
    assert got[11] == want[11]


def both(args, lo, hi, orientation=pn.FR, penalty=pn.NO_PENALTY):
    got = pn.fold_pairs(*args, lo, hi, orientation, penalty)
    same_result(got, pn.fold_pairs_loop(*args, lo, hi, orientation, penalty))
    r = dict(zip(NAMES, got))
    r.update(got[11])
    return r


def random_case(seed):
    """pairs whose loci lie in a stretch of 400 letters, so that a good part of the (x, y) is concordant at inserts of 0 .. 300"""
    rng = np.random.default_rng(seed)
    per = []
    for r in range(4 * int(rng.integers(0, 7))):
        if r % 2 == 0:
            dead = rng.random() < 0.2                         # a mate without an aligned locus
        loci = []
        for _ in range(int(rng.integers(0, 6)) if rng.random() < 0.85 else int(rng.integers(60, 140))):
            d = int(rng.choice([fn.SKIPPED, fn.NONE] if dead else [0, 1, 1, 2, 3, fn.SKIPPED, fn.NONE]))
            s = int(rng.integers(0, 400)) if d < fn.SKIPPED else 0
            e = s + int(rng.integers(0, 60)) if d < fn.SKIPPED else 0
            loci.append((d, s, e))
        per.append(loci)
    lo = int(rng.integers(0, 120))
    penalty = int(rng.choice([0, 1, 2, 5, pn.NO_PENALTY]))
    return case(per), lo, lo + int(rng.integers(0, 300)), penalty


@pytest.mark.parametrize("orientation", [pn.FR, pn.RF, pn.FF])
@pytest.mark.parametrize("seed", range(40))
def test_fold_pairs_equals_fold_pairs_loop(seed, orientation):
    args, lo, hi, penalty = random_case(seed + 1000 * orientation)
    r = both(args, lo, hi, orientation, penalty)
    # every read of a non-concordant pair is the single-read fold's, byte for byte
    single = fn.fold(*args)
    keep = np.repeat(r["cls"] != pn.CONCORDANT, 2)
    for name, w in zip(pn.PLACEMENTS, single[:7]):
        mask = np.repeat(keep, 2) if name == "best2" else keep
        assert np.array_equal(r[name][mask], w[mask]), name
    assert r["np"] == r["n_concordant"] + r["n_discordant"] + r["n_single"] + r["n_unplaced"]


def test_random_cases_reach_every_class_and_the_long_reads():
    seen, n_long, n_amb, n_rejected = set(), 0, 0, 0
    for orientation in (pn.FR, pn.RF, pn.FF):
        for seed in range(40):
            args, lo, hi, penalty = random_case(seed + 1000 * orientation)
            r = pn.fold_pairs(*args, lo, hi, orientation, penalty)
            seen |= set(r[7].tolist())
            n_long += int((np.diff(args[0].astype(np.int64)) >= 60).sum())
            n_amb += r[11]["n_pairs_ambiguous"]
            n_rejected += r[11]["n_concordant"] != pn.fold_pairs(*args, lo, hi, orientation)[11]["n_concordant"]
    assert seen == {pn.UNPLACED, pn.CONCORDANT, pn.DISCORDANT, pn.MATE1_ONLY, pn.MATE2_ONLY}
    assert n_long >= 20 and n_amb >= 5 and n_rejected >= 3


# mate 1 forward at [1000, 1100), mate 2 reverse at [1300, 1400): T = 400
FWD_REV = [[(0, 1000, 1100)], [], [], [(0, 1300, 1400)]]


def test_insert_bounds_are_inclusive():
    args = case(FWD_REV)
    for lo, hi, cls in ((400, 400, pn.CONCORDANT), (0, 400, pn.CONCORDANT), (400, 900, pn.CONCORDANT), (0, 399, pn.DISCORDANT),
                        (401, 900, pn.DISCORDANT)):
        r = both(args, lo, hi)
        assert r["cls"].tolist() == [cls], (lo, hi)
        assert r["tlen"].tolist() == [400 if cls == pn.CONCORDANT else 0]
    r = both(args, 100, 400)                                  # T exactly max_insert; max_insert + 1 = 401 is the case above
    assert (r["score"].tolist(), r["second_score"].tolist(), r["n_concordant"], r["n_pairs_ambiguous"]) == ([0], [NONE16], 1, 0)
    assert r["locus"].tolist() == [0, 1] and r["strand"].tolist() == [0, 1] and r["best2"].tolist() == [0, NO, NO, 0]
    assert r["start"].tolist() == [1000, 1300] and r["end"].tolist() == [1100, 1400] and r["second"].tolist() == [255, 255]
    assert (r["nr"], r["n_placed"], r["n_reverse"], r["n_ambiguous"]) == (2, 2, 1, 0)


def test_dovetail_containment_and_equal_starts():
    def cls_of(u, v, lo=0, hi=1000):
        return both(case([[(0,) + u], [], [], [(0,) + v]]), lo, hi)["cls"].tolist()[0]

    assert cls_of((1000, 1100), (999, 1200)) == pn.DISCORDANT      # the downstream mate starts in front of the upstream one
    assert cls_of((1000, 1100), (1000, 1100)) == pn.CONCORDANT     # equal starts (and ends)
    assert cls_of((1000, 1100), (1000, 1099)) == pn.DISCORDANT     # ... but v may not end in front of u
    assert cls_of((1000, 1100), (1040, 1100)) == pn.CONCORDANT     # containment that ends flush
    assert cls_of((1000, 1100), (1040, 1090)) == pn.DISCORDANT     # containment that does not
    assert cls_of((1000, 1100), (1000, 1160)) == pn.CONCORDANT
    r = both(case([[(0, 1000, 1100)], [], [], [(0, 1040, 1100)]]), 0, 1000)
    assert r["tlen"].tolist() == [100]


@pytest.mark.parametrize("orientation,fits", [(pn.FR, (0, 1)), (pn.RF, (1, 0)), (pn.FF, (0, 0))])
def test_strand_combinations_of_each_orientation(orientation, fits):
    """mate 1 at [1000, 1100) and mate 2 at [1300, 1400) on every combination of strands: one fits with mate 1 upstream; with the
    places swapped its mirror image fits with mate 2 upstream"""
    for s1 in (0, 1):
        for s2 in (0, 1):
            per = [[], [], [], []]
            per[s1].append((1, 1000, 1100))
            per[2 + s2].append((2, 1300, 1400))
            r = both(case(per), 100, 600, orientation)
            ok = (s1, s2) == fits
            assert r["cls"].tolist() == [pn.CONCORDANT if ok else pn.DISCORDANT], (s1, s2)
            assert r["tlen"].tolist() == [400 if ok else 0] and r["score"].tolist() == [3]
            per = [[], [], [], []]
            per[s1].append((1, 1300, 1400))
            per[2 + s2].append((2, 1000, 1100))
            r = both(case(per), 100, 600, orientation)
            ok = (1 - s1, 1 - s2) == fits if orientation != pn.FF else (s1, s2) == (1, 1)
            assert r["cls"].tolist() == [pn.CONCORDANT if ok else pn.DISCORDANT], (s1, s2)
            assert r["tlen"].tolist() == [-400 if ok else 0]


def test_tie_break_is_score_then_x_then_y():
    # (x, y) = (0, 3) and (1, 2) both score 2, (0, 2) scores 1 but is too long, (1, 3) is a dovetail: the least x wins
    per = [[(0, 1000, 1100), (1, 5000, 5100)], [], [], [(1, 5300, 5400), (2, 1300, 1400)]]
    r = both(case(per), 100, 600)
    assert r["locus"].tolist() == [0, 3] and r["score"].tolist() == [2] and r["second_score"].tolist() == [2] and r["n_pairs_ambiguous"] == 1
    # the same x with two y at one score: the least y
    per = [[(0, 1000, 1100)], [], [], [(1, 1350, 1450), (1, 1300, 1400)]]
    r = both(case(per), 100, 600)
    assert r["locus"].tolist() == [0, 1] and r["tlen"].tolist() == [450] and r["second_score"].tolist() == [NONE16]
    # a better score beats a smaller index
    per = [[(2, 1000, 1100), (0, 5000, 5100)], [], [], [(0, 1300, 1400), (1, 5300, 5400)]]
    r = both(case(per), 100, 600)
    assert r["locus"].tolist() == [1, 3] and r["score"].tolist() == [1] and r["second_score"].tolist() == [2]
    assert r["best2"].tolist() == [1, NO, NO, 1] and r["second"].tolist() == [2, 0]


def test_unpaired_penalty_decides_between_the_pair_and_the_single_winners():
    # the concordant pair costs 1 + 2 = 3, the single winners (mate 1 at 5000, mate 2 at 9000) cost 0 + 1 = 1
    per = [[(1, 1000, 1100), (0, 5000, 5100)], [], [(1, 9000, 9100)], [(2, 1300, 1400)]]
    args = case(per)
    r = both(args, 100, 600, penalty=1)
    single = fn.fold(*args)
    assert r["cls"].tolist() == [pn.DISCORDANT] and r["tlen"].tolist() == [0] and r["score"].tolist() == [1]
    assert r["second_score"].tolist() == [NONE16] and (r["n_discordant"], r["n_concordant"]) == (1, 0)
    for name, w in zip(pn.PLACEMENTS, single[:7]):
        assert np.array_equal(r[name], w), name
    assert r["locus"].tolist() == [1, 2] and r["strand"].tolist() == [0, 0]
    r = both(args, 100, 600, penalty=2)                       # one higher: 3 <= 1 + 2
    assert r["cls"].tolist() == [pn.CONCORDANT] and r["locus"].tolist() == [0, 3] and r["score"].tolist() == [3]
    assert r["strand"].tolist() == [0, 1] and r["dist"].tolist() == [1, 2] and r["second"].tolist() == [0, 1]
    assert r["best2"].tolist() == [0, NO, NO, 0] and r["tlen"].tolist() == [400]
    assert both(args, 100, 600)["cls"].tolist() == [pn.CONCORDANT]      # the default: a concordant pair always wins
    assert both(args, 100, 600, penalty=0)["cls"].tolist() == [pn.DISCORDANT]


def test_second_score_ignores_a_shadow_of_the_winner_and_counts_a_disjoint_pair():
    shadow = [[(0, 1000, 1100), (2, 1010, 1104)], [], [], [(0, 1300, 1400), (1, 1302, 1405)]]
    r = both(case(shadow), 100, 600)
    assert r["locus"].tolist() == [0, 2] and r["second_score"].tolist() == [NONE16] and r["n_pairs_ambiguous"] == 0
    assert r["second"].tolist() == [255, 255]
    disjoint = [[(0, 1000, 1100), (2, 1100, 1200)], [], [], [(0, 1300, 1400)]]      # x' touches x: no letter shared
    r = both(case(disjoint), 100, 600)
    assert r["locus"].tolist() == [0, 2] and r["second_score"].tolist() == [2] and r["second"].tolist() == [2, 255]
    other_y = [[(0, 1000, 1100)], [], [], [(0, 1300, 1400), (3, 1400, 1500)]]       # x' == x with y' elsewhere
    r = both(case(other_y), 100, 600)
    assert r["second_score"].tolist() == [3] and r["n_pairs_ambiguous"] == 0
    # a mate-1 locus on the other strand is elsewhere, but concordant only with a partner that fits it
    strands = [[(0, 1000, 1100)], [(1, 1350, 1450)], [(1, 1020, 1120)], [(0, 1300, 1400)]]
    r = both(case(strands), 100, 600)
    assert r["locus"].tolist() == [0, 3] and r["score"].tolist() == [0] and r["second_score"].tolist() == [2]
    assert r["second"].tolist() == [1, 1]


def test_equal_runner_up_is_ambiguous():
    per = [[(1, 1000, 1100), (1, 3000, 3100)], [], [], [(0, 1300, 1400), (0, 3300, 3400)]]
    r = both(case(per), 100, 600)
    assert r["locus"].tolist() == [0, 2] and r["score"].tolist() == [1] and r["second_score"].tolist() == [1]
    assert (r["n_concordant"], r["n_pairs_ambiguous"], r["n_ambiguous"]) == (1, 1, 2)


def test_sign_of_tlen():
    r = both(case(FWD_REV), 100, 600)                         # u = mate 1
    assert r["tlen"].tolist() == [400]
    r = both(case([[], [(0, 1300, 1400)], [(0, 1000, 1100)], []]), 100, 600)        # u = mate 2
    assert r["cls"].tolist() == [pn.CONCORDANT] and r["tlen"].tolist() == [-400] and r["strand"].tolist() == [1, 0]
    assert r["best2"].tolist() == [NO, 0, 0, NO] and r["n_reverse"] == 1


def test_mates_without_an_aligned_locus_and_no_pairs():
    per = [[(2, 1000, 1100)], [], [(fn.SKIPPED, 0, 0)], [(fn.NONE, 0, 0)],          # mate 1 only
           [], [], [], [(1, 1300, 1400), (1, 1900, 2000)],                          # mate 2 only, ambiguous as a read
           [(fn.NONE, 0, 0)], [], [], [],                                           # neither
           [(0, 1000, 1100)], [], [], [(0, 1300, 1400)]]
    args = case(per)
    r = both(args, 100, 600)
    assert r["cls"].tolist() == [pn.MATE1_ONLY, pn.MATE2_ONLY, pn.UNPLACED, pn.CONCORDANT]
    assert r["score"].tolist() == [2, 1, NONE16, 0] and r["tlen"].tolist() == [0, 0, 0, 400]
    assert r["second_score"].tolist() == [NONE16] * 4
    assert r["strand"].tolist() == [0, 255, 255, 1, 255, 255, 0, 1] and r["locus"].tolist() == [0, NO, NO, 3, NO, NO, 6, 7]
    assert (r["np"], r["n_concordant"], r["n_discordant"], r["n_single"], r["n_unplaced"]) == (4, 1, 0, 2, 1)
    assert (r["nr"], r["n_placed"], r["n_reverse"], r["n_ambiguous"]) == (8, 4, 2, 1)
    single = fn.fold(*args)
    for name, w in zip(pn.PLACEMENTS, single[:7]):
        assert np.array_equal(r[name], w), name
    r = both(case([]), 0, 100)
    assert all(r[k].size == 0 for k in NAMES) and r["np"] == r["nr"] == 0
    assert best_of(np.zeros(1, np.uint64), np.zeros(0, np.uint8)).size == 0


def test_sam_pair_fields():
    from kmer_index_amd import engine

    #            concordant FR     discordant      mate 1 only     mate 2 only     unplaced        concordant, u = mate 2
    strand = [0, 1,             0, 0,           1, 255,         255, 0,         255, 255,       1, 0]
    start = [999, 1299,         49, 8999,       499, 0,         0, 19,          0, 0,           1299, 999]
    cls = [pn.CONCORDANT, pn.DISCORDANT, pn.MATE1_ONLY, pn.MATE2_ONLY, pn.UNPLACED, pn.CONCORDANT]
    tlen = [400, 0, 0, 0, 0, -400]
    flag, pos, pnext, t = engine.sam_pair_fields(np.asarray(strand, np.uint8), np.asarray(start, np.uint32), np.asarray(cls, np.uint8),
                                                 np.asarray(tlen, np.int32))
    assert flag.tolist() == [0x1 | 0x2 | 0x20 | 0x40, 0x1 | 0x2 | 0x10 | 0x80,
                             0x1 | 0x40, 0x1 | 0x80,
                             0x1 | 0x8 | 0x10 | 0x40, 0x1 | 0x4 | 0x20 | 0x80,
                             0x1 | 0x4 | 0x40, 0x1 | 0x8 | 0x80,
                             0x1 | 0x4 | 0x8 | 0x40, 0x1 | 0x4 | 0x8 | 0x80,
                             0x1 | 0x2 | 0x10 | 0x40, 0x1 | 0x2 | 0x20 | 0x80]
    assert pos.tolist() == [1000, 1300, 50, 9000, 500, 500, 20, 20, 0, 0, 1300, 1000]
    assert pnext.tolist() == [1300, 1000, 9000, 50, 500, 500, 20, 20, 0, 0, 1000, 1300]
    assert t.tolist() == [400, -400, 0, 0, 0, 0, 0, 0, 0, 0, -400, 400]
    assert flag.dtype == np.uint16 and pos.dtype == np.int64 and pnext.dtype == np.int64 and t.dtype == np.int32
    empty = engine.sam_pair_fields(np.zeros(0, np.uint8), np.zeros(0, np.uint32), np.zeros(0, np.uint8), np.zeros(0, np.int32))
    assert all(x.size == 0 for x in empty)
