"""tests/realign_band.py on the CPU alone: its best value against the contract (tests/realign_naive.py) on every input of
tests/test_realign_bands_gpu.py and against the enumeration of paths (chain_checks.best_path_value), the replay of the oracle's own
runs, the conditions that the generated inputs are made for (asserted, not tuned: a generator that misses one is changed, never the
condition), and the -inf and key arithmetic of kmx_realign.hip as plain integer inequalities over the constants of the sources."""
import functools
import itertools
import os
import re

import pytest

from tests import align_naive as an
from tests import realign_band as rb
from tests import realign_naive as rn
from tests.chain_checks import best_path_value
from tests.chain_data import SMALL_SCORINGS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WIDE = (rb.DEFAULT, rb.ZERO, rb.ALL_255)                       # the scorings of the entries of the widest class: a second each in the oracle
SEEDS = range(6)
opts = lambda s, **more: dict(rn.DEFAULTS, **s, **more)


@functools.lru_cache(maxsize=None)
def gap_entries():
    return rb.located(rb.class_gaps(), an.MAX_EDITS)


@functools.lru_cache(maxsize=None)
def tie_entries():
    return {name: rb.located(b, rb.TIE_EDITS, b.sigma) for name, b in zip(rb.TIE_NAMES, rb.tie_texts())}


@functools.lru_cache(maxsize=None)
def raised_entries(max_edits, target):
    return rb.located(rb.tandem_reads(target), max_edits)


@functools.lru_cache(maxsize=None)
def fuzz_entries(seed):
    return rb.located(rb.fuzz_batch(seed), rb.FUZZ_CHAIN["max_edits"])


def check_entry(q, t, d, sigma, **opt):
    """best_v against the oracle, and the replay of the oracle's runs against its V and its four corners"""
    v, i0, j0, i1, j1, ops = rn.align_one(q, t, d, sigma, **opt)
    assert rb.best_v(q, t, d, sigma, **opt) == (v, i1, j1), (q.tolist(), t.tolist(), d, opt)
    if ops:
        runs = ([(i0 << 4) | rn.OP_S] if i0 else []) + rn.run_length(ops) + ([((len(q) - i1) << 4) | rn.OP_S] if i1 < len(q) else [])
        assert rb.replay_score(runs, q, t, j0, sigma, **opt) == (v, i1 - i0, j1 - j0), (q.tolist(), t.tolist(), d, opt)
    return v, ops


# ---- 1. the second implementation against the contract and against every path ---------------------------------------------------------------
@pytest.mark.parametrize("s", rb.SCORINGS, ids=rb.name_of)
def test_best_v_and_the_replay_equal_the_oracle_on_every_input_of_the_gpu_tests(s):
    opt = opts(s)
    n = 0
    for q, t, d, _ in gap_entries():
        if rb.class_of(d) < 3 or s in WIDE:
            check_entry(q, t, d, 4, **opt)
            n += 1
    for name, b in zip(rb.TIE_NAMES, rb.tie_texts()):
        for q, t, d, _ in tie_entries()[name]:
            check_entry(q, t, d, b.sigma, **opt)
            n += 1
    for max_edits, target in rb.RAISED:
        if rb.class_of(target) < 3 or s in WIDE:
            for q, t, d, _ in raised_entries(max_edits, target):
                check_entry(q, t, d, 4, **opt)
                n += 1
    for seed in SEEDS:
        for q, t, d, _ in fuzz_entries(seed):
            check_entry(q, t, d, 4, **opt)
            n += 1
    assert n >= 15 + 20 + 8 + 6 * 20


def test_best_v_equals_the_oracle_under_the_scoring_of_every_seeded_batch():
    for seed in range(12):
        b = rb.fuzz_batch(seed)
        for q, t, d, _ in fuzz_entries(seed):
            check_entry(q, t, d, 4, **opts(b.scoring))


@pytest.mark.parametrize("name", list(SMALL_SCORINGS))
def test_best_v_equals_an_enumeration_of_every_path_in_the_band(name):
    opt = dict(rn.DEFAULTS, **SMALL_SCORINGS[name])
    for m in range(5):
        for L in range(5):
            d = max(abs(m - L), 1)
            for q in itertools.product((0, 1), repeat=m):
                for t in itertools.product((0, 1), repeat=L):
                    assert rb.best_v(q, t, d, 2, **opt)[0] == best_path_value(q, t, d, 2, **opt), (q, t)


def test_the_replay_refuses_runs_that_lie():
    q, t = [0, 1, 2, 3, 0], [0, 1, 3, 2, 3, 0]
    good = rn.parse("1S1=1X1D2=")
    assert rb.replay_score(good, q, t, 1) == (3 - 4 - 7 - 5, 4, 5)
    assert rb.replay_score(good, q, t, 1, **rb.ALL_255) == (3 * 255 - 255 - 510 - 65535, 4, 5)
    for bad in ("1S2=1D2=", "1S1=1X1D1=1X", "1=1S1X1D2=", "1S1=1X1D3=", "1=1X1D2="):
        assert rb.replay_score(rn.parse(bad), q, t, 1) is None, bad
    assert rb.replay_score(good, q, t, 2) is None and rb.replay_score(good, q, t[:5], 1) is None


# ---- 2. what the inputs are made for ------------------------------------------------------------------------------------------------------------
def test_every_gap_read_lies_in_its_class_and_keeps_its_gap_whole_under_the_default_scoring():
    b = rb.class_gaps()
    entries = gap_entries()
    assert len(entries) == len(b.aligned) == 3 * 4 + len(rb.BOUNDARIES)
    assert [x for x in b.exact if x is not None] == list(rb.BOUNDARIES) and sorted(set(b.klass)) == [0, 1, 2, 3]
    for (q, t, d, script), kind, g, klass, exact in zip(entries, b.kind, b.g, b.klass, b.exact):
        assert rb.class_of(d) == klass and d <= 250 and (exact is None or d == exact), (d, klass, exact)
        if exact is None:
            assert d not in (31, 32, 63, 64, 127, 128)         # strictly inside
            assert g // (1 << klass) >= 8                      # the gap run crosses at least 8 lanes
        runs, score, sl, sr, tl, tr, nm, cflags = rn.realign_one(q, t, d, 4, script)
        assert cflags == rn.REALIGNED, rn.strings([0, len(runs)], runs)
        for op in kind:
            assert ((g << 4) | {"D": rn.OP_D, "I": rn.OP_I}[op]) in runs, (kind, g, rn.strings([0, len(runs)], runs))
        # the flanks of the gap are longer than what a clip in its place would save
        at = [k for k, v in enumerate(runs) if v & 15 in (rn.OP_D, rn.OP_I) and v >> 4 == g]
        for k in at:
            assert runs[k - 1] & 15 == rn.OP_EQ and runs[k + 1] & 15 == rn.OP_EQ
            assert min(runs[k - 1] >> 4, runs[k + 1] >> 4) > 6 + g + 5 or exact is not None


def ties_of(q, t, d, sigma, **opt):
    """(the cells that share the greatest V, the steps of the oracle's walk at which the diagonal and a gap state both equal H)"""
    H, E, F, s, Z = rn.tables(q, t, d, sigma, **opt)
    v, i0, j0, i1, j1, ops = rn.align_one(q, t, d, sigma, **opt)
    p = opt["clip_penalty"]
    cells = sum(H[i, j] - (p if i < len(q) else 0) == v for i in range(len(q) + 1) for j in range(len(t) + 1) if H.exists(i, j))
    i, j, steps = i0, j0, 0
    for op in ops:
        i, j = i + (op != rn.OP_D), j + (op != rn.OP_I)
        if op in (rn.OP_EQ, rn.OP_X):                          # a step that the walk took in state H, by the diagonal
            assert H[i, j] == H[i - 1, j - 1] + s(i, j)
            steps += H[i, j] in (E[i, j], F[i, j])
    assert (i, j) == (i1, j1)
    return cells, steps


@pytest.mark.parametrize("s", (rb.ZERO, rb.SCORINGS[2]), ids=rb.name_of)
def test_the_low_complexity_texts_have_tied_end_cells_and_tied_walk_steps(s):
    assert s in (rb.scoring(1, 0, 0, 0, 0), rb.scoring(1, 1, 0, 1, 0))
    for name, b in zip(rb.TIE_NAMES, rb.tie_texts()):
        entries = tie_entries()[name]
        assert len(entries) == len(b.aligned) >= 4 and all(60 <= len(q) <= 210 for q in b.aligned)
        found = [ties_of(q, t, d, b.sigma, **opts(s)) for q, t, d, _ in entries]
        assert any(cells >= 2 for cells, _ in found) and any(steps >= 1 for _, steps in found), (name, found)
    # the raised reads: the distance that puts them into the next class, exactly
    for max_edits, target in rb.RAISED:
        assert [d for _, _, d, _ in raised_entries(max_edits, target)] == [target] * 4 and rb.class_of(target) == rb.class_of(max_edits)
    assert [rb.class_of(target) for _, target in rb.RAISED] == [1, 2, 3]


def test_the_seeded_batches_hold_every_op_both_verdicts_and_a_realigned_gap():
    ops, verdicts, gaps, letters = set(), set(), 0, set()
    for seed in SEEDS:
        b = rb.fuzz_batch(seed)
        assert len(b.aligned) == 32 and all(20 <= len(q) <= 160 for q in b.aligned) and b.voters is b.aligned
        assert all((rb.revcomp(q) if i % 3 == 0 else q).tolist() == f.tolist() for i, (q, f) in enumerate(zip(b.aligned, b.forward)))
        letters |= {int(c) for q in b.aligned for c in q}
        for q, t, d, script in fuzz_entries(seed):
            runs, score, sl, sr, tl, tr, nm, cflags = rn.realign_one(q, t, d, 4, script, **opts(b.scoring, min_score=b.min_score))
            ops |= {v & 15 for v in runs}
            verdicts.add(cflags)
            gaps += cflags == rn.REALIGNED and any(v & 15 in (rn.OP_I, rn.OP_D) for v in runs)
    assert ops == {rn.OP_EQ, rn.OP_X, rn.OP_I, rn.OP_D, rn.OP_S} and verdicts == {rn.LOW, rn.REALIGNED} and gaps >= 1
    assert letters == {0, 1, 2, 3, rb.PAD}
    drawn = [rb.fuzz_batch(seed) for seed in range(12)]
    assert {b.min_score for b in drawn} == {rb.INT_MIN, 0, 40, rb.INT_MAX}
    assert {b.scoring["clip_penalty"] for b in drawn} == {0, 5, 65535} and {b.scoring["match"] for b in drawn} == {1, 2, 255}


# ---- 3. -inf and the key of the end cell, from the constants of the sources --------------------------------------------------------------------
def source(*path):
    with open(os.path.join(ROOT, *path)) as f:
        return f.read()


def constant(text, pattern):
    found = re.findall(pattern, text)
    assert len(found) == 1, pattern
    return eval(found[0], {"__builtins__": {}})                # an integer expression such as -(1 << 28)


def test_the_minus_infinity_and_the_key_bias_of_the_band_hold_at_the_bounds_of_the_header():
    hip = source("kmer_index_amd", "csrc", "kmx_realign.hip")
    neg = constant(hip, r"constexpr int kNeg = ([-()<\d ]+);")
    bias = constant(hip, r"constexpr int kKeyBias = ([-()<\d ]+);")
    core = source("kmer_index_amd", "csrc", "kmx_script_core.h")
    wave, classes = constant(core, r"constexpr uint32_t kWave = (\d+);"), constant(core, r"constexpr int kClasses = (\d+);")
    clips = source("kmer_index_amd", "csrc", "kmx_clips.h")
    top = {f: constant(clips, r"o\.%s > (\d+)\)" % f) for f in rb.FIELDS}
    header = source("include", "kmx.h")
    m_max = constant(header, r"#define KMX_ALIGN_MAX_READ +(\d+)u")
    d_max = constant(header, r"#define KMX_ALIGN_MAX_EDITS +(\d+)u")
    assert constant(clips, r"o\.match < (\d+) ") == 1
    assert (neg, bias, m_max, d_max) == (-(1 << 28), 1 << 20, an.MAX_READ, an.MAX_EDITS)
    assert top == dict(match=255, mismatch=255, gap_open=255, gap_extend=255, clip_penalty=65535)
    assert all(s[f] <= top[f] for s in rb.SCORINGS for f in rb.FIELDS) and any(all(s[f] == top[f] for f in rb.FIELDS) for s in rb.SCORINGS)
    int_min, W = -(1 << 31), 2 * d_max + 1
    slots = wave << (classes - 1)                              # the diagonal slots of a wave at NPL = 8: x < 512 in Ht + x gap_extend
    assert W <= slots - 1 and rb.class_of(d_max) == classes - 1
    for s in rb.SCORINGS + [top]:
        a, b, o, x, p = (s[f] for f in rb.FIELDS)
        # a value that a path can hold: H >= Z = -p, a gap state a whole band away from it at the most; nothing above m a
        real_lo, real_hi = -p - o - W * x, m_max * a
        # a value made from kNeg: a diagonal step from it, or the scan's Ht + x gap_extend of a slot that does not exist
        ghost_hi = neg + max(a, (slots - 1) * x)
        assert ghost_hi < real_lo, s
        assert neg + 255 * 502 < -4 * 10 ** 5 < -(top["clip_penalty"] + top["gap_open"] + W * top["gap_extend"]) <= real_lo  # the comment's own figures
        # the least sum: the scan starts from 2 kNeg and a gap of the whole row is taken off it
        assert 2 * neg - o - (slots - 1) * x >= int_min and 2 * neg - top["gap_open"] - 500 * top["gap_extend"] >= int_min, s
        # V = H - p [i < m] as the upper half of a 64-bit key; i and j as 16 bits each
        assert -2 * p + bias > 0 and real_hi + bias < 1 << 32 and real_hi <= (1 << 31) - 1, s
        assert m_max <= 0xFFFF and m_max + d_max <= 0xFFFF
