"""The contract of kmx_scripts_realign (tests/realign_naive.py) on the CPU alone: its best value against an enumeration of every path
inside the band, the reads of the issue that a unit-cost script breaks into pieces, and the consequences of the contract that the GPU
tests rely on, over seeded edited reads under five scorings."""
import itertools

import numpy as np
import pytest

from kmer_index_amd import synth
from tests import align_naive as an
from tests import clip_naive as cn
from tests import realign_naive as rn
from tests import script_naive as sn
from tests.chain_checks import best_path_value
from tests.chain_data import SMALL_SCORINGS as SCORINGS, clip_text as text, edited, other

N, E = 20_000, 24
# ---- 1. the best value against every path -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(SCORINGS))
def test_the_best_value_equals_an_enumeration_of_every_path_in_the_band(name):
    opt = dict(rn.DEFAULTS, **SCORINGS[name])
    n = 0
    for m in range(5):
        for L in range(5):
            d = max(abs(m - L), 1)
            for q in itertools.product((0, 1), repeat=m):
                for t in itertools.product((0, 1), repeat=L):
                    H, _, _, _, _ = rn.tables(q, t, d, 2, **opt)
                    v, i1, j1 = rn.end_cell(H, opt["clip_penalty"])
                    assert v == best_path_value(q, t, d, 2, **opt), (q, t)
                    got = rn.align_one(q, t, d, 2, **opt)
                    assert got[0] == v and got[3:5] == (i1, j1)
                    n += 1
    assert n == 31 * 31


def test_a_letter_outside_the_alphabet_equals_nothing():
    assert rn.align_one([2, 2], [2, 2], 1, 2)[5] == [] and rn.align_one([1, 2, 1], [1, 2, 1], 1, 3)[5] == [rn.OP_EQ] * 3


# ---- 2. the reads of the issue ---------------------------------------------------------------------------------------------------------------
def located(t, q, at, **opt):
    """(script string, realigned string, the eight values of realign_one) of q at the locus `at`, through the CPU oracles of the chain"""
    d, s, e = an.align_one(t, q, at, 0, E, 4)
    runs, bad = sn.script_one(q, t[s:e], d, 4)
    assert not bad
    out = rn.realign_one(q, t[s:e], d, 4, runs, **opt)
    return cn.strings([0, len(runs)], runs)[0], cn.strings([0, len(out[0])], out[0])[0], out


def test_the_gaps_that_a_unit_cost_script_breaks_into_pieces_come_out_whole():
    t = text()
    deletion = np.concatenate([t[8000:8070], t[8082:8162]])
    script, got, out = located(t, deletion, 8000)
    assert (script, got) == ("63=1D1=3D2=3D1=3D2=1D1=1D80=", "70=12D80=") and out[1:] == (132, 0, 0, 0, 0, 12, rn.REALIGNED)
    assert cn.clip_one(cn.parse(script))[1] == 102
    insertion = np.concatenate([t[6000:6070], other(t[6070:6074]), t[6070:6146]])
    script, got, out = located(t, insertion, 6000)
    assert (script, got) == ("69=2I1=2I76=", "70=4I76=") and out[1:] == (136, 0, 0, 0, 0, 4, rn.REALIGNED)
    assert cn.clip_one(cn.parse(script))[1] == 130


def test_the_planted_ends_of_the_clip_tests_are_clipped_as_the_trimmer_clips_them():
    t = text()
    subs = t[2000:2150].copy()
    subs[[0, 2, 4]] = other(subs[[0, 2, 4]])
    _, got, out = located(t, subs, 2000)
    assert got == "5S145=" and out[1:] == (140, 5, 0, 2, 0, 0, rn.REALIGNED)
    tail = np.concatenate([t[3000:3138], other(t[3138:3150])])
    script, got, out = located(t, tail, 3000)
    assert got == "138=12S" and out[1:3] == (133, 0) and out[3] == 12 and out[7] == rn.REALIGNED
    # below the floor the script stays, with the score of the whole script; an empty script is not looked at
    low = located(t, tail, 3000, min_score=134)[2]
    assert cn.strings([0, len(low[0])], low[0])[0] == script and low[1:] == (117, 0, 0, 0, 0, 6, rn.LOW)
    assert rn.realign_one(tail, t[3000:3149], 6, 4, []) == ([], 0, 0, 0, 0, 0, 0, rn.LOW)


# ---- 3. the consequences, over seeded edited reads -------------------------------------------------------------------------------------------
def seeded_entries(n_reads=240, m=60):
    """(q, t, d, script runs) of reads of m letters with 0 .. 5 edits, and a few with a tail of other letters"""
    t = text()
    z = synth.u64_stream(4711, 24 * n_reads).astype(np.int64) & 0x7FFFFFFF
    out = []
    for p in range(n_reads):
        zz = z[24 * p:24 * p + 24]
        s = 1000 + int(zz[0] % 15_000)
        q = edited(zz[2:], t[s:s + m], int(zz[1] % 6))
        if p % 8 == 0:
            q = np.concatenate([q[:m - 9], other(t[s + m - 9:s + m])])
        d, a, b = an.align_one(t, q, s, 0, E, 4)
        runs, bad = sn.script_one(q, t[a:b], d, 4)
        assert d <= E and not bad
        out.append((q, t[a:b], d, runs))
    return out


@pytest.mark.parametrize("name", list(SCORINGS))
def test_the_consequences_of_the_contract_hold_on_edited_reads(name):
    opt = dict(rn.DEFAULTS, **SCORINGS[name])
    entries = seeded_entries()
    assert len(entries) >= 200
    seen = dict(realigned=0, clipped=0, better=0, gaps=0)
    for q, t, d, script in entries:
        runs, score, sl, sr, tl, tr, nm, cflags = rn.realign_one(q, t, d, 4, script, **opt)
        trimmed = cn.clip_one(script, **opt)
        assert score >= trimmed[1]                             # the trimmed part is one of the paths, and it lies inside the band
        seen["better"] += score > trimmed[1]
        if cflags == rn.LOW:
            assert runs == [int(v) for v in script] and (sl, sr, tl, tr) == (0, 0, 0, 0) and score == rn.whole(script, **opt)[1]
            continue
        assert cflags == rn.REALIGNED
        kept = [v for v in runs if v & 15 != rn.OP_S]
        assert kept and [v & 15 for v in runs].count(rn.OP_S) == (sl > 0) + (sr > 0)
        assert (runs[0] & 15 == rn.OP_S) == (sl > 0) and (runs[-1] & 15 == rn.OP_S) == (sr > 0)
        if sl:
            assert runs[0] >> 4 == sl and kept[0] & 15 == rn.OP_EQ
        if sr:
            assert runs[-1] >> 4 == sr and kept[-1] & 15 == rn.OP_EQ
        assert kept[0] & 15 != rn.OP_D and kept[-1] & 15 != rn.OP_D
        assert all(a & 15 != b & 15 for a, b in zip(kept[:-1], kept[1:]))                      # runs, the BAM way
        i0, i1, j0, j1 = sl, len(q) - sr, tl, len(t) - tr
        assert cn.letters_of(kept, (rn.OP_EQ, rn.OP_X, rn.OP_I)) == i1 - i0 and cn.letters_of(kept, (rn.OP_EQ, rn.OP_X, rn.OP_D)) == j1 - j0
        assert sn.replay(q[i0:i1], t[j0:j1], kept, 4) == (nm, True)
        # the score is the weight of the kept runs and the clips that were paid
        w = sum(cn.weight(v, opt["match"], opt["mismatch"], opt["gap_open"], opt["gap_extend"]) for v in kept)
        assert score == w - opt["clip_penalty"] * ((sl > 0) + (sr > 0))
        seen["realigned"] += 1
        seen["clipped"] += sl + sr > 0
        seen["gaps"] += any(v & 15 in (rn.OP_I, rn.OP_D) for v in kept)
    assert seen["realigned"] >= 200 and seen["gaps"] >= 10, seen
    if opt["mismatch"]:                                        # (where a mismatch costs nothing, no end is worth a clip)
        assert seen["clipped"] >= 10, seen
    if name == "default":
        assert seen["better"] >= 5, seen
