"""Secondary placements without a GPU: tests/secondary_naive.py (the contract of KMX_MAP_SECONDARIES in executable form) against its
own one-locus-at-a-time statement and against the properties the contract promises, the hand-made cases, engine.xa_strings and
engine.sam_lines(xa=...) on hand-made arrays, the ABI of the new calls and their refusals that need no device."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from tests import fold_naive as fn
from tests import secondary_naive as sn
from tests.chain_checks import same_mixed

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NO = sn.NO_BEST
NEW = ("kmx_placements_secondaries", "kmx_secondaries_counts", "kmx_secondaries_view", "kmx_secondaries_view_device", "kmx_secondaries_scripts",
       "kmx_secondaries_md", "kmx_secondaries_free")


def best_of(locus_off, dist):
    best = np.full(len(locus_off) - 1, NO, np.uint32)
    for r in range(len(locus_off) - 1):
        a, b = int(locus_off[r]), int(locus_off[r + 1])
        keys = [(int(dist[l]), l - a) for l in range(a, b) if int(dist[l]) < sn.SKIPPED]
        if keys:
            best[r] = min(keys)[1]
    return best


def case(per_strand):
    """per_strand: for every internal read a list of (dist, start, end).  Returns (locus_off, dist, start, end) and the placements of
    fold_naive.fold."""
    off = np.zeros(len(per_strand) + 1, np.uint64)
    off[1:] = np.cumsum([len(x) for x in per_strand])
    flat = [t for x in per_strand for t in x]
    dist = np.asarray([t[0] for t in flat], np.uint8)
    start = np.asarray([t[1] for t in flat], np.uint32)
    end = np.asarray([t[2] for t in flat], np.uint32)
    return (off, dist, start, end), fn.fold(off, dist, start, end, best_of(off, dist))


def random_case(seed):
    """The shape of test_strands_map_cpu.random_case: few loci mostly, sometimes more than a wave's worth; intervals inside [0, 72) so
    that many overlap and many do not, some of them empty; SKIPPED and NONE loci; reads without loci."""
    rng = np.random.default_rng(1000 + seed)
    per = []
    for _ in range(2 * int(rng.integers(0, 12))):
        loci = []
        for _ in range(int(rng.integers(0, 6)) if rng.random() < 0.8 else int(rng.integers(60, 140))):
            d = int(rng.choice([0, 1, 1, 2, 3, sn.SKIPPED, sn.NONE]))
            s = int(rng.integers(0, 60 if rng.random() < 0.7 else 600)) if d < sn.SKIPPED else 0
            e = s + int(rng.integers(0, 12)) if d < sn.SKIPPED else 0
            loci.append((d, s, e))
        per.append(loci)
    return case(per)


def elsewhere(p, q):
    return p[0] != q[0] or max(p[1], q[1]) >= min(p[2], q[2])


# ---- 1. the two statements agree, and the properties of the contract ----------------------------------------------------------------------------
@pytest.mark.parametrize("seed", range(48))
def test_secondaries_equals_secondaries_loop_and_keeps_its_promises(seed):
    (off, dist, start, end), pl = random_case(seed)
    for N, delta in ((1, None), (3, None), (32, None), (4, 0), (32, 1), (2, sn.NO_DELTA)):
        got = sn.secondaries(off, dist, start, end, pl, N, delta)
        same_mixed(sn.NAMES, got, sn.secondaries_loop(off, dist, start, end, pl, N, delta))
        sec_off, locus, sd, ss, se, more, n_sec, n_multi, n_truncated = got
        nr = (off.size - 1) // 2
        assert sec_off.size == off.size and more.size == nr and n_sec == int(sec_off[-1]) == locus.size and n_truncated == int(more.sum())
        assert n_multi == sum(int(sec_off[2 * i + 2]) > int(sec_off[2 * i]) for i in range(nr))
        for i in range(nr):
            a, b, c = (int(off[2 * i + k]) for k in range(3))
            e0, e1, e2 = (int(sec_off[2 * i + k]) for k in range(3))
            ents = [int(x) for x in locus[e0:e2]]
            if pl[1][i] == 255:
                assert not ents and more[i] == 0
                continue
            assert ents == sorted(set(ents)) and all(a <= l < c for l in ents) and int(pl[0][i]) not in ents
            assert all(l < b for l in ents[:e1 - e0]) and all(l >= b for l in ents[e1 - e0:])
            assert np.array_equal(sd[e0:e2], dist[ents]) and np.array_equal(ss[e0:e2], start[ents]) and np.array_equal(se[e0:e2], end[ents])
            places = [(int(pl[1][i]), int(pl[3][i]), int(pl[4][i]))] + [(0 if l < b else 1, int(start[l]), int(end[l])) for l in ents]
            assert all(elsewhere(p, q) for k, p in enumerate(places) for q in places[k + 1:])
            cand = [l for l in range(a, c) if dist[l] < sn.SKIPPED and l != int(pl[0][i]) and l not in ents
                    and (delta in (None, sn.NO_DELTA) or int(dist[l]) <= int(pl[2][i]) + delta)]
            free = [l for l in cand if all(elsewhere((0 if l < b else 1, int(start[l]), int(end[l])), p) for p in places)]
            if more[i] == 0:
                assert not free                                # every untaken candidate overlaps a taken place on its strand
            else:
                assert len(ents) == N and free
            if delta in (None, sn.NO_DELTA):                   # the best entry is the fold's runner-up (the first pick, for every N)
                assert (min(int(dist[l]) for l in ents) if ents else 255) == int(pl[5][i])


# ---- 2. the hand-made cases -------------------------------------------------------------------------------------------------------------------
def entries(per_strand, N, delta=None, placements=None):
    arrays, pl = case(per_strand)
    if placements is not None:
        pl = placements
    out = sn.secondaries(*arrays, pl, N, delta)
    same_mixed(sn.NAMES, out, sn.secondaries_loop(*arrays, pl, N, delta))
    return [int(x) for x in out[1]], [int(x) for x in out[5]], out


def test_a_chain_of_three_mutually_overlapping_loci_gives_one_place():
    # the primary at [100, 150); three loci around 300 that overlap one another: the best of them is the one entry
    ents, more, _ = entries([[(0, 100, 150), (2, 300, 350), (1, 310, 360), (3, 290, 345)], []], 32)
    assert ents == [2] and more == [0]


def test_a_locus_is_excluded_only_once_the_pick_it_overlaps_is_taken():
    # locus 2 overlaps locus 1 (the first pick), not the primary: with N = 1 it is what `more` reports, with N = 2 it never is an entry
    per = [[(0, 100, 150), (1, 300, 350), (2, 340, 390), (3, 500, 550)], []]
    ents, more, _ = entries(per, 1)
    assert ents == [1] and more == [1]
    ents, more, _ = entries(per, 2)
    assert ents == [1, 3] and more == [0]
    # ... and a locus that overlaps the primary is never one
    ents, more, _ = entries([[(0, 100, 150), (1, 120, 170)], []], 4)
    assert ents == [] and more == [0]


def test_ties_by_index_and_forward_before_reverse():
    # two disjoint loci of distance 1 behind the primary: N = 1 takes the lower index
    ents, more, _ = entries([[(0, 100, 150), (1, 400, 450), (1, 300, 350)], []], 1)
    assert ents == [1] and more == [1]
    # the same distance on both strands: forward first
    ents, more, _ = entries([[(0, 100, 150), (1, 300, 350)], [(1, 300, 350)]], 1)
    assert ents == [1] and more == [1]
    ents, more, out = entries([[(0, 100, 150), (1, 300, 350)], [(1, 300, 350)]], 2)
    assert ents == [1, 2] and more == [0] and out[0].tolist() == [0, 1, 2]


def test_a_twin_on_the_other_strand_at_the_same_interval_is_an_entry():
    ents, more, out = entries([[(0, 100, 140)], [(0, 100, 140)]], 32)
    assert ents == [1] and more == [0] and out[0].tolist() == [0, 0, 1] and out[6:] == (1, 1, 0)


def test_max_delta():
    per = [[(1, 100, 150), (1, 200, 250), (2, 300, 350), (3, 400, 450)], []]
    assert entries(per, 32)[0] == [1, 2, 3]
    assert entries(per, 32, 0)[0] == [1]
    assert entries(per, 32, 1)[0] == [1, 2]
    assert entries(per, 32, 2)[0] == [1, 2, 3]
    assert entries(per, 32, sn.NO_DELTA)[0] == [1, 2, 3]


def test_n_of_1_and_of_32():
    per = [[(0, 100 * k, 100 * k + 50) for k in range(40)], []]
    ents, more, out = entries(per, 1)
    assert ents == [1] and more == [1] and out[6:] == (1, 1, 1)
    ents, more, out = entries(per, 32)
    assert ents == list(range(1, 33)) and more == [1] and out[6:] == (32, 1, 1)
    ents, more, out = entries([per[0][:33], []], 32)
    assert ents == list(range(1, 33)) and more == [0]          # exactly N candidates: not truncated


def test_a_rescued_primary_excludes_no_locus_by_index():
    per = [[(1, 100, 150), (2, 300, 350)], []]
    rescued = (np.asarray([NO], np.uint32), np.asarray([1], np.uint8), np.asarray([0], np.uint8), np.asarray([100], np.uint32), np.asarray([150], np.uint32))
    ents, more, _ = entries(per, 4, placements=rescued)        # on the reverse strand: both forward loci lie elsewhere
    assert ents == [0, 1] and more == [0]
    rescued = (rescued[0], np.asarray([0], np.uint8)) + rescued[2:]
    ents, more, _ = entries(per, 4, placements=rescued)        # on the forward strand: locus 0 is the same place
    assert ents == [1]
    ents, _, _ = entries(per, 4, 1, placements=rescued)        # the delta counts from the rescued distance
    assert ents == []


def test_an_unplaced_read_and_no_reads():
    ents, more, out = entries([[(sn.NONE, 0, 0), (sn.SKIPPED, 0, 0)], [], [(0, 5, 9), (0, 50, 90)], []], 4)
    assert ents == [3] and more == [0, 0] and out[0].tolist() == [0, 0, 0, 1, 1]
    out = sn.secondaries(np.zeros(1, np.uint64), *(np.zeros(0, t) for t in (np.uint8, np.uint32, np.uint32)), tuple(np.zeros(0, np.uint32) for _ in range(5)), 4)
    assert out[0].tolist() == [0] and out[1].size == 0 and out[5].size == 0 and out[6:] == (0, 0, 0)


# ---- 3. XA -----------------------------------------------------------------------------------------------------------------------------------
def test_xa_on_hand_made_arrays_with_and_without_contigs(engine):
    sec_off = np.asarray([0, 1, 2, 2, 2, 2, 3], np.uint64)     # read 0: one entry per strand; read 1: none; read 2: one reverse entry
    dist = np.asarray([0, 2, 1], np.uint8)
    start = np.asarray([99, 1004, 2500], np.uint32)
    cigars = ["40=", "10=1X29=", ""]
    want = ["chr,+100,40=,0;chr,-1005,10=1X29=,2;", "", "chr,-2501,*,1;"]
    assert engine.xa_strings(sec_off, dist, start, None, cigars, rname="chr") == want == sn.xa(sec_off, dist, start, cigars, rname="chr")
    assert engine.xa_strings(sec_off, dist, start, None, cigars, strand_names="FR", rname="chr")[0] == "chr,F100,40=,0;chr,R1005,10=1X29=,2;"
    ctg = np.asarray([0, 1, 2], np.uint32)
    names, ctg_off = ["cA", "cB", "cC"], [0, 1000, 2000, 3000]
    want = ["cA,+100,40=,0;cB,-5,10=1X29=,2;", "", "cC,-501,*,1;"]
    assert engine.xa_strings(sec_off, dist, start, ctg, cigars, located=(names, ctg_off)) == want
    assert sn.xa(sec_off, dist, start, cigars, ctg=ctg, names=names, ctg_off=ctg_off) == want
    with pytest.raises(ValueError):
        engine.xa_strings(sec_off, dist, start, None, cigars, located=(names, ctg_off))
    with pytest.raises(ValueError):
        engine.xa_strings(sec_off, dist, start, None, cigars)
    for item in want[0].split(";")[:-1]:                       # bwa's grammar
        assert re.fullmatch(r"[^,;\s]+,[+-]\d+,([0-9]+[MIDNSHP=X])+,\d+", item)


def test_sam_lines_with_xa(engine):
    from kmer_index_amd import synth

    reads = [synth.ranks(700 + i, 8 + i, 4) for i in range(4)]
    ranks, roff = np.concatenate(reads), np.concatenate([[0], np.cumsum([r.size for r in reads])]).astype(np.uint64)
    strand = np.asarray([0, 1, 255, 0], np.uint8)
    start = np.asarray([10, 20, 0, 40], np.uint32)
    placements = (np.zeros(4, np.uint32), strand, np.asarray([0, 1, 255, 2], np.uint8), start, start + 8, np.full(4, 255, np.uint8))
    cigars = ["8=", "9=", "", "11="]
    mds = ["8", "9", "", "11"]
    mapq = np.asarray([60, 0, 0, 30], np.uint8)
    args = (["a", "b", "c", "d"], ranks, roff, "ACGT", [3, 2, 1, 0], 4, "chr", placements, cigars, mds, mapq)
    old = engine.sam_lines(*args)
    assert engine.sam_lines(*args, xa=None) == old and engine.sam_lines(*args, xa=[""] * 4) == old
    xa = ["chr,+100,8=,0;", "", "chr,-7,10=,1;", "chr,-300,11=,2;chr,+900,5=1I5=,3;"]
    new = engine.sam_lines(*args, xa=xa)
    assert new[1] == old[1]                                    # an empty string: no tag
    assert new[2] == old[2]                                    # an unplaced read carries no tags at all
    for i in (0, 3):
        assert new[i] == old[i] + "\tXA:Z:" + xa[i]
        f = new[i].split("\t")
        assert f[-2].startswith("MD:Z:") and f[-3].startswith("NM:i:") and f[-1].startswith("XA:Z:")
        assert re.fullmatch(r"XA:Z:([^,;\s]+,[+-]\d+,([0-9]+[MIDNSHP=X])+,\d+;)+", f[-1])
    with pytest.raises(ValueError):
        engine.sam_lines(*args, xa=xa[:3])


# ---- 4. the ABI ---------------------------------------------------------------------------------------------------------------------------------
def test_struct_size_constants_and_the_capability_macro(engine):
    assert C.sizeof(engine.SecondaryOptions) == 16 and engine.SECONDARY_MAX == 32 == sn.SECONDARY_MAX and engine.SECONDARY_NO_DELTA == 0xFFFFFFFF
    hdr = open(os.path.join(ROOT, "include", "kmx.h")).read()
    assert re.search(r"^#define KMX_MAP_SECONDARIES 1$", hdr, re.M) and re.search(r"^#define KMX_VERSION 5$", hdr, re.M)
    assert re.search(r"^#define KMX_SECONDARY_MAX 32$", hdr, re.M)
    assert "struct_size;    /* = sizeof(kmx_secondary_options): 16 */" in hdr
    for name in NEW:
        assert name in engine.EXPORTS and re.search(r"\b" + name + r"\(", hdr) and hasattr(engine.lib(), name)


def test_refusals_that_need_no_device(engine):
    L = engine.lib()
    out = C.c_void_p()
    opt = lambda **kw: engine.SecondaryOptions(**dict(dict(struct_size=16, max_secondary=4, max_delta=0xFFFFFFFF, flags=0), **kw))
    one = C.c_void_p(1)                                        # never dereferenced: the refusal comes first
    for lo, al, pl, o, inout, word in ((None, one, one, opt(), out, b"loci handle is NULL"), (one, None, one, opt(), out, b"alignments handle is NULL"),
                                       (one, one, None, opt(), out, b"placements handle is NULL"), (one, one, one, None, out, b"options is NULL"),
                                       (one, one, one, opt(), None, b"inout is NULL"), (one, one, one, opt(struct_size=15), out, b"struct_size"),
                                       (one, one, one, opt(flags=1), out, b"flags must be 0"), (one, one, one, opt(max_secondary=0), out, b"max_secondary"),
                                       (one, one, one, opt(max_secondary=33), out, b"max_secondary")):
        st = L.kmx_placements_secondaries(lo, al, pl, C.byref(o) if o is not None else None, None, C.byref(inout) if inout is not None else None)
        assert st == 1 and word in L.kmx_last_error() and b"kmx_placements_secondaries" in L.kmx_last_error(), word
        assert not out.value                                   # no handle was made
    assert L.kmx_secondaries_counts(None, None, None, None, None) == 1 and b"kmx_secondaries_counts" in L.kmx_last_error()
    assert L.kmx_secondaries_view(None, *[None] * 7) == 1 and b"kmx_secondaries_view" in L.kmx_last_error()
    assert L.kmx_secondaries_view_device(None, *[None] * 7) == 1 and b"kmx_secondaries_view_device" in L.kmx_last_error()
    so = engine.ScriptOptions(16, 0, 0)
    assert L.kmx_secondaries_scripts(one, None, one, C.byref(so), C.byref(out)) == 1 and b"kmx_secondaries_scripts: strand reads handle is NULL" in L.kmx_last_error()
    assert L.kmx_secondaries_scripts(one, one, None, C.byref(so), C.byref(out)) == 1 and b"kmx_secondaries_scripts: secondaries handle is NULL" in L.kmx_last_error()
    mo = engine.MdOptions(8, 0)
    letters = np.frombuffer(b"ACGT", np.uint8)
    for ix, sc, se, o, inout, word in ((one, one, one, None, out, b"options is NULL"), (one, one, one, mo, None, b"inout is NULL"),
                                       (None, one, one, mo, out, b"index is NULL"), (one, one, one, engine.MdOptions(8, 1), out, b"flags must be 0")):
        st = L.kmx_secondaries_md(ix, sc, se, letters.ctypes.data, C.byref(o) if o is not None else None, None, C.byref(inout) if inout is not None else None)
        assert st == 1 and word in L.kmx_last_error() and b"kmx_secondaries_md" in L.kmx_last_error(), word
    assert L.kmx_secondaries_md(one, one, one, None, C.byref(mo), None, C.byref(out)) == 1 and b"kmx_secondaries_md: NULL letters table" in L.kmx_last_error()
    assert not out.value
    L.kmx_secondaries_free(None)
