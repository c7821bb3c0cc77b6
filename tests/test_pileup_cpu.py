"""The pileup without a device: tests/pileup_naive.py, the executable form of the contracts of kmx_clips_pileup_device /
kmx_clips_rescues_pileup and kmx_pileup_sites (include/kmx.h, KMX_PILEUP), on hand-written entries whose planes can be read off the
CIGAR, against a second implementation that expands every CIGAR to columns first, and on the identities the contract implies; then the
ABI: struct sizes, the capability macro, and the refusals that come before any handle is looked at."""
import ctypes as C
import os
import re

import numpy as np

from kmer_index_amd import synth
from tests import pileup_naive as pn
from tests.chain_data import clip_text as text, other

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N, SIGMA = 20_000, 4
OTHER, DEL, INS = SIGMA, SIGMA + 1, SIGMA + 2
OPS = {"=": pn.OP_EQ, "X": pn.OP_X, "I": pn.OP_I, "D": pn.OP_D, "S": pn.OP_S, "M": 0, "N": 3}
NEW = ("kmx_clips_pileup_device", "kmx_clips_rescues_pileup", "kmx_pileup_counts", "kmx_pileup_view", "kmx_pileup_view_device", "kmx_pileup_free",
       "kmx_pileup_sites", "kmx_sites_counts", "kmx_sites_view", "kmx_sites_view_device", "kmx_sites_free")


def parse(cigar):
    return [(OPS[op], int(ln)) for ln, op in re.findall(r"(\d+)([=XIDSMN])", cigar)]


def read_of(t, runs, s, tl=0):
    """a read that fits the runs at text position s + tl: the text under '=', another letter under 'X', letter 1 in 'I' and 'S'"""
    q, j = [], s + tl
    for op, ln in runs:
        if op == pn.OP_EQ:
            q.append(t[j:j + ln])
        elif op == pn.OP_X:
            q.append(other(t[j:j + ln]))
        elif op in (pn.OP_I, pn.OP_S):
            q.append(np.full(ln, 1, np.uint8))
        j += ln if op in (pn.OP_EQ, pn.OP_X, pn.OP_D) else 0
    return np.concatenate(q).astype(np.uint8) if q else np.zeros(0, np.uint8)


def entries(items, t=None):
    """items: (cigar string, start, tl, tr[, read]) -> (scripts, clips, start, end, ranks, roff): one read and one locus per entry, the
    clips carrying the same runs with the given tl / tr, score 100 and no flag"""
    t = text() if t is None else t
    sel, cig_off, cigar, start, end, reads, tls, trs = [], [0], [], [], [], [], [], []
    for k, item in enumerate(items):
        cig, s, tl, tr = item[:4]
        runs = parse(cig)
        span = sum(ln for op, ln in runs if op in (pn.OP_EQ, pn.OP_X, pn.OP_D))
        sel.append(k)
        cigar += [(ln << 4) | op for op, ln in runs]
        cig_off.append(len(cigar))
        start.append(s)
        end.append(s + tl + span + tr)
        tls.append(tl)
        trs.append(tr)
        reads.append(item[4] if len(item) > 4 else read_of(t, runs, s, tl))
    ne = len(items)
    roff = np.concatenate([[0], np.cumsum([len(q) for q in reads])]).astype(np.uint64)
    ranks = np.concatenate(reads).astype(np.uint8) if reads else np.zeros(0, np.uint8)
    scripts = (np.arange(ne + 1, dtype=np.uint64), np.asarray(sel, np.uint32), np.asarray(cig_off, np.uint64), np.asarray(cigar, np.uint32))
    z16 = np.zeros(ne, np.uint16)
    clips = (np.full(ne, 100, np.int32), z16, z16, np.asarray(tls, np.uint16), np.asarray(trs, np.uint16), z16, np.zeros(ne, np.uint8), scripts[2], scripts[3])
    return scripts, clips, np.asarray(start, np.uint32), np.asarray(end, np.uint32), ranks, roff


def run(items, lo=0, hi=N, with_clips=True, counts=None, **opt):
    sc, cl, start, end, ranks, roff = entries(items)
    counts = pn.planes(lo, hi, SIGMA) if counts is None else counts
    out = pn.add(counts, lo, hi, SIGMA, sc, cl if with_clips else None, start, end, ranks, roff, n=N, **opt)
    return counts, out


def letters_at(counts, a, b):
    """the letter with a count of 1 at every position of [a, b), -1 where there is none or more than one"""
    sub = counts[:SIGMA, a:b]
    return np.where(sub.sum(0) == 1, sub.argmax(0), -1)


# ---- 1. hand-written entries ----------------------------------------------------------------------------------------------------------------
def test_hand_written_entries():
    t = text()
    counts, out = run([("150=", 2000, 0, 0)])
    assert out == dict(n_added=1, n_filtered=0, n_mismatched=0, n_cells=150) and counts.sum() == 150
    assert np.array_equal(letters_at(counts, 2000, 2150), t[2000:2150]) and not counts[SIGMA:].any()

    counts, out = run([("70=12D80=", 8000, 0, 0)])
    assert out["n_cells"] == 162 and np.flatnonzero(counts[DEL]).tolist() == list(range(8070, 8082)) and counts[DEL].max() == 1
    assert np.array_equal(letters_at(counts, 8000, 8070), t[8000:8070]) and np.array_equal(letters_at(counts, 8082, 8162), t[8082:8162])
    assert not counts[:SIGMA, 8070:8082].any()

    counts, out = run([("70=4I76=", 6000, 0, 0)])
    assert out["n_cells"] == 147 and np.flatnonzero(counts[INS]).tolist() == [6069] and counts[INS, 6069] == 1
    assert np.array_equal(letters_at(counts, 6000, 6146), t[6000:6146])

    counts, out = run([("5S145=", 2000, 2, 0)])                # the text interval starts at start + tl
    assert out["n_cells"] == 145 and not counts[:, :2002].any() and np.array_equal(letters_at(counts, 2002, 2147), t[2002:2147])
    assert not counts[:, 2147:].any()

    counts, out = run([("3I140=7I", 3000, 0, 0)])              # terminal I runs are overhangs: no cell
    assert out == dict(n_added=1, n_filtered=0, n_mismatched=0, n_cells=140) and not counts[INS].any()
    counts, out = run([("2S3I140=7I1S", 3000, 0, 0)])
    assert out["n_cells"] == 140 and not counts[INS].any()

    q = t[4000:4100].copy()
    q[10] = 9                                                  # a letter >= sigma under X: the OTHER plane
    counts, out = run([("10=1X89=", 4000, 0, 0, q)])
    assert out["n_cells"] == 100 and np.flatnonzero(counts[OTHER]).tolist() == [4010] and not counts[:SIGMA, 4010].any()


def test_a_region_cuts_a_read_on_either_side():
    whole, _ = run([("70=12D30=4I46=", 8000, 0, 0)])
    for lo, hi in ((8010, 8100), (8075, 8078), (7000, 8001), (8157, 9000), (8111, 8112), (8112, 8113), (100, 200)):
        part, out = run([("70=12D30=4I46=", 8000, 0, 0)], lo, hi)
        assert np.array_equal(part, whole[:, lo:hi]) and out["n_cells"] == int(whole[:, lo:hi].sum()) and out["n_added"] == 1, (lo, hi)
    assert whole[INS, 8111] == 1 and whole[INS].sum() == 1     # (the anchor of the I run: the last letter of '30=')


def test_adding_twice_doubles_and_a_fresh_call_resets():
    items = [("70=12D80=", 8000, 0, 0), ("150=", 8050, 0, 0)]
    once, a = run(items)
    twice, b = run(items, counts=once.copy())
    assert np.array_equal(twice, 2 * once) and a == b and twice.dtype == np.uint32
    again, _ = run(items)                                      # without ADD the planes start at zero
    assert np.array_equal(again, once)
    full = np.full((SIGMA + 3, 10), pn.U32, np.uint32)         # the counters wrap
    sc, cl, start, end, ranks, roff = entries([("10=", 0, 0, 0)])
    pn.add(full, 0, 10, SIGMA, sc, None, start, end, ranks, roff, n=N)
    assert int(full.min()) == 0 and int((full == 0).sum()) == 10


def test_the_three_filters():
    items = [("150=", 2000, 0, 0), ("150=", 2100, 0, 0), ("150=", 2200, 0, 0), ("150=", 2300, 0, 0)]
    sc, cl, start, end, ranks, roff = entries(items)
    score, flags = cl[0].copy(), cl[6].copy()
    score[1], flags[2] = 50, pn.CLIP_LOW
    cl = (score,) + cl[1:6] + (flags,) + cl[7:]
    mapq = np.asarray([60, 3], np.uint8)                       # reads 0, 1 | 2, 3

    def go(clips=cl, **opt):
        counts = pn.planes(0, N, SIGMA)
        return counts, pn.add(counts, 0, N, SIGMA, sc, clips, start, end, ranks, roff, n=N, **opt)

    assert go()[1]["n_filtered"] == 0
    c, out = go(min_score=51)
    assert (out["n_added"], out["n_filtered"]) == (3, 1) and c[:, 2100:2200].sum() == 50       # (what entry 0 leaves there)
    assert go(min_score=50)[1]["n_filtered"] == 0
    c, out = go(skip_low=True)
    assert (out["n_added"], out["n_filtered"]) == (3, 1) and c[:, 2300:2350].sum() == 50
    assert go(clips=None, skip_low=True, min_score=1000)[1]["n_filtered"] == 0      # both need clips
    c, out = go(mapq=mapq, min_mapq=4)
    assert (out["n_added"], out["n_filtered"]) == (2, 2) and not c[:, 2250:].any()
    assert go(mapq=mapq, min_mapq=3)[1]["n_filtered"] == 0
    assert go(mapq=mapq, min_mapq=4, min_score=51, skip_low=True)[1] == dict(n_added=1, n_filtered=3, n_mismatched=0, n_cells=150)


def test_every_mismatched_cause_adds_nothing():
    t = text()
    good = ("100=", 5000, 0, 0)
    sc, cl, start, end, ranks, roff = entries([good])

    def verdict(sc=sc, cl=cl, start=start, end=end, ranks=ranks, roff=roff, **opt):
        counts = pn.planes(0, N, SIGMA)
        out = pn.add(counts, 0, N, SIGMA, sc, cl, start, end, ranks, roff, n=N, **opt)
        assert (out["n_mismatched"] == 1) == (not counts.any()) and out["n_added"] + out["n_mismatched"] == 1 and out["n_filtered"] == 0
        return out["n_mismatched"]

    assert verdict() == 0
    assert verdict(bound=0) == 1                                                                  # l >= bound
    assert verdict(sc=(np.asarray([0, 0], np.uint64),) + sc[1:]) == 1                             # no such r
    assert verdict(start=np.asarray([5101], np.uint32)) == 1                                      # not s <= t
    assert verdict(start=np.asarray([N - 50], np.uint32), end=np.asarray([N + 50], np.uint32)) == 1   # not t <= n
    tl = lambda a, b: cl[:3] + (np.asarray([a], np.uint16), np.asarray([b], np.uint16)) + cl[5:]
    assert verdict(cl=tl(60, 41)) == 1                                                            # tl + tr > t - s
    assert verdict(cl=tl(1, 0)) == 1                                                              # = X D lengths != t - s - tl - tr
    assert verdict(roff=np.asarray([0, 99], np.uint64)) == 1                                      # = X I S lengths != m
    for cig, bad in (("50=2M48=", 1), ("50=3N50=", 1), ("40=5S55=", 1), ("5S90=5S", 0), ("5S5S85=5S", 1), ("2I96=2D2X", 0)):
        s2 = entries([(cig, 5000, 0, 0, t[5000:5100].copy())])
        counts = pn.planes(0, N, SIGMA)
        out = pn.add(counts, 0, N, SIGMA, s2[0], s2[1], s2[2], s2[3], s2[4], s2[5], n=N)
        assert out["n_mismatched"] == bad and (not counts.any()) == bool(bad), cig
    # no runs: no counter moves at all
    none = (sc[0], sc[1], np.asarray([0, 0], np.uint64), sc[3])
    assert pn.add(pn.planes(0, N, SIGMA), 0, N, SIGMA, none, None, start, end, ranks, roff, n=N) == dict(n_added=0, n_filtered=0, n_mismatched=0, n_cells=0)


# ---- 2. a second implementation, and the identities -----------------------------------------------------------------------------------------
def random_items(seed, count):
    """seeded consistent scripts: runs of = X I D without two neighbours of one kind, S at either end now and then"""
    z = synth.u64_stream(seed, 64 * count).astype(np.int64) & 0x7FFFFFFF
    items = []
    for p in range(count):
        zz = z[64 * p:64 * p + 64]
        ops, last = [], None
        for k in range(1 + int(zz[0] % 9)):
            op = (pn.OP_EQ, pn.OP_X, pn.OP_I, pn.OP_D)[int(zz[1 + 2 * k] % 4)]
            if op == last:
                op = pn.OP_EQ if op != pn.OP_EQ else pn.OP_X
            ops.append((op, 1 + int(zz[2 + 2 * k] % 40)))
            last = op
        if zz[30] % 3 == 0:
            ops.insert(0, (pn.OP_S, 1 + int(zz[31] % 9)))
        if zz[32] % 3 == 0:
            ops.append((pn.OP_S, 1 + int(zz[33] % 9)))
        cig = "".join(f"{ln}{'=XIDS'[(pn.OP_EQ, pn.OP_X, pn.OP_I, pn.OP_D, pn.OP_S).index(op)]}" for op, ln in ops)
        items.append((cig, 1000 + int(zz[40] % 3000), int(zz[41] % 4), int(zz[42] % 4)))
    return items


def test_random_scripts_equal_the_column_expansion_and_the_identities_hold():
    t = text()
    items = random_items(7400, 200)
    for lo, hi in ((0, N), (1500, 3300)):
        sc, cl, start, end, ranks, roff = entries(items)
        counts = pn.planes(lo, hi, SIGMA)
        out = pn.add(counts, lo, hi, SIGMA, sc, cl, start, end, ranks, roff, n=N)
        assert out["n_added"] == 200 and out["n_mismatched"] == 0
        second = pn.planes(lo, hi, SIGMA)
        aligned = 0
        for k, (cig, s, tl, tr) in enumerate(items):
            runs = parse(cig)
            pn.expanded(second, lo, hi, SIGMA, runs, ranks[int(roff[k]):int(roff[k + 1])], s + tl)
            j = s + tl
            for op, ln in runs:                                # the = X letters inside the region
                if op in (pn.OP_EQ, pn.OP_X):
                    aligned += max(0, min(j + ln, hi) - max(j, lo))
                j += ln if op in (pn.OP_EQ, pn.OP_X, pn.OP_D) else 0
        assert np.array_equal(counts, second) and counts.dtype == np.uint32
        assert int(counts[:SIGMA + 1].sum()) == aligned and out["n_cells"] == int(counts.sum())
        assert counts[INS].any() and counts[DEL].any() and not counts[OTHER].any()
    assert t.size == N


# ---- 3. the sites ---------------------------------------------------------------------------------------------------------------------------
def test_sites_rules():
    t = np.asarray([0, 1, 2, 3, 0, 1, 2, 3], np.uint8)
    counts = pn.planes(0, 8, SIGMA)
    counts[:, 0] = [8, 2, 0, 0, 5, 0, 0]                       # depth 10 (OTHER 5 is not in it ... it is: channels 0 .. sigma + 1)
    counts[:, 1] = [1, 4, 0, 0, 0, 0, 0]                       # depth 5, alt A = 1: 1 * 5 >= 1 * 5 passes at equality
    counts[:, 2] = [3, 3, 4, 0, 0, 5, 6]                       # depth 15: A, C, DEL, INS pass at 1/5; G is the reference
    counts[:, 3] = [0, 0, 0, 0, 0, 0, 9]                       # depth 0: skipped although INS is 9
    counts[:, 5] = [0, 0, 0, 0, 20, 0, 0]                      # OTHER alone: covered, never a candidate
    counts[:, 6] = [1, 0, 9, 0, 0, 0, 0]
    pos, ref, alt, depth, count, ref_count, ctg, n_covered = pn.sites(counts, 0, t, SIGMA)
    assert n_covered == 5 and ctg is None
    assert list(zip(pos.tolist(), alt.tolist())) == [(1, 0), (2, 0), (2, 1), (2, DEL), (2, INS)]          # ordered by (pos, channel)
    assert depth.tolist() == [5, 15, 15, 15, 15] and count.tolist() == [1, 3, 3, 5, 6] and ref.tolist() == [1, 2, 2, 2, 2]
    assert ref_count.tolist() == [4, 4, 4, 4, 4] and [a.dtype for a in (pos, ref, alt, depth, count, ref_count)] == \
        [np.uint32, np.uint8, np.uint8, np.uint32, np.uint32, np.uint32]
    # position 0: depth 8 + 2 + 5 = 15, C = 2: 2 * 5 < 15 fails; at 2/15 it passes at equality, at 3/15 it fails again
    assert 0 not in pos.tolist()
    assert (0, 1) in list(zip(*[a.tolist() for a in pn.sites(counts, 0, t, SIGMA, frac=(2, 15))[:3:2]]))
    assert 0 not in pn.sites(counts, 0, t, SIGMA, frac=(3, 15))[0].tolist()
    # min_alt and min_depth
    assert pn.sites(counts, 0, t, SIGMA, min_alt=4)[2].tolist() == [DEL, INS]
    assert pn.sites(counts, 0, t, SIGMA, min_depth=6)[0].tolist() == [2] * 4 and pn.sites(counts, 0, t, SIGMA, min_depth=6)[7] == 4
    assert pn.sites(counts, 0, t, SIGMA, min_depth=0, min_alt=0)[0].tolist() == pos.tolist()     # 0 means 1
    # a region that starts inside the text, and a contig table
    got = pn.sites(counts[:, 1:3], 5, np.concatenate([t, t]), SIGMA, ctg_off=[0, 6, 16])
    assert got[0].tolist() == [5, 6, 6, 6, 6] and got[6].tolist() == [0, 1, 1, 1, 1] and got[1].tolist() == [1, 2, 2, 2, 2]
    assert got[2].tolist() == [0, 0, 1, DEL, INS] and got[6].dtype == np.uint32


# ---- 4. the ABI -----------------------------------------------------------------------------------------------------------------------------
def test_struct_sizes_constants_and_the_capability_macro(engine):
    assert C.sizeof(engine.PileupOptions) == 40 and C.sizeof(engine.SitesOptions) == 20
    assert (engine.PILEUP_ADD, engine.PILEUP_SKIP_LOW, engine.PILEUP_AUTO, engine.PILEUP_ATOMIC, engine.PILEUP_TILED) == (1, 2, 0, 1, 2)
    hdr = open(os.path.join(ROOT, "include", "kmx.h")).read()
    assert re.search(r"^#define KMX_PILEUP 1$", hdr, re.M) and re.search(r"^#define KMX_VERSION 5$", hdr, re.M)
    assert re.search(r"^#define KMX_PILEUP_ADD +1u", hdr, re.M) and re.search(r"^#define KMX_PILEUP_SKIP_LOW +2u", hdr, re.M)
    assert "= sizeof(kmx_pileup_options): 40 */" in hdr and "= sizeof(kmx_sites_options): 20 */" in hdr
    assert "CHANNEL-MAJOR: counts[c len + (pos - lo)]" in hdr and "THE RESULT NEVER DEPENDS ON THEM" in hdr
    for name in NEW:
        assert name in engine.EXPORTS and re.search(r"\b" + name + r"\(", hdr) and hasattr(engine.lib(), name)
    assert issubclass(engine.Pileup, engine._Handle) and issubclass(engine.Sites, engine._Handle)


def test_refusals_that_need_no_device(engine):
    L = engine.lib()
    out = C.c_void_p()
    one = C.c_void_p(1)                                        # never dereferenced: the refusal comes first
    opt = lambda **kw: engine.PileupOptions(**dict(dict(struct_size=40, flags=0, lo=0, hi=0, min_score=0, min_mapq=0, mode=0, tile=0), **kw))
    rows = ((None, out, b"options is NULL"), (opt(), None, b"inout is NULL"), (opt(struct_size=39), out, b"struct_size"), (opt(flags=4), out, b"unknown flag bits"),
            (opt(mode=3), out, b"mode"), (opt(tile=32), out, b"tile"), (opt(tile=96), out, b"tile"), (opt(tile=1), out, b"tile"))
    for o, inout, word in rows:
        by = C.byref(o) if o is not None else None
        io = C.byref(inout) if inout is not None else None
        assert L.kmx_clips_pileup_device(one, one, one, one, one, one, 2, None, by, None, io) == 1
        assert word in L.kmx_last_error() and b"kmx_clips_pileup_device: " in L.kmx_last_error(), word
        assert L.kmx_clips_rescues_pileup(one, one, one, one, one, None, by, None, io) == 1
        assert word in L.kmx_last_error() and b"kmx_clips_rescues_pileup: " in L.kmx_last_error(), word
        assert not out.value                                   # no handle was made
    ok = C.byref(opt(flags=3, mode=2, tile=64))
    for args, word in (((None, one, one, one, one, one), b"index is NULL"), ((one, None, one, one, one, one), b"alignments handle is NULL"),
                       ((one, one, None, one, one, one), b"scripts handle is NULL"), ((one, one, one, None, one, None), b"d_roff is NULL")):
        assert L.kmx_clips_pileup_device(*args, 2, None, ok, None, C.byref(out)) == 1 and word in L.kmx_last_error(), word
    for args, word in (((None, one, one, one), b"index is NULL"), ((one, None, one, one), b"reads handle is NULL"), ((one, one, None, one), b"rescues handle is NULL"),
                       ((one, one, one, None), b"scripts handle is NULL")):
        assert L.kmx_clips_rescues_pileup(*args, None, None, ok, None, C.byref(out)) == 1 and word in L.kmx_last_error(), word
    assert not out.value
    so = lambda **kw: engine.SitesOptions(**dict(dict(struct_size=20, min_depth=1, min_alt=1, frac_num=1, frac_den=5), **kw))
    for ix, pu, o, inout, word in ((one, one, None, out, b"options is NULL"), (one, one, so(), None, b"inout is NULL"), (one, one, so(struct_size=19), out, b"struct_size"),
                                   (one, one, so(frac_den=0), out, b"frac_den is 0"), (one, one, so(frac_num=6), out, b"frac_num > frac_den"),
                                   (None, one, so(), out, b"index is NULL"), (one, None, so(frac_num=5), out, b"pileup handle is NULL")):
        st = L.kmx_pileup_sites(ix, pu, C.byref(o) if o is not None else None, None, C.byref(inout) if inout is not None else None)
        assert st == 1 and word in L.kmx_last_error() and b"kmx_pileup_sites: " in L.kmx_last_error(), word
        assert not out.value
    assert L.kmx_pileup_counts(None, *[None] * 7) == 1 and b"kmx_pileup_counts" in L.kmx_last_error()
    assert L.kmx_pileup_view(None, None) == 1 and b"kmx_pileup_view" in L.kmx_last_error()
    assert L.kmx_pileup_view_device(None, None) == 1 and b"kmx_pileup_view_device" in L.kmx_last_error()
    assert L.kmx_sites_counts(None, None, None) == 1 and b"kmx_sites_counts" in L.kmx_last_error()
    assert L.kmx_sites_view(None, *[None] * 7) == 1 and L.kmx_sites_view_device(None, *[None] * 7) == 1
    L.kmx_pileup_free(None)
    L.kmx_sites_free(None)


def test_header_with_pileup_declarations_is_c99(tmp_path):
    import subprocess
    src = tmp_path / "pileup.c"
    src.write_text('#include "kmx.h"\n'
                   "#if KMX_PILEUP != 1 || KMX_VERSION != 5\n#error capability macro\n#endif\n"
                   "_Static_assert(sizeof(kmx_pileup_options) == 40, \"forty bytes\");\n"
                   "_Static_assert(sizeof(kmx_sites_options) == 20, \"five words\");\n"
                   "int use(const kmx_index* ix, const kmx_alignments* al, const kmx_scripts* sc, const kmx_clips* cl, const void* ranks, const void* roff,\n"
                   "        const kmx_strand_reads* rd, const kmx_rescues* rs, void* stream) {\n"
                   "  kmx_pileup_options o = {sizeof(kmx_pileup_options), KMX_PILEUP_ADD | KMX_PILEUP_SKIP_LOW, 0, 0, -3, 0, KMX_PILEUP_TILED, 64};\n"
                   "  kmx_sites_options so = {sizeof(kmx_sites_options), 1, 1, 1, 5};\n"
                   "  kmx_pileup* p = 0; kmx_sites* s = 0; uint64_t lo, hi, a, f, m, c, ns, nc; uint32_t ch;\n"
                   "  const uint32_t *counts, *pos, *depth, *count, *ref_count, *ctg; const uint8_t *ref, *alt;\n"
                   "  if (kmx_clips_pileup_device(ix, al, sc, cl, ranks, roff, 2, 0, &o, stream, &p) != KMX_OK) return 1;\n"
                   "  if (kmx_clips_rescues_pileup(ix, rd, rs, sc, 0, 0, &o, stream, &p) != KMX_OK) return 1;\n"
                   "  kmx_pileup_counts(p, &lo, &hi, &ch, &a, &f, &m, &c); kmx_pileup_view(p, &counts); kmx_pileup_view_device(p, &counts);\n"
                   "  kmx_pileup_sites(ix, p, &so, stream, &s); kmx_sites_counts(s, &ns, &nc);\n"
                   "  kmx_sites_view(s, &pos, &ref, &alt, &depth, &count, &ref_count, &ctg);\n"
                   "  kmx_sites_view_device(s, &pos, &ref, &alt, &depth, &count, &ref_count, &ctg);\n"
                   "  kmx_sites_free(s); kmx_pileup_free(p); return 0; }\n")
    res = subprocess.run(["gcc", "-std=c11", "-Wall", "-Wextra", "-pedantic", "-Werror", f"-I{os.path.join(ROOT, 'include')}", "-c", str(src), "-o",
                          str(tmp_path / "pileup.o")], capture_output=True, text=True)
    assert res.returncode == 0, res.stderr
