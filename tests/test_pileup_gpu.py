"""The pileup on the GPU: kmx_clips_pileup_device, kmx_clips_rescues_pileup, kmx_pileup_sites and the `pileup=` keyword of the chain
calls.  The oracle is always tests/pileup_naive.py on the host views of the engine's own handles (the scripts, the clips, the
alignments or the rescue's jobs) and on the reads as the device holds them; every plane, its dtype and every counter must be
identical, the device view must equal the host view, and the result must not depend on the path (ATOMIC, TILED) or on the tile.
tests/test_pileup_cpu.py shows on the CPU alone what hand-written entries must give.  No batch is larger than those of the chain tests
(tests/chain_data.py).  Untested: an index with several replicas, and the different-devices refusals."""
import ctypes as C

import numpy as np
import pytest

from tests import pileup_naive as pn
from tests.chain_checks import check_pileup, close_all, dev_array, doubled, pileup_want, refused, same, snapshot, untouched
from tests.chain_data import (CHAIN as PAIR_CHAIN, CLIP_CHAIN as CHAIN, CLIP_SIZES as SIZES, CLIPS, COMP4, COMPLEMENT, INSERT, K, M, N, PAIR_WORKLOADS, SCRIPTS,
                              boundary_reads, clip_planted_reads, clip_text as text, other, pairs_of, rc4, realign_batch, rescue_pairs_of, table_reads,
                              text_of)
from tests.helpers import pack

pytestmark = pytest.mark.gpu

ZERO = dict(n_added=0, n_filtered=0, n_mismatched=0, n_cells=0)
SITES = pn.SITES + ("ctg",)


def plus(a, b):
    return {k: a[k] + b[k] for k in a}


def check_sites(st, counts, lo, txt, sigma, ctg_off=None, **opt):
    want = pn.sites(counts, lo, txt, sigma, ctg_off, **opt)
    got = st.host()
    same(SITES[:6], got[:6], want[:6])
    assert (got[6] is None) == (ctg_off is None) and (ctg_off is None or (got[6].dtype == np.uint32 and np.array_equal(got[6], want[6])))
    assert st.counts() == dict(n_sites=want[0].size, n_covered=want[7])
    dv = st.device_ptrs()
    for name, p, g in zip(SITES, dv, got):
        assert bool(p) == (g is not None and g.size > 0), name
        if p:
            assert np.array_equal(dev_array(p, g.size, g.dtype), g), name
    return dict(zip(SITES, got))


@pytest.fixture(scope="module")
def index(engine):
    idx = engine.Index(text(), 4, [K], table=2)
    yield idx
    idx.close()


@pytest.fixture(scope="module")
def mapped(index):
    out = index.map_reads_strands(*pack(realign_batch()), K, COMP4, **CHAIN, scripts=True)
    yield out
    close_all(list(out))


@pytest.fixture(scope="module")
def small(index):
    t = text()
    out = index.map_reads_strands(*pack([t[9000:9150].copy(), rc4(t[9100:9250]), t[1000:1100].copy()]), K, COMP4, **CHAIN, scripts=True)
    yield out
    close_all(list(out))


# ---- 1. the batch of the realignment tests through the three sources and both paths -----------------------------------------------------
def test_scripts_trimmed_and_realigned_clips_equal_the_oracle_on_both_paths(engine, index, mapped):
    reads, loci, al, pl, sc = mapped
    ranks2, roff2 = doubled(reads)
    d_ranks2, d_roff2, nr2, stream = reads.device_ptrs()
    held = []
    try:
        trimmed = sc.clip()
        realigned = sc.realign_device(index, al, d_ranks2, d_roff2, nr2, stream=stream)
        held += [trimmed, realigned]
        before = snapshot(sc, trimmed, realigned, al)
        pu = engine.Pileup()
        held.append(pu)
        seen = []
        for cl in (None, trimmed, realigned):
            counts, ctr = pileup_want(sc, cl, al, ranks2, roff2)
            assert ctr["n_added"] == sc.counts()["n_sel"] >= 45 and ctr["n_mismatched"] == 0
            for mode in (engine.PILEUP_ATOMIC, engine.PILEUP_TILED, engine.PILEUP_AUTO):
                got = sc.pileup(index, al, reads, mode=mode, pileup=pu) if cl is None else cl.pileup(index, sc, al, reads, mode=mode, pileup=pu)
                assert got is pu
                check_pileup(pu, counts, ctr)
            seen.append(counts)
        # the gaps of the two table reads: in pieces in the scripts, whole in the realignment; the clipped ends go
        assert all(c[5, 8060:8095].any() and c[6, 6060:6080].any() for c in seen)       # DEL and INS of the two table reads
        assert int(seen[0].astype(np.int64).sum()) > int(seen[1].astype(np.int64).sum()) and not np.array_equal(seen[1], seen[2])
        untouched(before, sc, trimmed, realigned, al)
    finally:
        close_all(held)


# ---- 2. coverage and sites --------------------------------------------------------------------------------------------------------------
def test_coverage_and_the_one_site_of_a_planted_substitution(engine, index):
    t = text()
    batch, depth, count = [], 0, 0
    for i in range(60):
        s = 6950 + 5 * i
        q = t[s:s + M].copy()
        if s <= 7200 < s + M:
            depth += 1
            if i % 2:
                q[7200 - s] = other(q[7200 - s])
                count += 1
        batch.append(rc4(q) if i % 3 == 0 else q)
    assert (depth, count) == (30, 15)
    held = list(index.map_reads_strands(*pack(batch), K, COMP4, **CHAIN, scripts=True))
    try:
        reads, loci, al, pl, sc = held
        ranks2, roff2 = doubled(reads)
        counts, ctr = pileup_want(sc, None, al, ranks2, roff2)
        assert ctr["n_added"] == 60 and ctr["n_cells"] == 60 * M
        pu = sc.pileup(index, al, reads)
        held.append(pu)
        check_pileup(pu, counts, ctr)
        st = pu.sites(index, min_alt=2)
        held.append(st)
        got = check_sites(st, counts, 0, t, 4, min_alt=2)
        assert [got[k].tolist() for k in SITES[:6]] == [[7200], [int(t[7200])], [int(other(t[7200]))], [depth], [count], [depth - count]]
        assert st.counts()["n_covered"] == 59 * 5 + M
        assert pu.sites(index, min_alt=2, frac=(9, 10), sites=st) is st
        assert check_sites(st, counts, 0, t, 4, min_alt=2, frac=(9, 10))["pos"].size == 0 and st.device_ptrs() == (None,) * 7
        # every letter that is not the reference's, at any count: the substituted letter is the only one there is
        pu.sites(index, min_alt=1, frac=(0, 1), sites=st)
        assert check_sites(st, counts, 0, t, 4, min_alt=1, frac=(0, 1))["pos"].tolist() == [7200]
        # a region, and the sites of it
        counts2, ctr2 = pileup_want(sc, None, al, ranks2, roff2, 7150, 7201)
        sc.pileup(index, al, reads, lo=7150, hi=7201, pileup=pu)
        check_pileup(pu, counts2, ctr2, 7150, 7201)
        pu.sites(index, min_alt=2, sites=st)
        assert check_sites(st, counts2, 7150, t, 4, min_alt=2)["pos"].tolist() == [7200]
    finally:
        close_all(held)


# ---- 3. tile, region and lane-stride edges ----------------------------------------------------------------------------------------------
def test_tile_and_region_edges_are_identical_across_paths_and_tiles(engine, index):
    t = text()
    T = 1024                                                   # the default tile of seven channels
    starts = (T - 1, T, T + 1, 2 * T - M, 2 * T - M + 1, 3960, 4096, 4097, 6900, 6990, 8041, 8100, 8190)
    batch = [t[s:s + M].copy() for s in starts] + table_reads()[:2]
    held = list(index.map_reads_strands(*pack(batch), K, COMP4, **CHAIN, scripts=True))
    try:
        reads, loci, al, pl, sc = held
        ranks2, roff2 = doubled(reads)
        cl = sc.clip()
        held.append(cl)
        pu = engine.Pileup()
        held.append(pu)
        assert sc.counts()["n_sel"] == len(batch)
        for lo, hi in ((0, N), (4097, 8191), (7000, 7001), (15_000, 16_000), (T, 2 * T), (T + 1, 2 * T - 1)):
            counts, ctr = pileup_want(sc, cl, al, ranks2, roff2, lo, hi)
            assert ctr["n_added"] == len(batch) and (ctr["n_cells"] == 0) == (lo == 15_000)
            for mode, tile in ((engine.PILEUP_ATOMIC, 0), (engine.PILEUP_TILED, 64), (engine.PILEUP_TILED, 0), (engine.PILEUP_TILED, 4096),
                               (engine.PILEUP_AUTO, 64)):
                cl.pileup(index, sc, al, reads, lo=lo, hi=hi, mode=mode, tile=tile, pileup=pu)
                check_pileup(pu, counts, ctr, lo, hi)
    finally:
        close_all(held)


# ---- 4. the lane stride: reads of 1 .. 1024 letters; reads of letters outside the alphabet ---------------------------------------------
def test_read_lengths_around_the_wave_and_reads_of_nothing_but_insertions(engine, index):
    import torch
    voters, aligned = boundary_reads()
    ranks, roff = pack(aligned)
    held = [index.vote_windows(*pack(voters), K, 1, 8, 2, 0)]
    try:
        loci = held[0]
        al = loci.align(index, ranks, roff, 250, 64)
        sc = al.scripts(index, loci, ranks, roff)
        cl = sc.realign(index, al, ranks, roff)
        held += [al, sc, cl]
        assert sorted(np.diff(roff.astype(np.int64)).tolist())[:6] == [1, 63, 64, 65, 128, 129] and sc.counts()["n_sel"] == len(aligned)
        d_ranks, d_roff = torch.from_numpy(ranks).cuda(), torch.from_numpy(roff.view(np.int64)).cuda()
        torch.cuda.synchronize()
        pu = engine.Pileup()
        held.append(pu)
        for clips in (None, cl):
            counts, ctr = pileup_want(sc, clips, al, ranks, roff)
            assert ctr["n_added"] == len(aligned) and ctr["n_mismatched"] == 0
            for mode, tile in ((engine.PILEUP_ATOMIC, 0), (engine.PILEUP_TILED, 0), (engine.PILEUP_TILED, 64)):
                sc.pileup_device(index, al, d_ranks.data_ptr(), d_roff.data_ptr(), roff.size - 1, clips=clips, mode=mode, tile=tile, pileup=pu)
                check_pileup(pu, counts, ctr)
        # the reads blanked: every script is mI against the empty substring; ADDED, and no cell
        blank = np.full(ranks.size, 255, np.uint8)
        al2 = loci.align(index, blank, roff, 250, 64)
        sc2 = al2.scripts(index, loci, blank, roff, all=True)
        held += [al2, sc2]
        assert sc2.counts()["n_sel"] >= len(aligned) and all(s.endswith("I") and s[:-1].isdigit() for s in sc2.strings())
        d_blank = torch.from_numpy(blank).cuda()
        torch.cuda.synchronize()
        for mode in (engine.PILEUP_ATOMIC, engine.PILEUP_TILED):
            sc2.pileup_device(index, al2, d_blank.data_ptr(), d_roff.data_ptr(), roff.size - 1, mode=mode, pileup=pu)
            counts, ctr = pileup_want(sc2, None, al2, blank, roff)
            check_pileup(pu, counts, ctr)
            assert ctr == dict(ZERO, n_added=sc2.counts()["n_sel"]) and not counts.any()
    finally:
        close_all(held)


# ---- 5. accumulation ----------------------------------------------------------------------------------------------------------------------
def test_accumulation_regions_through_one_handle_and_no_entries(engine, index, mapped, small):
    reads, loci, al, pl, sc = mapped
    reads_s, _, al_s, _, sc_s = small
    big, little = doubled(reads), doubled(reads_s)
    held = []
    try:
        pu = sc.pileup(index, al, reads, add=True)             # add=True into a new handle: zeroed planes
        held.append(pu)
        c1, k1 = pileup_want(sc, None, al, *big)
        check_pileup(pu, c1, k1)
        assert sc_s.pileup(index, al_s, reads_s, add=True, mode=engine.PILEUP_TILED, pileup=pu) is pu
        c2, k2 = pileup_want(sc_s, None, al_s, *little, counts=c1)
        assert k2["n_added"] == 3 and int(c2[:, 9100:9150].sum()) - int(c1[:, 9100:9150].sum()) == 100
        check_pileup(pu, c2, plus(k1, k2))
        sc.pileup(index, al, reads, add=True, mode=engine.PILEUP_ATOMIC, pileup=pu)
        c3, k3 = pileup_want(sc, None, al, *big, counts=c2)
        check_pileup(pu, c3, plus(plus(k1, k2), k3))
        # another region with add=True: refused, and the planes and the counters stay
        assert "KMX_PILEUP_ADD" in refused(engine, lambda: sc.pileup(index, al, reads, lo=1, add=True, pileup=pu), "kmx_clips_pileup_device")
        assert "KMX_PILEUP_ADD" in refused(engine, lambda: sc.pileup(index, al, reads, hi=N - 1, add=True, pileup=pu), "kmx_clips_pileup_device")
        check_pileup(pu, c3, plus(plus(k1, k2), k3))
        # small / large / small regions through the one handle: every call without add starts afresh
        for lo, hi in ((2000, 2100), (0, N), (8000, 8003), (3000, 9000)):
            sc.pileup(index, al, reads, lo=lo, hi=hi, pileup=pu)
            check_pileup(pu, *pileup_want(sc, None, al, *big, lo, hi), lo, hi)
        # no entries: a read without a window
        nothing = list(index.map_reads_strands(*pack([np.full(M, 4, np.uint8)]), K, COMP4, **CHAIN, scripts=True))
        held += nothing
        assert nothing[4].counts()["n_sel"] == 0
        for mode in (engine.PILEUP_ATOMIC, engine.PILEUP_TILED):
            nothing[4].pileup(index, nothing[2], nothing[0], lo=10, hi=20, mode=mode, pileup=pu)
            check_pileup(pu, pn.planes(10, 20, 4), ZERO, 10, 20)
        sc.pileup(index, al, reads, lo=10, hi=20, add=True, pileup=pu)
        nothing[4].pileup(index, nothing[2], nothing[0], lo=10, hi=20, add=True, pileup=pu)
        check_pileup(pu, *pileup_want(sc, None, al, *big, 10, 20), 10, 20)
    finally:
        close_all(held)


# ---- 6. the filters -------------------------------------------------------------------------------------------------------------------------
def test_min_score_skip_low_and_min_mapq(engine, index, mapped):
    reads, loci, al, pl, sc = mapped
    ranks2, roff2 = doubled(reads)
    held = []
    try:
        cl = sc.clip(min_score=134)
        mq = pl.mapq(CHAIN["max_edits"], per_edit=2)            # 2 (25 - dist) for a read without a runner-up: below the cap, so the edits show
        pu = engine.Pileup()
        held += [cl, mq, pu]
        n_sel, n_low = sc.counts()["n_sel"], cl.counts()["n_low"]
        assert 0 < n_low < n_sel
        mapq = mq.host()
        read_sel_off = sc.host()[0].astype(np.int64)
        of_entry = mapq[np.repeat(np.arange(read_sel_off.size - 1), np.diff(read_sel_off)) >> 1]
        values = np.unique(of_entry)
        thr = int(values[values.size // 2])                    # a value that splits the entries
        assert values.size >= 2 and 0 < int((of_entry < thr).sum()) < n_sel
        score = cl.host()[0]
        cut = int(np.sort(score)[n_sel // 2])
        seen = {}
        for name, opt, with_mapq in (("low", dict(skip_low=True), False), ("score", dict(min_score=cut), False), ("mapq", dict(min_mapq=thr), True),
                                     ("all", dict(skip_low=True, min_score=cut, min_mapq=thr), True), ("none", dict(min_mapq=0, min_score=int(score.min())), True)):
            counts, ctr = pileup_want(sc, cl, al, ranks2, roff2, mapq=mapq if with_mapq else None, **opt)
            for mode in (engine.PILEUP_ATOMIC, engine.PILEUP_TILED):
                cl.pileup(index, sc, al, reads, mapq=mq if with_mapq else None, mode=mode, pileup=pu, **opt)
                check_pileup(pu, counts, ctr)
            seen[name] = ctr
        assert seen["low"]["n_filtered"] == n_low and seen["score"]["n_filtered"] == int((score < cut).sum()) > 0 and seen["none"]["n_filtered"] == 0
        assert seen["mapq"]["n_filtered"] == int((of_entry < thr).sum()) and seen["all"]["n_filtered"] >= max(seen[k]["n_filtered"] for k in ("low", "score", "mapq"))
        # the scripts alone know neither a score nor LOW; a raw device pointer serves as the MAPQ array
        counts, ctr = pileup_want(sc, None, al, ranks2, roff2, mapq=mapq, min_mapq=thr, skip_low=True, min_score=10 ** 6)
        sc.pileup(index, al, reads, mapq=mq.device_ptrs()[0], min_mapq=thr, skip_low=True, min_score=10 ** 6, pileup=pu)
        check_pileup(pu, counts, ctr)
        assert ctr["n_filtered"] == seen["mapq"]["n_filtered"]
    finally:
        close_all(held)


# ---- 7. pairs with a rescue into one handle; an alphabet of 20 letters ---------------------------------------------------------------------
def test_pairs_with_rescued_mates_go_into_one_handle(engine):
    name = "dna4_k10"
    sigma, k, n = PAIR_WORKLOADS[name]
    txt = text_of(sigma, n)
    idx = engine.Index(txt, sigma, [k], table=2)
    held = []
    try:
        ranks, roff = rescue_pairs_of(name)
        ranks, roff = ranks[:int(roff[80])], roff[:81]          # 40 pairs, 10 of them to rescue
        kw = dict(PAIR_CHAIN, **INSERT)
        out = idx.map_pairs(ranks, roff, k, COMP4, **kw, scripts=True, rescue=True, clip=dict(clip_penalty=0), pileup={})
        held += list(out)
        reads, loci, al, pl, pairs, sc, res, cl, rcl, pu = out
        held.append(rcl.scripts)
        assert isinstance(pu, engine.Pileup) and res.counts()["n_taken"] == rcl.counts()["n_sel"] == 10
        ranks2, roff2 = doubled(reads)
        c1, k1 = pileup_want(sc, cl, al, ranks2, roff2, 0, n, n)
        c2, k2 = pileup_want(rcl.scripts, rcl, res, ranks2, roff2, 0, n, n, counts=c1)
        assert k2["n_added"] == 10 and k2["n_mismatched"] == 0 and k2["n_cells"] > 0
        with pytest.raises(ValueError):
            idx.map_pairs(ranks, roff, k, COMP4, **kw, pileup={})
        check_pileup(pu, c2, plus(k1, k2), 0, n)
        # the separate calls, on the tiled path and into a region
        mine = cl.pileup(idx, sc, al, reads, lo=20_000, hi=30_001, mode=engine.PILEUP_TILED)
        held.append(mine)
        rcl.pileup(idx, rcl.scripts, res, reads, lo=20_000, hi=30_001, add=True, mode=engine.PILEUP_TILED, pileup=mine)
        check_pileup(mine, c2[:, 20_000:30_001], dict(plus(k1, k2), n_cells=int(c2[:, 20_000:30_001].sum())), 20_000, 30_001)
        # without clips the chain takes the scripts, and closes the Scripts of the rescued mates that it made for this alone
        plain = idx.map_pairs(ranks, roff, k, COMP4, **kw, scripts=True, rescue=True, pileup=dict(mode=engine.PILEUP_ATOMIC))
        held += list(plain)
        assert len(plain) == 8 and isinstance(plain[-1], engine.Pileup) and isinstance(plain[-2], engine.Rescues)
        rsc = plain[6].scripts(idx, plain[0])
        held.append(rsc)
        d1, j1 = pileup_want(plain[5], None, plain[2], ranks2, roff2, 0, n, n)
        d2, j2 = pileup_want(rsc, None, plain[6], ranks2, roff2, 0, n, n, counts=d1)
        check_pileup(plain[-1], d2, plus(j1, j2), 0, n)
        st = plain[-1].sites(idx, min_depth=2)
        held.append(st)
        check_sites(st, d2, 0, txt, sigma, min_depth=2)
    finally:
        close_all(held)
        idx.close()


def test_an_alphabet_of_twenty_letters(engine):
    name = "aa20_k5"
    sigma, k, n = PAIR_WORKLOADS[name]
    txt = text_of(sigma, n)
    idx = engine.Index(txt, sigma, [k], table=2)
    held = []
    try:
        ranks, roff = pairs_of(name)
        ranks, roff = ranks[:int(roff[80])], roff[:81]
        comp = np.asarray(COMPLEMENT[sigma], np.uint8)
        out = idx.map_pairs(ranks, roff, k, comp, **PAIR_CHAIN, **INSERT, scripts=True, pileup=dict(mode=engine.PILEUP_TILED))
        held += list(out)
        reads, loci, al, pl, pairs, sc, pu = out
        ranks2, roff2 = doubled(reads)
        counts, ctr = pileup_want(sc, None, al, ranks2, roff2, 0, n, n, sigma)
        assert counts.shape[0] == 23 and ctr["n_added"] >= 40
        check_pileup(pu, counts, ctr, 0, n, sigma)
        sc.pileup(idx, al, reads, mode=engine.PILEUP_ATOMIC, pileup=pu)
        check_pileup(pu, counts, ctr, 0, n, sigma)
        st = pu.sites(idx, frac=(1, 10))
        held.append(st)
        check_sites(st, counts, 0, txt, sigma, frac=(1, 10))
        assert st.counts()["n_covered"] > 1000
    finally:
        close_all(held)
        idx.close()


# ---- 8. a contig table ----------------------------------------------------------------------------------------------------------------------
def test_sites_carry_the_contig_under_a_contig_table(engine, index):
    t = text()
    q, r, p = t[6800:6800 + M].copy(), t[7050:7050 + M].copy(), t[12_100:12_100 + M].copy()
    q[100], r[50], p[100] = other(q[100]), other(r[50]), other(p[100])          # 6900, 7100 and 12 200: one in each contig
    batch = [q, q.copy(), rc4(q), r, rc4(r), p, p.copy(), t[6810:6810 + M].copy()]
    ctg_off = np.concatenate([[0], np.cumsum(SIZES)]).astype(np.uint64)
    idx = engine.Index(t, 4, [K], table=2)
    held = []
    try:
        idx.set_contigs(ctg_off)
        out = idx.map_reads_strands(*pack(batch), K, COMP4, **CHAIN, scripts=True, pileup=dict(lo=6000, hi=13_000))
        held += list(out)
        reads, loci, al, pl, sc, pu = out
        counts, ctr = pileup_want(sc, None, al, *doubled(reads), 6000, 13_000)
        check_pileup(pu, counts, ctr, 6000, 13_000)
        st = pu.sites(idx, min_alt=2)
        held.append(st)
        got = check_sites(st, counts, 6000, t, 4, ctg_off, min_alt=2)
        assert got["pos"].tolist() == [6900, 7100, 12_200] and got["ctg"].tolist() == [0, 1, 2] and got["count"].tolist() == [3, 2, 2]
        # the same planes under an index without a table: no ctg
        plain = pu.sites(index, min_alt=2)
        held.append(plain)
        assert check_sites(plain, counts, 6000, t, 4, None, min_alt=2)["ctg"] is None and plain.device_ptrs()[6] is None
    finally:
        close_all(held)
        idx.close()


# ---- 9. the refusals after looking, and the chain keyword -----------------------------------------------------------------------------------
def test_refusals_after_looking_and_the_state_of_the_handle(engine, index, mapped, small):
    reads, loci, al, pl, sc = mapped
    reads_s, loci_s, al_s, _, sc_s = small
    d_ranks2, d_roff2, nr2, stream = reads.device_ptrs()
    held = []
    try:
        pu = sc.pileup(index, al, reads, lo=100, hi=200)
        held.append(pu)
        empty = dict(lo=0, hi=0, n_channels=0, **ZERO)
        for call, word in ((lambda: sc.pileup(index, al, reads, lo=5, hi=5, pileup=pu), "region"), (lambda: sc.pileup(index, al, reads, hi=N + 1, pileup=pu), "region"),
                           (lambda: sc.pileup(index, al, reads, lo=N, pileup=pu), "region"),
                           (lambda: sc.pileup_device(index, al, d_ranks2, d_roff2, nr2 - 1, pileup=pu), "nr differs"),
                           (lambda: sc_s.clip().pileup(index, sc, al, reads, pileup=pu), "n_sel differs")):
            sc.pileup(index, al, reads, lo=100, hi=200, pileup=pu)
            assert word in refused(engine, call, "kmx_clips_pileup_device")
            assert pu.counts() == empty and pu.device_ptrs() == (None,) and pu.host()[0].size == 0      # the handle holds nothing
        # with add=True a refusal leaves the handle as it was
        sc.pileup(index, al, reads, lo=100, hi=200, pileup=pu)
        keep = (pu.planes(), pu.counts())
        assert "region" in refused(engine, lambda: sc.pileup(index, al, reads, lo=9, hi=9, add=True, pileup=pu), "kmx_clips_pileup_device")
        assert "nr differs" in refused(engine, lambda: sc.pileup_device(index, al, d_ranks2, d_roff2, nr2 + 2, add=True, pileup=pu), "kmx_clips_pileup_device")
        assert np.array_equal(pu.planes(), keep[0]) and pu.counts() == keep[1]
        # '=' and 'X' joined; an odd nr with a MAPQ array
        joined = al.scripts_device(index, loci, d_ranks2, d_roff2, nr2, m=True, stream=stream)
        held.append(joined)
        assert "KMX_SCRIPT_M" in refused(engine, lambda: joined.pileup(index, al, reads, pileup=pu), "kmx_clips_pileup_device")
        single = list(index.map_reads(*pack([text()[500:650].copy()]), K, **CHAIN, scripts=True))
        held += single
        assert "odd nr" in refused(engine, lambda: single[2].pileup_device(index, single[1], d_ranks2, d_roff2, 1, mapq=d_ranks2, pileup=pu), "kmx_clips_pileup_device")
        # a refusal before looking leaves the result
        sc.pileup(index, al, reads, lo=100, hi=200, pileup=pu)
        o = engine.PileupOptions(40, 0, 0, 0, 0, 0, 3, 0)
        assert engine.lib().kmx_clips_pileup_device(index._h, al._h, sc._h, None, d_ranks2, d_roff2, nr2, None, C.byref(o), None, C.byref(pu._h)) == 1
        assert pu.counts() == keep[1]
        # the sites: a pileup that holds nothing; an index with another alphabet; a shorter text
        st = pu.sites(index)
        held.append(st)
        nothing = sc.pileup(index, al, reads, lo=1, hi=2)
        held.append(nothing)
        with pytest.raises(engine.KmxError):
            sc.pileup(index, al, reads, lo=7, hi=7, pileup=nothing)
        assert "holds nothing" in refused(engine, lambda: nothing.sites(index, sites=st), "kmx_pileup_sites")
        assert st.counts() == dict(n_sites=0, n_covered=0) and st.device_ptrs() == (None,) * 7
        other_idx = engine.Index(text()[:150].copy(), 4, [K], table=2)     # the pileup's region ends behind this text
        try:
            assert "not one over this index" in refused(engine, lambda: pu.sites(other_idx, sites=st), "kmx_pileup_sites")
        finally:
            other_idx.close()
    finally:
        close_all(held)


def test_the_chain_keyword_is_the_separate_calls(engine, index):
    batch = pack(clip_planted_reads()[:6] + clip_planted_reads()[7:13])
    held = []
    try:
        for bad in (dict(pileup={}), dict(scripts=True, pileup=dict(min_mapq=1)), dict(scripts=True, pileup=dict(region=3))):
            with pytest.raises(ValueError):
                index.map_reads_strands(*batch, K, COMP4, **CHAIN, **bad)
        base = index.map_reads_strands(*batch, K, COMP4, **CHAIN, scripts=True, tags=True, letters="ACGT", clip={}, realign={})
        held += list(base)
        assert [type(h).__name__ for h in base] == ["StrandReads", "Loci", "Alignments", "Placements", "Scripts", "SamTags", "Clips"]
        got = index.map_reads_strands(*batch, K, COMP4, **CHAIN, scripts=True, tags=True, letters="ACGT", clip={}, realign={},
                                      pileup=dict(min_mapq=30, skip_low=True, min_score=100, lo=900, hi=19_000, mode=engine.PILEUP_TILED, tile=128))
        held += list(got)
        assert [type(h).__name__ for h in got] == [type(h).__name__ for h in base] + ["Pileup"]
        reads, loci, al, pl, sc, tags, cl, pu = got
        same(SCRIPTS, sc.host(), base[4].host())
        same(CLIPS, cl.host(), base[6].host())
        apart = base[6].pileup(index, base[4], base[2], base[0], lo=900, hi=19_000, mapq=base[5].mapq, min_mapq=30, skip_low=True, min_score=100)
        held.append(apart)
        assert np.array_equal(pu.planes(), apart.planes()) and pu.counts() == apart.counts()
        counts, ctr = pileup_want(sc, cl, al, *doubled(reads), 900, 19_000, mapq=tags.mapq.host(), min_mapq=30, skip_low=True, min_score=100)
        check_pileup(pu, counts, ctr, 900, 19_000)
        assert ctr["n_added"] > 0
        # into: the caller's handle is added to, and returned
        again = index.map_reads_strands(*batch, K, COMP4, **CHAIN, scripts=True, pileup=dict(into=apart, lo=900, hi=19_000))
        held += list(again[:-1])
        assert again[-1] is apart and len(again) == 6
        c2, k2 = pileup_want(again[4], None, again[2], *doubled(again[0]), 900, 19_000, counts=counts)
        check_pileup(apart, c2, plus(ctr, k2), 900, 19_000)
        # into another region: the chain raises and leaves the caller's handle open and as it was
        with pytest.raises(engine.KmxError):
            index.map_reads_strands(*batch, K, COMP4, **CHAIN, scripts=True, pileup=dict(into=apart))
        check_pileup(apart, c2, plus(ctr, k2), 900, 19_000)
    finally:
        close_all(held)
