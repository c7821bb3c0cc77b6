"""What the tests of the mapping chain share as code: the copy of a device view, the comparison of arrays by name, the refusal of a
call, the classes that own the handles of a mapped batch, and the checkers that compare an engine handle with its naive model.
Nothing here needs a device to be imported (torch is imported where a device view is read).  pytest does not rewrite the asserts
of this module, so each carries its own message."""
import functools

import numpy as np
import pytest

from tests import chain_naive as ch
from tests import clip_naive as cn
from tests import fold_naive as fn
from tests import md_naive as mn
from tests import pair_naive as pn
from tests import pileup_naive as pun
from tests import realign_naive as rn
from tests import script_naive as sn
from tests import supp_naive as sp
from tests.chain_data import (CLIPS, COMP4, COMPLEMENT, FOLD, K, LETTERS, LETTERS4, MD, N, N_READS, PAIRS, PLACEMENTS, READ_WORKLOADS, SUPP_CHAIN, SUPP_E,
                              CHAIN, reads_of, supp_planted_reads, supp_text, text_of)
from tests.helpers import pack


# ---- arrays ---------------------------------------------------------------------------------------------------------------------------------
def dev_array(ptr, n, dtype):
    """n elements at a device pointer as a numpy copy"""
    import torch

    if n == 0 or not ptr:
        return np.zeros(0, dtype)

    class _Arr:
        def __init__(self):
            self.__cuda_array_interface__ = {"shape": (int(n) * np.dtype(dtype).itemsize,), "typestr": "|u1", "data": (int(ptr), False), "version": 2}

    out = torch.as_tensor(_Arr(), device="cuda").clone()
    torch.cuda.synchronize()
    return out.cpu().numpy().view(dtype)


def differ(name, g, w):
    """the message of two arrays that should have been equal: dtypes, shapes, the first differing index and both values there"""
    g, w = np.asarray(g), np.asarray(w)
    text = f"{name}: got {g.dtype}{g.shape}, want {w.dtype}{w.shape}"
    if g.shape == w.shape and g.size:
        bad = np.flatnonzero(g.ravel() != w.ravel())
        if bad.size:
            text += f"; {bad.size} differ, the first at {int(bad[0])}: got {g.ravel()[bad[0]]!r}, want {w.ravel()[bad[0]]!r}"
    return text


def equal(name, g, w):
    """one array against another, values only"""
    assert np.array_equal(g, w), differ(name, g, w)


def same(names, got, want):
    for name, g, w in zip(names, got, want):
        assert g.dtype == w.dtype, differ(name, g, w)
        assert np.array_equal(g, w), differ(name, g, w)


def same_mixed(names, got, want):
    """same() for results that hold counters among their arrays"""
    for name, g, w in zip(names, got, want):
        if isinstance(w, np.ndarray):
            assert g.dtype == w.dtype, differ(name, g, w)
            assert np.array_equal(g, w), differ(name, g, w)
        else:
            assert g == w, f"{name}: got {g!r}, want {w!r}"


def counts_equal(what, got, want):
    assert got == want, f"{what}: got {got!r}, want {want!r}"


# ---- calls and handles ------------------------------------------------------------------------------------------------------------------------
def refused(engine, call, fn=None, status=1):
    """the text of the KmxError that call() must raise with this status; with fn, the text names that function"""
    with pytest.raises(engine.KmxError) as e:
        call()
    text = str(e.value)
    assert e.value.status == status and (fn is None or fn + ": " in text), f"status {e.value.status} (want {status}), text {text!r} (want {fn!r} in it)"
    return text


def close_all(held):
    for h in reversed(held):
        if isinstance(h, tuple):                               # a SamTags
            close_all([x for x in h if x is not None])
        elif h is not None:
            h.close()


def snapshot(*handles):
    """what untouched() compares after a call that must only read these handles"""
    return [(h.host(), h.device_ptrs(), h.counts()) for h in handles]


def untouched(before, *handles):
    for (host, ptrs, counts), h in zip(before, handles):
        assert h.device_ptrs() == ptrs and h.counts() == counts, f"{type(h).__name__}: pointers or counts changed"
        for g, w in zip(h.host(), host):
            assert g.dtype == w.dtype and np.array_equal(g, w), differ(type(h).__name__, g, w)


def counters_of(pl, pr):
    c, k = dict(pl.counts(), n_pairs_ambiguous=pr.counts()["n_ambiguous"]), pr.counts()
    c.update({x: k[x] for x in ("np", "n_concordant", "n_discordant", "n_single", "n_unplaced")})
    return c


def entry_of(pl, sc, i):
    """the entry of public read i among the scripts of the placements"""
    strand = pl.host(best2=False)[1]
    read_sel_off = sc.host()[0]
    r = 2 * i + int(strand[i])
    assert strand[i] != 255 and read_sel_off[r + 1] > read_sel_off[r], f"read {i}: strand {strand[i]}, entries {read_sel_off[r:r + 2].tolist()}"
    return int(read_sel_off[r])


def doubled(reads):
    """(ranks2, roff2) of a StrandReads as the device holds them: the reads that the chain aligned"""
    d_ranks2, d_roff2, nr2, _ = reads.device_ptrs()
    roff2 = dev_array(d_roff2, nr2 + 1, np.uint64)
    return dev_array(d_ranks2, int(roff2[-1]), np.uint8), roff2


def spell(ranks, sigma):
    return "".join(LETTERS[sigma][int(x)] for x in ranks)


def read_of_entries(read_sel_off):
    return np.repeat(np.arange(read_sel_off.size - 1), np.diff(read_sel_off.astype(np.int64)))


class MappedPairs:
    """map_pairs of a batch with the host arrays of its loci and alignments"""

    def __init__(self, idx, sigma, ranks, roff, k, **kw):
        self.idx, self.sigma, self.ranks, self.roff = idx, sigma, ranks, roff
        self.reads, self.loci, self.al, self.pl, self.pairs = idx.map_pairs(ranks, roff, k, np.asarray(COMPLEMENT[sigma], np.uint8), **kw)
        self.h_loci, self.h_al = self.loci.host(), self.al.host()

    def close(self):
        for h in (self.pairs, self.pl, self.al, self.loci, self.reads):
            h.close()


class MappedStrands:
    """map_reads_strands of a batch with the host arrays of its loci and alignments"""

    def __init__(self, idx, sigma, ranks, roff, k, **kw):
        self.idx, self.sigma, self.ranks, self.roff = idx, sigma, ranks, roff
        self.reads, self.loci, self.al, self.pl = idx.map_reads_strands(ranks, roff, k, np.asarray(COMPLEMENT[sigma], np.uint8), **kw)
        self.h_loci, self.h_al = self.loci.host(), self.al.host()

    def close(self):
        for h in (self.pl, self.al, self.loci, self.reads):
            h.close()


class StrandWork:
    """the indexes and, per (workload, band), MappedStrands of reads_of(name, N_READS, reverse_odd=True)"""

    def __init__(self, engine):
        self.engine = engine
        self.indexes, self.mapped = {}, {}

    def index(self, name):
        if name not in self.indexes:
            sigma, k, n, _ = READ_WORKLOADS[name]
            self.indexes[name] = self.engine.Index(text_of(sigma, n), sigma, [k], table=2)
        return self.indexes[name]

    def workload(self, name, band=8):
        if (name, band) not in self.mapped:
            sigma, k, _, _ = READ_WORKLOADS[name]
            self.mapped[(name, band)] = MappedStrands(self.index(name), sigma, *reads_of(name, n_reads=N_READS, reverse_odd=True), k, **dict(CHAIN, band=band))
        return self.mapped[(name, band)]

    def close(self):
        for m in self.mapped.values():
            m.close()
        for idx in self.indexes.values():
            idx.close()


# ---- the checkers ---------------------------------------------------------------------------------------------------------------------------
def check_fold(pl, h_loci, h_al):
    """The placements against the oracle on these host loci and alignments; returns the oracle's result by name."""
    dist, start, end, best, _ = h_al
    want = fn.fold(h_loci[0], dist, start, end, best)
    same(FOLD, pl.host(), want[:7])
    c = pl.counts()
    counts_equal("the placements' counts", (c["nr"], c["n_placed"], c["n_reverse"], c["n_ambiguous"]), ((h_loci[0].size - 1) // 2,) + want[7:])
    return dict(zip(FOLD + ("n_placed", "n_reverse", "n_ambiguous"), want))


def check_pairs(pl, pr, h_loci, h_al, min_insert, max_insert, orientation=pn.FR, unpaired_penalty=pn.NO_PENALTY):
    """The placements and the pairs against the oracle on these host loci and alignments; returns the oracle's result by name."""
    dist, start, end, best, _ = h_al
    want = pn.fold_pairs(h_loci[0], dist, start, end, best, min_insert, max_insert, orientation, unpaired_penalty)
    same(PLACEMENTS, pl.host(), want[:7])
    same(PAIRS, pr.host(), want[7:11])
    c, k = dict(pl.counts(), **{"n_pairs_ambiguous": pr.counts()["n_ambiguous"]}), pr.counts()
    c.update({x: k[x] for x in ("np", "n_concordant", "n_discordant", "n_single", "n_unplaced")})
    counts_equal("the counters of the placements and the pairs", c, want[11])
    out = dict(zip(PLACEMENTS + PAIRS, want))
    out.update(want[11])
    return out


def check_md(md, sc, start, end, text, sigma, bound=None):
    """The md handle against md_naive on the host views of the scripts and these start / end arrays; returns the oracle's strings."""
    _, sel, cig_off, cigar = sc.host()
    want = mn.md(sel, cig_off, cigar, start, end, text, LETTERS[sigma], bound)
    got = md.host()
    same(MD, got, want[:2])
    counts_equal("the md counts", md.counts(), dict(n_sel=sel.size, n_bytes=want[1].size, n_mismatched=want[2]))
    d_off, d_md = md.device_ptrs()
    same(MD, (dev_array(d_off, sel.size + 1, np.uint64), dev_array(d_md, want[1].size, np.uint8)), got)
    counts_equal("the md strings", md.strings(), mn.strings(*want[:2]))
    return md.strings()


def check_rebuild(strings, sc, ranks2, roff2, start, end, text, sigma):
    """every string matches the grammar, and SEQ + CIGAR + MD give back text[start:end]"""
    read_sel_off, sel, cig_off, cigar = sc.host()
    for e, (r, l) in enumerate(zip(read_of_entries(read_sel_off), sel)):
        runs = cigar[int(cig_off[e]):int(cig_off[e + 1])]
        assert mn.GRAMMAR.match(strings[e]), f"entry {e}: the MD string {strings[e]!r} is outside the grammar"
        seq = spell(ranks2[int(roff2[r]):int(roff2[r + 1])], sigma)
        got, want = mn.rebuild(seq, runs, strings[e]), spell(text[int(start[l]):int(end[l])], sigma)
        assert got == want, f"entry {e}: SEQ + CIGAR + MD {strings[e]!r} give {got!r}, the text has {want!r}"


def check_clips(cl, sc, **opt):
    """The clips handle against clip_naive on the host views of the scripts; the device views against the host views.  Returns the
    oracle's arrays by name, with its strings and counters."""
    _, sel, cig_off, cigar = sc.host()
    want = cn.clip(cig_off, cigar, **dict(cn.DEFAULTS, **opt))
    got = cl.host()
    same(CLIPS, got, want[:9])
    counts_equal("the clips' counts", cl.counts(), dict(n_sel=sel.size, n_ops=want[8].size, n_clipped=want[9], n_low=want[10]))
    dv = cl.device_ptrs()
    sizes = (sel.size,) * 7 + (sel.size + 1, want[8].size)
    for name, p, n, g in zip(CLIPS, dv, sizes, got):
        assert (p is None) == (n == 0), f"{name}: the device pointer is {p!r} for {n} elements"
        equal(name + " (device view)", dev_array(p, n, g.dtype), g)
    counts_equal("the clips' strings", cl.strings(), cn.strings(want[7], want[8]))
    assert want[8].size <= cigar.size + 2 * sel.size, f"{want[8].size} runs beyond the bound the output is allocated at, {cigar.size} + 2 * {sel.size}"
    out = dict(zip(CLIPS, want[:9]))
    out.update(strings=cl.strings(), n_clipped=want[9], n_low=want[10], sel=sel)
    return out


def check_clip_md(md, want, start, end, txt, bound=None):
    """The md handle of clipped entries against clip_naive.md; returns the strings."""
    w = cn.md(want["sel"], want["cig_off"], want["cigar"], want["tl"], want["tr"], start, end, txt, LETTERS4, bound)
    got = md.host()
    same(MD, got, w[:2])
    counts_equal("the md counts", md.counts(), dict(n_sel=want["sel"].size, n_bytes=w[1].size, n_mismatched=w[2]))
    d_off, d_md = md.device_ptrs()
    same(MD, (dev_array(d_off, want["sel"].size + 1, np.uint64), dev_array(d_md, w[1].size, np.uint8)), got)
    return mn.strings(*w[:2])


def check_realign(cl, sc, want):
    """The clips handle against the oracle's tuple `want`; the device views against the host views.  Returns the oracle's arrays by
    name, with its strings and counters."""
    n_sel = sc.counts()["n_sel"]
    got = cl.host()
    same(CLIPS, got, want[:9])
    counts_equal("the clips' counts", cl.counts(), dict(n_sel=n_sel, n_ops=want[8].size, n_clipped=want[9], n_low=want[10]))
    sizes = (n_sel,) * 7 + (n_sel + 1, want[8].size)
    for name, p, n, g in zip(CLIPS, cl.device_ptrs(), sizes, got):
        assert (p is None) == (n == 0), f"{name}: the device pointer is {p!r} for {n} elements"
        equal(name + " (device view)", dev_array(p, n, g.dtype), g)
    counts_equal("the clips' strings", cl.strings(), rn.strings(want[7], want[8]))
    out = dict(zip(CLIPS, want[:9]))
    out.update(strings=cl.strings(), n_clipped=want[9], n_low=want[10], sel=sc.host()[1])
    return out


# ---- supplementary alignments -------------------------------------------------------------------------------------------------------------------
SUPP_SIZES = {"ent": "n_sup", "locus": "n_sup", "strand": "n_sup", "q0": "n_sup", "q1": "n_sup", "t0": "n_sup", "t1": "n_sup", "score": "n_sup",
              "second_score": "n_sup", "nm": "n_sup", "ctg": "n_sup", "more": "nr"}


def roff2_of(reads):
    _, d_roff2, nr2, _ = reads.device_ptrs()
    return dev_array(d_roff2, nr2 + 1, np.uint64) if nr2 else np.zeros(1, np.uint64)


def check_supp(sup, reads, al, pl, asc, acl, **opt):
    """The handle against supp_naive on the host views of the handles it was made from; the device views against the host views.
    Returns the oracle's dict."""
    _, start, end = al.host()[:3]
    read_sel_off, sel = asc.host()[:2]
    want = sp.supplementaries(roff2_of(reads), start, end, al.contigs_host(), pl.host(best2=False), read_sel_off, sel, acl.host(),
                              **dict(sp.DEFAULTS, **opt))
    got = sup.host()
    nr = (roff2_of(reads).size - 1) // 2
    assert len(got) == len(sp.ARRAYS) == 13, f"{len(got)} views, {len(sp.ARRAYS)} names"
    for name, g in zip(sp.ARRAYS, got):
        if want[name] is None:
            assert g is None, f"{name}: a view where the oracle has none"
        else:
            same((name,), (g,), (want[name],))
    counts_equal("the supplementaries' counts", sup.counts(), dict(nr=nr, n_sup=want["n_sup"], n_split=want["n_split"], n_truncated=want["n_truncated"]))
    c = sup.counts()
    for name, p, g in zip(sp.ARRAYS, sup.device_ptrs(), got):
        n = c["nr"] + 1 if name == "sup_off" else c[SUPP_SIZES[name]]
        if name == "ctg" and g is None:
            assert p is None, "ctg: a device pointer without a host view"
            continue
        assert (p is None) == (n == 0), f"{name}: the device pointer is {p!r} for {n} elements"
        equal(name + " (device view)", dev_array(p, n, g.dtype), g)
    return want


@functools.lru_cache(maxsize=None)
def supp_cpu_chain():
    """The planted batch of the supplementary tests through front, vote, align, fold, the scripts of every aligned locus and their
    clips: the host arrays that supp_naive takes, by name."""
    t = supp_text()
    ranks, roff = pack(supp_planted_reads())
    reads, loci, al = ch._front(t, 4, ranks, roff, K, COMP4, 1, SUPP_CHAIN["band"], SUPP_CHAIN["min_votes"], 0, SUPP_E, SUPP_CHAIN["max_span"])
    dist, start, end, best, _ = al.arrays
    f = fn.fold(loci.arrays[0], dist, start, end, best)
    read_sel_off, sel, cig_off, cigar, bad = sn.scripts(t, *reads.arrays, loci.arrays[0], dist, start, end, best, 4, True, False)
    assert bad == 0, f"{bad} scripts of the planted batch do not replay"
    clips = cn.clip(cig_off, cigar, **cn.DEFAULTS)
    return dict(roff2=reads.arrays[1], locus_off=loci.arrays[0], dist=dist, start=start, end=end, placements=f[:7], read_sel_off=read_sel_off, sel=sel,
                clips=clips[:9], strings=cn.strings(clips[7], clips[8]))


def supp_oracle(c, ctg=None, **opt):
    return sp.supplementaries(c["roff2"], c["start"], c["end"], ctg, c["placements"], c["read_sel_off"], c["sel"], c["clips"], **opt)


def supp_rows(out, i=0):
    """(ent, strand, q0, q1, t0, t1, score, second_score) of the entries of read i"""
    a, b = int(out["sup_off"][i]), int(out["sup_off"][i + 1])
    return [tuple(int(out[k][x]) for k in ("ent", "strand", "q0", "q1", "t0", "t1", "score", "second_score")) for x in range(a, b)]


# ---- the pileup -------------------------------------------------------------------------------------------------------------------------------
def pileup_want(sc, cl, source, ranks2, roff2, lo=0, hi=N, n=N, sigma=4, counts=None, mapq=None, **opt):
    """(planes, counters) of the oracle for the entries of `sc` (cl: their Clips or None) over the start / end of `source`, an
    Alignments or a Rescues; counts: planes to add to"""
    h = source.host()
    start, end = (h[1], h[2]) if type(source).__name__ == "Alignments" else (h[5], h[6])
    counts = pun.planes(lo, hi, sigma) if counts is None else counts.copy()
    out = pun.add(counts, lo, hi, sigma, sc.host(), None if cl is None else cl.host(), start, end, ranks2, roff2, mapq, n=n, **opt)
    return counts, out


def check_pileup(pu, counts, ctr, lo=0, hi=N, sigma=4):
    """the handle against the oracle's planes and counters; the device view against the host view"""
    got = pu.planes()
    assert got.dtype == np.uint32 and got.shape == (sigma + 3, hi - lo) and np.array_equal(got, counts), differ("planes", got, counts)
    counts_equal("the pileup's counts", pu.counts(), dict(lo=lo, hi=hi, n_channels=sigma + 3, **ctr))
    (d_counts,) = pu.device_ptrs()
    assert d_counts, "the pileup has no device pointer"
    equal("planes (device view)", dev_array(d_counts, got.size, np.uint32), got.ravel())
    total = int(counts.astype(np.int64).sum())
    assert ctr["n_cells"] == total or ctr["n_cells"] >= 2 ** 32, f"n_cells is {ctr['n_cells']}, the planes sum to {total}"


# ---- the realignment ----------------------------------------------------------------------------------------------------------------------------
def best_path_value(q, t, d, sigma, match, mismatch, gap_open, gap_extend, clip_penalty, **_):
    """The greatest value of any path inside the band, by walking every path: a recursion over the paths, no table.  A path starts at
    any cell that exists (a start at i > 0 pays p), takes '=' / 'X', I and D steps through cells that exist (a gap run of len letters
    costs o + len x, so a step that goes on in the direction of the last one pays x alone) and ends anywhere (an end at i < m pays p)."""
    m, L = len(q), len(t)
    exists = lambda i, j: 0 <= i <= m and 0 <= j <= L and abs(j - i) <= d

    def onwards(i, j, last):
        best = -clip_penalty if i < m else 0                   # ending here
        if exists(i + 1, j + 1):
            s = match if q[i] == t[j] and q[i] < sigma else -mismatch
            best = max(best, s + onwards(i + 1, j + 1, "M"))
        if exists(i + 1, j):
            best = max(best, -gap_extend - (0 if last == "I" else gap_open) + onwards(i + 1, j, "I"))
        if exists(i, j + 1):
            best = max(best, -gap_extend - (0 if last == "D" else gap_open) + onwards(i, j + 1, "D"))
        return best

    return max((0 if i == 0 else -clip_penalty) + onwards(i, j, None) for i in range(m + 1) for j in range(L + 1) if exists(i, j))
