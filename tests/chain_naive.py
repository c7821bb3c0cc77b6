"""The whole mapping chain on the CPU, from the text and the reads alone: glue over the naives of the single stages, no alignment
code of its own.  In order: fold_naive.double_reads, front_naive.hits, vote_naive.vote, align_naive.align, fold_naive.fold or
pair_naive.fold_pairs, rescue_naive.rescue, script_naive.scripts, md_naive.md / clip_naive.md, mapq_naive.mapq,
secondary_naive.secondaries and clip_naive.clip.

strands() and pairs() return what Index.map_reads_strands(scripts=True, tags=True, ...) and Index.map_pairs(rescue=True, tags=True)
return, in host form: a tuple with one Stage per handle, in the order of the handles, the SamTags as a Tags of four Stages (None
where the engine has None).  Stage.arrays are the arrays of the handle's host() (of the device views for the reads, which have no
host view), array for array and dtype for dtype; Stage.totals are those of the handle's counts() that the naives define.

tile(result, R) is the result of the batch made of R copies of the base batch back to back (tile_reads), built from the base
batch's result alone: arrays with an entry per read, locus, job, entry or letter are repeated, offset arrays are continued, indexes
into the loci, the internal reads and the jobs are moved on by their number per copy, and every total is multiplied.  Every stage of
the chain looks at one read or one pair at a time and no statistic of the batch enters any result, which is why this holds;
tests/test_front_cpu.py checks it against the chain on the tiled batch itself."""
import collections

import numpy as np

from tests import align_naive as an
from tests import clip_naive as cn
from tests import fold_naive as fn
from tests import front_naive as frn
from tests import mapq_naive as mqn
from tests import md_naive as mn
from tests import pair_naive as pn
from tests import rescue_naive as rn
from tests import script_naive as sn
from tests import secondary_naive as secn
from tests import vote_naive as vn

NO = fn.NO_BEST
NO_SPAN = 0xFFFFFFFF
Stage = collections.namedtuple("Stage", "kind arrays totals")
Tags = collections.namedtuple("Tags", "mapq md rescue_scripts rescue_md")

# per kind, per array: "per" = one entry per something, repeated as it is; "off" = an offset array; "loci" / "reads" / "jobs" = one
# entry per something that is an index into the loci / the internal reads / the jobs of the batch (0xFFFFFFFF: none); None = no array
SPEC = {
    "reads": ("per", "off"),
    "loci": ("off", "per", "per", "per", "per"),
    "alignments": ("per",) * 5,                                # (best is an index within the read's loci)
    "placements": ("loci",) + ("per",) * 6,                    # (so is best2)
    "pairs": ("per",) * 4,
    "scripts": ("off", "loci", "off", "per"),
    "rescues": ("off", "reads") + ("per",) * 6,
    "rescue_scripts": ("off", "jobs", "off", "per"),
    "mapq": ("per",),
    "md": ("off", "per"),
    "secondaries": ("off", "loci", "per", "per", "per", None, "per"),
    "clips": ("per",) * 7 + ("off", "per"),
}


def tile_reads(ranks, roff, R):
    """(ranks, roff) of R copies of a batch back to back"""
    roff = np.asarray(roff, np.uint64)
    return np.tile(np.asarray(ranks, np.uint8), R), _tile_off(roff, R)


def _tile_off(a, R):
    total = a[-1]
    return np.concatenate([a[:-1] + a.dtype.type(r) * total for r in range(R)] + [np.asarray([a.dtype.type(R) * total], a.dtype)]).astype(a.dtype)


def _tile_index(a, R, per_copy):
    moved = np.tile(a.astype(np.int64), R) + np.repeat(np.arange(R, dtype=np.int64) * per_copy, a.size)
    return np.where(np.tile(a, R) == NO, NO, moved).astype(a.dtype)


def tile(result, R):
    flat = [s for x in result for s in (x if isinstance(x, Tags) else (x,)) if s is not None]
    by_kind = {s.kind: s for s in flat}
    per_copy = {"loci": by_kind["loci"].arrays[1].size, "reads": by_kind["reads"].arrays[1].size - 1,
                "jobs": by_kind["rescues"].arrays[1].size if "rescues" in by_kind else 0}

    def one(s):
        if s is None:
            return None
        arrays = []
        for a, how in zip(s.arrays, SPEC[s.kind]):
            arrays.append(None if how is None else np.tile(a, R) if how == "per" else _tile_off(a, R) if how == "off" else _tile_index(a, R, per_copy[how]))
        return Stage(s.kind, tuple(arrays), {k: v * R for k, v in s.totals.items()})

    return tuple(Tags(*[one(s) for s in x]) if isinstance(x, Tags) else one(x) for x in result)


# ---- the stages ----------------------------------------------------------------------------------------------------------------------------
def _front(text, sigma, ranks, roff, w, complement, stride, band, min_votes, max_occ, max_edits, max_span):
    """the doubled batch, its loci and its alignments: (Stage reads, Stage loci, Stage alignments)"""
    text = np.asarray(text, np.uint8)
    ranks2, roff2 = fn.double_reads(ranks, roff, complement, sigma)
    win_off, hit_off, positions, _ = frn.hits(text, sigma, ranks2, roff2, w, stride)
    locus_off, diag, span, votes, skipped, n_votes = vn.vote(hit_off, positions, win_off, stride, band, min_votes, max_occ)
    al = an.align(text, ranks2, roff2, locus_off, diag, span, max_edits, NO_SPAN if max_span is None else max_span, sigma)
    nr2 = roff2.size - 1
    return (Stage("reads", (ranks2, roff2), {}),
            Stage("loci", (locus_off, diag, span, votes, skipped), dict(nr=nr2, n_loci=int(diag.size), n_votes=int(n_votes))),
            Stage("alignments", tuple(al), dict(nr=nr2, n_loci=int(diag.size), n_aligned=int(al[4].sum()), n_skipped=int((al[0] == an.SKIPPED).sum()))))


def _scripts(kind, text, sigma, reads, off, dist, start, end, best):
    got = sn.scripts(text, *reads.arrays, off, dist, start, end, best, sigma, False, False)
    return Stage(kind, tuple(got[:4]), dict(nr=reads.arrays[1].size - 1, n_sel=int(got[1].size), n_ops=int(got[3].size), n_mismatched=int(got[4])))


def _md(sel, cig_off, cigar, start, end, text, letters, bound=None, clips=None):
    if clips is None:
        got = mn.md(sel, cig_off, cigar, start, end, text, letters, bound)
    else:
        c = clips.arrays
        got = cn.md(sel, c[7], c[8], c[3], c[4], start, end, text, letters, bound)
    return Stage("md", tuple(got[:2]), dict(n_sel=int(len(sel)), n_bytes=int(got[1].size), n_mismatched=int(got[2])))


def _clips(scripts, options):
    got = cn.clip(scripts.arrays[2], scripts.arrays[3], **dict(cn.DEFAULTS, **options))
    return Stage("clips", tuple(got[:9]), dict(n_sel=int(scripts.arrays[1].size), n_ops=int(got[8].size), n_clipped=int(got[9]), n_low=int(got[10])))


def _mapq(pl, max_edits, pairs=None):
    kw = {} if pairs is None else dict(cls=pairs[0], score=pairs[2], second_score=pairs[3])
    mapq, counts = mqn.mapq(pl[1], pl[2], pl[5], max_edits, **kw)
    return Stage("mapq", (mapq,), counts)


def strands(text, sigma, ranks, roff, w, complement, letters, stride=1, band=0, min_votes=1, max_occ=0, max_edits=0, max_span=None,
            secondaries=0, clip=None):
    """Index.map_reads_strands(..., scripts=True, tags=True, letters=letters, secondaries=secondaries, clip=clip):
    (reads, loci, alignments, placements, scripts, Tags(mapq, md, None, None)[, secondaries][, clips])"""
    reads, loci, al = _front(text, sigma, ranks, roff, w, complement, stride, band, min_votes, max_occ, max_edits, max_span)
    dist, start, end, best, _ = al.arrays
    f = fn.fold(loci.arrays[0], dist, start, end, best)
    pl = Stage("placements", tuple(f[:7]), dict(nr=int(f[1].size), n_placed=f[7], n_reverse=f[8], n_ambiguous=f[9]))
    sc = _scripts("scripts", text, sigma, reads, loci.arrays[0], dist, start, end, f[6])
    cl = None if clip is None else _clips(sc, clip)
    md = _md(sc.arrays[1], sc.arrays[2], sc.arrays[3], start, end, text, letters, clips=cl)
    out = (reads, loci, al, pl, sc, Tags(_mapq(f, max_edits), md, None, None))
    if secondaries:
        s = secn.secondaries(loci.arrays[0], dist, start, end, f[:7], secondaries)
        out += (Stage("secondaries", tuple(s[:5]) + (None, s[5]), dict(nr=int(f[1].size), n_sec=s[6], n_multi=s[7], n_truncated=s[8])),)
    return out if cl is None else out + (cl,)


def pairs(text, sigma, ranks, roff, w, complement, letters, min_insert, max_insert, orientation=pn.FR, stride=1, band=0, min_votes=1, max_occ=0,
          max_edits=0, max_span=None):
    """Index.map_pairs(..., rescue=True, tags=True, letters=letters):
    (reads, loci, alignments, placements, pairs, scripts, rescues, Tags(mapq, md, rescue_scripts, rescue_md)), the placements and
    the pairs as the rescue leaves them"""
    text = np.asarray(text, np.uint8)
    reads, loci, al = _front(text, sigma, ranks, roff, w, complement, stride, band, min_votes, max_occ, max_edits, max_span)
    dist, start, end, best, _ = al.arrays
    f = pn.fold_pairs(loci.arrays[0], dist, start, end, best, min_insert, max_insert, orientation)
    p, pr, counters, jobs, totals = rn.rescue(text, sigma, *reads.arrays, loci.arrays[0], dist, start, end, f[:7], f[7:11], min_insert, max_insert,
                                              max_edits, orientation)
    pl = Stage("placements", tuple(p), {k: counters[k] for k in ("nr", "n_placed", "n_reverse", "n_ambiguous")})
    prs = Stage("pairs", tuple(pr), dict({k: counters[k] for k in ("np", "n_concordant", "n_discordant", "n_single", "n_unplaced")},
                                         n_ambiguous=counters["n_pairs_ambiguous"]))
    res = Stage("rescues", tuple(jobs), dict(totals))
    sc = _scripts("scripts", text, sigma, reads, loci.arrays[0], dist, start, end, p[6])
    md = _md(sc.arrays[1], sc.arrays[2], sc.arrays[3], start, end, text, letters)
    job_off, read, _, _, jdist, jstart, jend, status = jobs
    taken = np.full(reads.arrays[1].size - 1, NO, np.uint32)
    taken[read[status == 3]] = 0                               # (at most one job per internal read)
    rsc = _scripts("rescue_scripts", text, sigma, reads, job_off, jdist, jstart, jend, taken)
    rmd = _md(rsc.arrays[1], rsc.arrays[2], rsc.arrays[3], jstart, jend, text, letters, bound=int(read.size))
    return (reads, loci, al, pl, prs, sc, res, Tags(_mapq(p, max_edits, pr), md, rsc, rmd))
