#!/usr/bin/env python
"""kmx_clips_pileup_device and kmx_pileup_sites, beside kmx_scripts_clip on the same handles, at a batch of the size the test suite
runs: 4000 public reads of 150 letters (8000 internal reads) on a DNA4 text of 10^6 letters, k = 10.  A SMALL-BATCH FIGURE THAT
INCLUDES LAUNCH OVERHEADS AND THE ZEROING OF THE PLANES: no rate at a user's size follows from it.  The tiled path
that DESIGN.md 7t records was measured with this probe while it existed (the rows under "tiled_path_as_measured" of
profiles/pileup_probe.json); the library has one path now, and the probe times that.

Two shapes.  sparse: every read comes from a random place of the text (coverage 0.6), the region is the text.  dense: the same reads
drawn from a window of 20 000 letters (coverage 30), the region once the window and once the text.  Each call is timed between two
device events on the stream of the batch, after a warm-up, --passes times; the median, the least and the greatest go to --json
(profiles/pileup_probe.json).  The host alternative is an estimate: the time to copy the scripts and the reads to the host, plus
tests/pileup_naive.py on 200 entries scaled up to the batch."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from kmer_index_amd import engine, synth  # noqa: E402
from tests import pileup_naive  # noqa: E402
from tools.probe_realign import timed  # noqa: E402

WINDOW = 20_000


def reads_of(text, n_reads, m, seed, w0, width):
    """n_reads reads of m letters from [w0, w0 + width) with 0 .. 3 substitutions, every other one reverse-complemented"""
    z = synth.u64_stream(seed, 8 * n_reads).astype(np.int64) & 0x7FFFFFFF
    comp = engine.complement_table(4)
    out = []
    for p in range(n_reads):
        zz = z[8 * p:8 * p + 8]
        s = w0 + int(zz[0] % (width - m))
        q = text[s:s + m].copy()
        for e in range(int(zz[1] % 4)):
            at = int(zz[2 + e] % m)
            q[at] = (q[at] + 1 + int(zz[5 + e] % 3)) % 4
        out.append(comp[q[::-1]] if p % 2 else q)
    return np.concatenate(out).astype(np.uint8), (np.arange(n_reads + 1) * m).astype(np.uint64)


def host_alternative(sc, al, reads, n, n_entries=200):
    """seconds: the copies a host pileup needs, and the oracle's loop on the first n_entries entries scaled to all of them"""
    t0 = time.perf_counter()
    scripts = sc.host()
    d_ranks2, d_roff2, nr2, _ = reads.device_ptrs()
    import torch

    class _Arr:
        def __init__(self, ptr, nbytes):
            self.__cuda_array_interface__ = {"shape": (int(nbytes),), "typestr": "|u1", "data": (int(ptr), False), "version": 2}

    roff2 = torch.as_tensor(_Arr(d_roff2, 8 * (nr2 + 1)), device="cuda").cpu().numpy().view(np.uint64)
    ranks2 = torch.as_tensor(_Arr(d_ranks2, int(roff2[-1])), device="cuda").cpu().numpy()
    _, start, end = al.host()[:3]
    t1 = time.perf_counter()
    read_sel_off, sel, cig_off, cigar = scripts
    k = min(n_entries, sel.size)
    cut = np.minimum(read_sel_off, k)                           # the first k entries, with the reads they belong to
    counts = pileup_naive.planes(0, n, 4)
    pileup_naive.add(counts, 0, n, 4, (cut, sel[:k], cig_off[:k + 1], cigar), None, start, end, ranks2, roff2, n=n)
    t2 = time.perf_counter()
    return dict(copy_ms=1e3 * (t1 - t0), loop_ms_estimated=1e3 * (t2 - t1) * sel.size / max(k, 1), entries_run=int(k),
                what="an estimate: the loop ran on entries_run entries and is scaled to n_sel")


def shape(idx, text, ranks, roff, regions, a):
    comp = engine.complement_table(4)
    out = {}
    reads, loci, al, pl, sc = idx.map_reads_strands(ranks, roff, 10, comp, band=8, min_votes=2, max_edits=a.max_edits, max_span=64, scripts=True)
    d_ranks2, d_roff2, nr2, stream = reads.device_ptrs()
    cl, pu, st = engine.Clips(), engine.Pileup(), engine.Sites()
    out["internal_reads"], out["entries"] = nr2, sc.counts()
    out["scripts_clip"] = timed(stream, a.passes, lambda: sc.clip(stream=stream, clips=cl))
    for name, (lo, hi) in regions.items():
        r = out[name] = dict(lo=lo, hi=hi)
        r["clips_atomic"] = timed(stream, a.passes, lambda: cl.pileup(idx, sc, al, reads, lo=lo, hi=hi, stream=stream, pileup=pu))
        r["atomic"] = timed(stream, a.passes, lambda: sc.pileup(idx, al, reads, lo=lo, hi=hi, stream=stream, pileup=pu))
        r["atomic_add"] = timed(stream, a.passes, lambda: sc.pileup(idx, al, reads, lo=lo, hi=hi, add=True, stream=stream, pileup=pu))   # no zeroing
        sc.pileup(idx, al, reads, lo=lo, hi=hi, stream=stream, pileup=pu)
        r["counts"] = pu.counts()
        r["sites"] = timed(stream, a.passes, lambda: pu.sites(idx, min_alt=2, stream=stream, sites=st))
        r["sites_counts"] = st.counts()
    out["host_alternative"] = host_alternative(sc, al, reads, text.size)
    for h in (st, pu, cl, sc, pl, al, loci, reads):
        h.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--reads", type=int, default=4000)
    ap.add_argument("--read-len", type=int, default=150)
    ap.add_argument("--max-edits", type=int, default=24)
    ap.add_argument("--passes", type=int, default=7)
    ap.add_argument("--json", default=os.path.join("profiles", "pileup_probe.json"))
    a = ap.parse_args()
    if a.reads > 4096:
        sys.exit("probe_pileup: at most 4096 public reads (DESIGN.md 7k: the chain's front is not run above the suite's batch sizes)")
    text = synth.ranks(951, a.n, 4)
    idx = engine.Index(text, 4, [10], table=engine.TABLE_DENSE)
    w0 = a.n // 2
    out = dict(n=a.n, k=10, reads=a.reads, read_len=a.read_len, max_edits=a.max_edits, passes=a.passes, window=[w0, w0 + WINDOW],
               what="small batch; device events around each call: launch overheads and the zeroing of the planes included")
    out["sparse"] = shape(idx, text, *reads_of(text, a.reads, a.read_len, 952, 0, a.n), dict(text=(0, a.n)), a)
    out["dense"] = shape(idx, text, *reads_of(text, a.reads, a.read_len, 953, w0, WINDOW), dict(window=(w0, w0 + WINDOW), text=(0, a.n)), a)
    if os.path.exists(a.json):                                 # the record of the path that was taken out stays with the file
        kept = json.load(open(a.json)).get("tiled_path_as_measured")
        if kept is not None:
            out["tiled_path_as_measured"] = kept
    os.makedirs(os.path.dirname(a.json) or ".", exist_ok=True)
    with open(a.json, "w") as f:
        json.dump(out, f, indent=1)

    def brief(v):
        if isinstance(v, dict):
            return v["median_ms"] if "median_ms" in v else {k: brief(x) for k, x in v.items()}
        return v

    print(json.dumps(brief(out)))
    idx.close()


if __name__ == "__main__":
    main()
