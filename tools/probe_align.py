#!/usr/bin/env python3
"""kmx_loci_align on the workload of tools/probe_vote.py.  BASELINE configs[1] index (DNA4, n = 1e8, k = 10), reads of 150 letters
cut from the text with 2 % substitutions, stride 1, band = 8, min_votes = 4, then max_edits = 8 and max_span = 64:
  (a)  windows search + vote + host view of the loci (the path that existed before: it must reproduce probe_vote's figure);
  (a') the same + kmx_loci_align + host view of the alignments.
Median of --passes passes after a warm-up.  Writes the times, the bytes that crossed to the host, loci per second of the align
call alone (timed from outside: the k_align_* kernels have no slot in kmx_stats_get) and the bit-vector column updates of the
forward pass (computed from the loci: a column per text letter of every window, a word update per 64 read letters of the
locus's class) to profiles/align_probe.json.  For the kernel split run --passes 1 under rocprofv3 --kernel-trace --stats and
divide the column updates by the time of k_align_fwd.  DESIGN.md section 7h."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from kmer_index_amd import engine, synth  # noqa: E402
from tools.probe_vote import make_reads, timed  # noqa: E402


def forward_work(n, roff, off, diag, span, dist, max_edits):
    """(columns, word updates) of the forward pass: per aligned-or-not locus hi - lo columns, each over NW words."""
    m = np.repeat(np.diff(roff.astype(np.int64)), np.diff(off.astype(np.int64)))
    run = dist != engine.ALIGN_SKIPPED
    lo = np.maximum(diag - max_edits, 0)
    hi = np.maximum(lo, np.minimum(n, diag + span.astype(np.int64) + m + max_edits))
    nw = (m + 63) // 64
    cls = np.select([nw <= 1, nw <= 2, nw <= 4, nw <= 8], [1, 2, 4, 8], 16)
    cols = np.where(run, hi - lo, 0)
    return int(cols.sum()), int((cols * cls).sum())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=100_000_000)
    ap.add_argument("--reads", type=int, default=100_000)
    ap.add_argument("--len", type=int, default=150)
    ap.add_argument("--passes", type=int, default=5)
    ap.add_argument("--max-edits", type=int, default=8)
    ap.add_argument("--max-span", type=int, default=64)
    ap.add_argument("--json", default=os.path.join("profiles", "align_probe.json"))
    a = ap.parse_args()

    k, stride, band, min_votes = 10, 1, 8, 4
    text = synth.ranks(1002, a.n, 4)
    idx = engine.Index(text, 4, [k])
    ranks, roff = make_reads(text, a.reads, a.len)
    out = {"n": a.n, "k": k, "reads": a.reads, "read_len": a.len, "stride": stride, "band": band, "min_votes": min_votes,
           "max_edits": a.max_edits, "max_span": a.max_span, "passes": a.passes}
    res, loci, al = engine.Result(), engine.Loci(), engine.Alignments()

    def path_a():
        idx.search_windows(ranks, roff, k, stride, result=res)
        return res.vote(band, min_votes, 0, loci=loci).host()

    def path_a2():
        got = path_a()
        return got, loci.align(idx, ranks, roff, a.max_edits, a.max_span, alignments=al).host()

    def align_only():
        return loci.align(idx, ranks, roff, a.max_edits, a.max_span, alignments=al).counts()

    out["a_windows_vote_view"] = timed(path_a, a.passes)
    out["a2_windows_vote_align_views"] = timed(path_a2, a.passes)
    got, aligned = path_a2()
    out["align_call_alone"] = timed(align_only, a.passes)       # upload of the reads, kernels, the two small read-backs; no host view
    c, ca = loci.counts(), al.counts()
    out["loci_counts"], out["align_counts"] = c, ca
    out["a_bytes_to_host"] = int(sum(x.nbytes for x in got))
    out["a2_bytes_to_host"] = out["a_bytes_to_host"] + int(sum(x.nbytes for x in aligned))
    out["align_bytes_per_locus"] = sum(x.nbytes for x in aligned) / max(ca["n_loci"], 1)
    out["loci_per_s_align_call"] = ca["n_loci"] / (1e-3 * out["align_call_alone"]["median_ms"]) if ca["n_loci"] else 0.0
    cols, words = forward_work(a.n, roff, got[0], got[1], got[2], aligned[0], a.max_edits)
    out["forward_columns"], out["forward_word_updates"] = cols, words
    out["dist_histogram"] = {str(d): int(v) for d, v in zip(*np.unique(aligned[0], return_counts=True))}
    os.makedirs(os.path.dirname(a.json) or ".", exist_ok=True)
    with open(a.json, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
