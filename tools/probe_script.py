#!/usr/bin/env python3
"""kmx_alignments_scripts on the workload of tools/probe_vote.py / tools/probe_align.py.  BASELINE configs[1] index (DNA4, n = 1e8,
k = 10), reads of 150 letters cut from the text with 2 % substitutions, stride 1, band = 8, min_votes = 4, max_edits = 8 and
max_span = 64:
  (a)  windows search + vote + align + host views of the loci and the alignments (the path that existed before: it must reproduce
       probe_align's (a') figure);
  (a') the same + kmx_alignments_scripts + host view of the scripts.
Median of --passes passes after a warm-up.  Writes the times, the scripts call alone (timed from outside: the k_script_* kernels
have no slot in kmx_stats_get), the bytes that crossed to the host, n_sel and n_ops, and the same with KMX_SCRIPT_ALL, to
profiles/script_probe.json.  For the kernel split run --passes 1 under rocprofv3 --kernel-trace --stats.  DESIGN.md section 7i."""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from kmer_index_amd import engine, synth  # noqa: E402
from tools.probe_vote import make_reads, timed  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=100_000_000)
    ap.add_argument("--reads", type=int, default=100_000)
    ap.add_argument("--len", type=int, default=150)
    ap.add_argument("--passes", type=int, default=5)
    ap.add_argument("--max-edits", type=int, default=8)
    ap.add_argument("--max-span", type=int, default=64)
    ap.add_argument("--json", default=os.path.join("profiles", "script_probe.json"))
    a = ap.parse_args()

    k, stride, band, min_votes = 10, 1, 8, 4
    text = synth.ranks(1002, a.n, 4)
    idx = engine.Index(text, 4, [k])
    ranks, roff = make_reads(text, a.reads, a.len)
    out = {"n": a.n, "k": k, "reads": a.reads, "read_len": a.len, "stride": stride, "band": band, "min_votes": min_votes,
           "max_edits": a.max_edits, "max_span": a.max_span, "passes": a.passes}
    res, loci, al, scr = engine.Result(), engine.Loci(), engine.Alignments(), engine.Scripts()

    def path_a():
        idx.search_windows(ranks, roff, k, stride, result=res)
        got = res.vote(band, min_votes, 0, loci=loci).host()
        return got + loci.align(idx, ranks, roff, a.max_edits, a.max_span, alignments=al).host()

    out["a_windows_vote_align_views"] = timed(path_a, a.passes)
    out["a_bytes_to_host"] = int(sum(x.nbytes for x in path_a()))
    out["loci_counts"], out["align_counts"] = loci.counts(), al.counts()
    for name, every in (("best", False), ("all", True)):
        def path_a2():
            return path_a() + al.scripts(idx, loci, ranks, roff, all=every, scripts=scr).host()

        def scripts_only():
            return al.scripts(idx, loci, ranks, roff, all=every, scripts=scr).counts()

        rec = {"a2_with_scripts_and_view": timed(path_a2, a.passes)}
        rec["scripts_call_alone"] = timed(scripts_only, a.passes)   # upload of the reads, kernels, the two small read-backs; no host view
        got = scr.host()
        rec["counts"] = scr.counts()
        rec["script_bytes_to_host"] = int(sum(x.nbytes for x in got))
        rec["a2_bytes_to_host"] = out["a_bytes_to_host"] + rec["script_bytes_to_host"]
        rec["entries_per_s_scripts_call"] = rec["counts"]["n_sel"] / (1e-3 * rec["scripts_call_alone"]["median_ms"])
        rec["added_ms"] = rec["a2_with_scripts_and_view"]["median_ms"] - out["a_windows_vote_align_views"]["median_ms"]
        rec["runs_per_entry_histogram"] = {str(c): int(v) for c, v in zip(*np.unique(np.diff(got[2].astype(np.int64)), return_counts=True))}
        out[name] = rec
    os.makedirs(os.path.dirname(a.json) or ".", exist_ok=True)
    with open(a.json, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
