#!/usr/bin/env python
"""kmx_scripts_realign_device beside kmx_alignments_scripts_device + kmx_scripts_clip on the same handles, at a batch of the size the
test suite runs: 4000 public reads of 150 letters (8000 internal reads) on a DNA4 text of 10^6 letters, k = 10.  A SMALL-BATCH FIGURE
THAT INCLUDES LAUNCH OVERHEADS AND THE CALLS' OWN READ-BACKS: no rate at a user's size follows from it.

Every read comes from a random place with 0 .. 3 edits; every tenth has lost 12 letters in a row, every other one is reverse-
complemented.  Each call is timed between two device events on the stream of the batch, after a warm-up, --passes times; the median,
the least and the greatest go to --json (profiles/realign_probe.json)."""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from kmer_index_amd import engine, synth  # noqa: E402


def reads_of(text, n_reads, m, seed):
    z = synth.u64_stream(seed, 8 * n_reads).astype(np.int64) & 0x7FFFFFFF
    comp = engine.complement_table(4)
    out = []
    for p in range(n_reads):
        zz = z[8 * p:8 * p + 8]
        s = int(zz[0] % (text.size - m - 16))
        q = text[s:s + m + 12].copy()
        q = np.concatenate([q[:70], q[82:]]) if p % 10 == 0 else q[:m]
        for e in range(int(zz[1] % 4)):
            at = int(zz[2 + e] % m)
            q[at] = (q[at] + 1 + int(zz[5 + e] % 3)) % 4
        out.append(comp[q[::-1]] if p % 2 else q)
    ranks = np.concatenate(out).astype(np.uint8)
    roff = np.concatenate([[0], np.cumsum([len(q) for q in out])]).astype(np.uint64)
    return ranks, roff


def timed(stream, passes, call):
    import torch

    s = torch.cuda.ExternalStream(stream) if stream else torch.cuda.current_stream()
    call()                                                     # the warm-up: buffers grow, code objects load
    ms = []
    for _ in range(passes):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(s)
        call()
        b.record(s)
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return dict(median_ms=float(np.median(ms)), min_ms=min(ms), max_ms=max(ms), passes_ms=ms)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--reads", type=int, default=4000)
    ap.add_argument("--read-len", type=int, default=150)
    ap.add_argument("--max-edits", type=int, default=24)
    ap.add_argument("--passes", type=int, default=7)
    ap.add_argument("--json", default=os.path.join("profiles", "realign_probe.json"))
    a = ap.parse_args()
    if a.reads > 4096:
        sys.exit("probe_realign: at most 4096 public reads (DESIGN.md 7k: the chain's front is not run above the suite's batch sizes)")
    text = synth.ranks(951, a.n, 4)
    ranks, roff = reads_of(text, a.reads, a.read_len, 952)
    idx = engine.Index(text, 4, [10], table=engine.TABLE_DENSE)
    comp = engine.complement_table(4)
    reads, loci, al, pl = idx.map_reads_strands(ranks, roff, 10, comp, band=8, min_votes=2, max_edits=a.max_edits, max_span=64)
    d_ranks2, d_roff2, nr2, stream = reads.device_ptrs()
    sc, cl, rl = engine.Scripts(), engine.Clips(), engine.Clips()
    out = dict(n=a.n, k=10, reads=a.reads, internal_reads=nr2, read_len=a.read_len, max_edits=a.max_edits, passes=a.passes,
               what="small batch; device events around each call, launch overheads and the calls' read-backs included")
    out["scripts_device"] = timed(stream, a.passes, lambda: al.scripts_device(idx, loci, d_ranks2, d_roff2, nr2, stream=stream, scripts=sc))
    out["scripts_clip"] = timed(stream, a.passes, lambda: sc.clip(stream=stream, clips=cl))
    out["scripts_realign_device"] = timed(stream, a.passes, lambda: sc.realign_device(idx, al, d_ranks2, d_roff2, nr2, stream=stream, clips=rl))
    out["entries"] = sc.counts()
    out["clips"], out["realigned"] = cl.counts(), rl.counts()
    trimmed, again = cl.host(), rl.host()
    out["entries_with_a_better_score"] = int((again.score > trimmed.score).sum())
    out["entries_with_a_worse_score"] = int((again.score < trimmed.score).sum())
    dist = al.host().dist[sc.host().sel]
    out["dist_histogram"] = np.bincount(dist, minlength=1).tolist()
    os.makedirs(os.path.dirname(a.json) or ".", exist_ok=True)
    with open(a.json, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps({k: (v["median_ms"] if isinstance(v, dict) and "median_ms" in v else v) for k, v in out.items() if k != "dist_histogram"}))
    for h in (rl, cl, sc, pl, al, loci, reads):
        h.close()
    idx.close()


if __name__ == "__main__":
    main()
