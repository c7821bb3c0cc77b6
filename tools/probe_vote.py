#!/usr/bin/env python3
"""kmx_windows_vote against what a caller does without it.  BASELINE configs[1] index (DNA4, n = 1e8, k = 10), reads of 150
letters cut from the text with 2 % substitutions, stride 1, band = 8, min_votes = 4, at max_occ 0 and 200:
  (a) windows search + vote + host view of the loci;
  (b) windows search + host view of the hits + tests/vote_naive.vote on the host, the numpy part timed separately.
Median of --passes passes after a warm-up ((b)'s numpy part: --naive-passes passes, no warm-up: it has no state to warm).
Array equality of (a) and (b) is checked once per max_occ.  Writes the times, the bytes that crossed to the host on each side
and k_vote's share of the kernel time of (a) to profiles/vote_probe.json.  --no-baseline runs (a) alone (the numpy side of (b)
needs minutes and tens of GB at the full 1e5 reads).  DESIGN.md section 7g."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from kmer_index_amd import engine, synth  # noqa: E402
from tests.vote_naive import vote  # noqa: E402


def timed(fn, passes, warm=True):
    if warm:
        fn()
    t = []
    for _ in range(passes):
        t0 = time.perf_counter()
        fn()
        t.append(1e3 * (time.perf_counter() - t0))
    return {"median_ms": float(np.median(t)), "min_ms": min(t), "max_ms": max(t), "passes_ms": t}


def make_reads(text, n_reads, length):
    z = synth.u64_stream(3003, n_reads * (length + 1)).astype(np.int64) & 0x7FFFFFFFFFFF
    start = z[:n_reads] % (text.size - length + 1)
    ranks = text[(start[:, None] + np.arange(length, dtype=np.int64)[None, :]).reshape(-1)].copy()
    u = z[n_reads:]
    sub = u % 50 == 0                                         # 2 % substitutions
    ranks[sub] = (ranks[sub] + 1 + (u[sub] >> 8) % 3) % 4
    return ranks.astype(np.uint8), np.arange(n_reads + 1, dtype=np.uint64) * np.uint64(length)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=100_000_000)
    ap.add_argument("--reads", type=int, default=100_000)
    ap.add_argument("--len", type=int, default=150)
    ap.add_argument("--passes", type=int, default=5)
    ap.add_argument("--naive-passes", type=int, default=5)
    ap.add_argument("--no-baseline", action="store_true")
    ap.add_argument("--json", default=os.path.join("profiles", "vote_probe.json"))
    a = ap.parse_args()

    k, stride, band, min_votes = 10, 1, 8, 4
    text = synth.ranks(1002, a.n, 4)
    idx = engine.Index(text, 4, [k])
    ranks, roff = make_reads(text, a.reads, a.len)
    out = {"n": a.n, "k": k, "reads": a.reads, "read_len": a.len, "stride": stride, "band": band, "min_votes": min_votes,
           "passes": a.passes, "naive_passes": a.naive_passes, "runs": {}}
    res, loci = engine.Result(), engine.Loci()
    for max_occ in (0, 200):
        run = {}

        def path_a():
            idx.search_windows(ranks, roff, k, stride, result=res)
            return res.vote(band, min_votes, max_occ, loci=loci).host()
        run["a_windows_vote_view"] = timed(path_a, a.passes)
        got = path_a()
        c = loci.counts()
        run["counts"] = c
        run["hits"] = res.counts()["n_hits"]
        run["a_bytes_to_host"] = int(sum(x.nbytes for x in got))
        run["a_bytes_per_locus"] = run["a_bytes_to_host"] / max(c["n_loci"], 1)
        # k_vote's share of the kernel time of one pass of (a)
        idx.stats_enable(True)
        idx.stats_reset()
        path_a()
        stats = idx.stats()
        idx.stats_enable(False)
        total = sum(s["total_ms"] for s in stats.values())
        run["a_kernel_ms"] = {name: s["total_ms"] for name, s in stats.items() if s["launches"]}
        run["a_k_vote_share"] = stats["k_vote"]["total_ms"] / total if total else 0.0
        if not a.no_baseline:
            def path_b_device():
                idx.search_windows(ranks, roff, k, stride, result=res)
                return res.host(copy=False), res.window_offsets()
            run["b_windows_view_hits"] = timed(path_b_device, a.passes)
            host, win = path_b_device()
            run["b_numpy_vote"] = timed(lambda: vote(host[0], host[1], win, stride, band, min_votes, max_occ), a.naive_passes, warm=False)
            want = vote(host[0], host[1], win, stride, band, min_votes, max_occ)
            run["arrays_equal"] = bool(all(g.dtype == x.dtype and np.array_equal(g, x) for g, x in zip(got, want[:5])) and c["n_votes"] == want[5])
            run["b_bytes_to_host"] = int(host[0].nbytes + host[1].nbytes + host[2].nbytes + host[3].nbytes + win.nbytes)
            run["b_bytes_per_hit"] = run["b_bytes_to_host"] / max(run["hits"], 1)
            b_med = run["b_windows_view_hits"]["median_ms"] + run["b_numpy_vote"]["median_ms"]
            b_spread = (run["b_windows_view_hits"]["max_ms"] - run["b_windows_view_hits"]["min_ms"]) + \
                       (run["b_numpy_vote"]["max_ms"] - run["b_numpy_vote"]["min_ms"])
            run["b_total_median_ms"] = b_med
            run["b_spread_ms"] = b_spread
            run["a_beats_b_by_more_than_b_spread"] = bool(run["a_windows_vote_view"]["median_ms"] + b_spread < b_med)
        out["runs"]["max_occ_%d" % max_occ] = run
    os.makedirs(os.path.dirname(a.json) or ".", exist_ok=True)
    with open(a.json, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
