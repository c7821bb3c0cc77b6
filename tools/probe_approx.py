#!/usr/bin/env python3
"""Approximate search (kmx_search_approx) on BASELINE config 2's index (DNA4, n = 1e8, k = 10, seed 1002, default options).

Legs (reads from synth.planted_reads, 0 .. e substitutions each):
  a  1e6 reads, m = 40,  e = 3  (four 10-letter pieces, ~381 candidates per read: verification-bound)
  b  1e6 reads, m = 20,  e = 1
  c  1e6 reads, m = 150, e = 3  (stitched pieces, few candidates: bound by the piece search)
Per leg: reads/s end to end (host buffers in, host arrays out; median of --passes timed passes after a warm-up), candidates/s,
the piece batch alone through Index.search (same pieces, host form), and a check that every read's source window is among its
hits.  Also: kmx_index_text's first derivation (time, packed bytes).  --json writes the result line to a file.
--edit adds to every leg the edit-distance search (KMX_APPROX_EDIT, same m and e, reads from synth.planted_reads_edit:
substitutions, insertions and deletions) next to the Hamming figures of the same run: reads/s, candidates/s, band cells/s
bound ((4e + 1) m cells per piece hit), hits, chunks, and the check that every read's source start is among its hits.
For a kernel trace run one leg with --passes 1 under rocprofv3 --kernel-trace --stats."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402,F401  (one HIP runtime per process: see engine.lib)
from kmer_index_amd import engine, synth  # noqa: E402

LEGS = {"a": (1_000_000, 40, 3, 3001), "b": (1_000_000, 20, 1, 3002), "c": (1_000_000, 150, 3, 3003)}


def piece_offsets(qoff, e):
    m = np.diff(qoff.astype(np.int64))
    base, rem = m // (e + 1), m % (e + 1)
    j = np.arange(e + 1, dtype=np.int64)
    starts = qoff[:-1].astype(np.int64)[:, None] + j[None, :] * base[:, None] + np.minimum(j[None, :], rem[:, None])
    return np.concatenate([starts.reshape(-1), qoff[-1:].astype(np.int64)]).astype(np.uint64)


def median_time(fn, passes):
    fn()                                                     # warm-up
    ts = []
    for _ in range(passes):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    median_time.spread = (float(min(ts)), float(max(ts)))     # of the last call
    return float(np.median(ts))


def sources_found(ho, pos, start):
    """How many reads have their source start among their hits."""
    nq = start.size
    qi = np.repeat(np.arange(nq, dtype=np.uint64), np.diff(ho).astype(np.int64))
    keys = (qi << np.uint64(32)) | pos.astype(np.uint64)
    want = (np.arange(nq, dtype=np.uint64) << np.uint64(32)) | start
    at = np.searchsorted(keys, want)
    return int(np.sum((at < keys.size) & (keys[np.minimum(at, keys.size - 1)] == want)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--legs", default="abc")
    ap.add_argument("--passes", type=int, default=5)
    ap.add_argument("--no-pieces", action="store_true", help="skip the piece-search-alone timing")
    ap.add_argument("--edit", action="store_true", help="also time the edit-distance search of every leg")
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    n, sigma = 100_000_000, 4
    text = synth.ranks(1002, n, sigma)
    idx = engine.Index(text, sigma, [10])
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    packed = idx.text_packed_bytes()
    derive_ms = (time.perf_counter() - t0) * 1e3
    out = {"probe": "approx", "config": 2, "n": n, "k": 10, "text_derive_ms": round(derive_ms, 2), "packed_bytes": packed, "legs": {}}
    print(f"kmx_index_text: first derivation {derive_ms:.2f} ms, {packed} packed bytes", flush=True)
    for leg in args.legs:
        nq, m, e, seed = LEGS[leg]
        q, off = synth.planted_reads(seed, text, nq, m, sigma, e)
        box = {}

        def run():
            r = idx.search_approx(q, off, e)
            box["host"] = r.host()
            box["counts"] = r.counts()
            r.close()

        t = median_time(run, args.passes)
        t_min, t_max = median_time.spread
        ho, pos, mm, st = box["host"]
        c = box["counts"]
        # every read's source window (planted with at most e substitutions) is among its hits
        start = (synth.u64_stream(seed, nq) % np.uint64(n - m + 1)).astype(np.uint64)
        found = sources_found(ho, pos, start)
        rec = {"nq": nq, "m": m, "e": e, "median_s": round(t, 5), "min_s": round(t_min, 5), "max_s": round(t_max, 5), "reads_per_s": round(nq / t, 1),
               "n_candidates": c["n_candidates"],
               "candidates_per_s": round(c["n_candidates"] / t, 1), "n_hits": c["n_hits"], "n_chunks": c["n_chunks"],
               "status_ok": int(np.sum(st == engine.Q_OK)), "sources_found": found}
        if not args.no_pieces:
            poff = piece_offsets(off, e)

            def pieces():
                r = idx.search(q, poff)
                r.host(copy=False)
                r.close()

            tp = median_time(pieces, args.passes)
            rec["piece_search_s"] = round(tp, 5)
        if args.edit:
            q2, off2, start2 = synth.planted_reads_edit(seed, text, nq, m, sigma, e)

            def run_edit():
                r = idx.search_approx(q2, off2, e, edit=True)
                box["host"] = r.host()
                box["lengths"] = r.lengths()
                box["counts"] = r.counts()
                r.close()

            t2 = median_time(run_edit, args.passes)
            t2_min, t2_max = median_time.spread
            ho2, pos2, dist2, st2 = box["host"]
            c2 = box["counts"]
            rec["edit"] = {"median_s": round(t2, 5), "min_s": round(t2_min, 5), "max_s": round(t2_max, 5), "reads_per_s": round(nq / t2, 1), "n_candidates": c2["n_candidates"],
                           "candidates_per_s": round(c2["n_candidates"] / t2, 1),
                           "band_cells_bound_per_s": round(c2["n_candidates"] * (4 * e + 1) * m / t2, 1), "n_hits": c2["n_hits"],
                           "hits_other_length": int(np.sum(box["lengths"] != m)), "n_chunks": c2["n_chunks"],
                           "status_ok": int(np.sum(st2 == engine.Q_OK)), "sources_found": sources_found(ho2, pos2, start2.astype(np.uint64)),
                           "slowdown_vs_hamming": round(t2 / t, 3)}
        out["legs"][leg] = rec
        print(f"leg {leg}: m={m} e={e} {json.dumps(rec)}", flush=True)
    idx.close()
    line = json.dumps(out)
    print(line)
    if args.json:
        with open(args.json, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
