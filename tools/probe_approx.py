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
--strands times the both-strand search (kmx_search_approx_strands) of every leg, reads from synth.planted_reads_strands (a
seeded half reverse-complemented; with --edit also the edit form, reads from synth.planted_reads_edit_strands): reads/s end
to end, piece hits, chunks, hits per strand, and the check that every read's source start is among its hits on its strand.
--baseline times, on the same reads, what a caller does without that entry point: kmx_search_approx of the batch, the
reverse complement of every read on the host, kmx_search_approx of that batch, and a numpy merge of the two results by
(query, position, strand); it uses only kmx_search_approx, so it also runs against a library that lacks the new symbol.
--no-plain skips the single-strand legs.
--report (with --edit) times, on every leg's edit reads, the reporting call (kmx_search_approx_opts) with loci + best and with
loci + best + max_hits = 1 next to the plain KMX_APPROX_EDIT call of the same run and the numpy pass a caller runs on the
plain result to get the same answer (host_report): end-to-end times, hits returned against the plain call's, bytes copied to
the host, whether the arrays equal the host filter's, and how many reads have a returned hit within e of their planted start.
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


def sources_found_strands(ho, pos, strands, start, strand):
    """How many reads have (source start, strand) among their hits."""
    nq = start.size
    qi = np.repeat(np.arange(nq, dtype=np.uint64), np.diff(ho).astype(np.int64))
    keys = (qi << np.uint64(33)) | (pos.astype(np.uint64) << np.uint64(1)) | strands.astype(np.uint64)
    want = (np.arange(nq, dtype=np.uint64) << np.uint64(33)) | (start.astype(np.uint64) << np.uint64(1)) | strand.astype(np.uint64)
    at = np.searchsorted(keys, want)
    return int(np.sum((at < keys.size) & (keys[np.minimum(at, keys.size - 1)] == want)))


def host_merge(nq, fwd, rev):
    """Two results of kmx_search_approx (hit_off, positions, distances[, lengths]) as one, ordered by (query, position,
    strand): what kmx_search_approx_strands returns, made with numpy."""
    keys, cols = [], []
    for strand, (ho, pos, *rest) in enumerate((fwd, rev)):
        qi = np.repeat(np.arange(nq, dtype=np.uint64), np.diff(ho).astype(np.int64))
        keys.append((qi << np.uint64(33)) | (pos.astype(np.uint64) << np.uint64(1)) | np.uint64(strand))
        cols.append(rest)
    keys = np.concatenate(keys)
    order = np.argsort(keys, kind="stable")
    keys = keys[order]
    out_ho = np.zeros(nq + 1, np.uint64)
    out_ho[1:] = fwd[0][1:] + rev[0][1:]
    merged = [np.concatenate([c[k] for c in cols])[order] for k in range(len(cols[0]))]
    return out_ho, ((keys >> np.uint64(1)) & np.uint64(0xFFFFFFFF)).astype(np.uint32), (keys & np.uint64(1)).astype(np.uint8), merged


def host_report(nq, e, ho, pos, dist, lens, max_hits):
    """loci + best (+ cap) of a one-strand KMX_APPROX_EDIT result with numpy, as a caller without kmx_search_approx_opts does
    it: (hit_off, positions, distances, lengths, found).  One-strand lists ascend strictly, so the hits within e letters of a
    hit are among its e list neighbours on each side."""
    nh = pos.size
    qi = np.repeat(np.arange(nq, dtype=np.int64), np.diff(ho).astype(np.int64))
    p, d = pos.astype(np.int64), dist.astype(np.int64)
    alive = np.ones(nh, bool)
    for j in range(1, e + 1):
        near = (qi[j:] == qi[:-j]) & (p[j:] - p[:-j] <= e)
        alive[j:] &= ~(near & (d[:-j] <= d[j:]))             # a left neighbour at no greater distance
        alive[:-j] &= ~(near & (d[j:] < d[:-j]))             # a right neighbour at a smaller one
    least = np.full(nq, 255, np.int64)
    np.minimum.at(least, qi[alive], d[alive])
    keep = alive & (d == least[qi])
    found = np.bincount(qi[keep], minlength=nq).astype(np.uint64)
    if max_hits:                                             # one stratum is left: the first max_hits of each list
        c = np.cumsum(keep) - keep
        first = np.concatenate([[0], np.cumsum(np.bincount(qi, minlength=nq))])[:-1]
        rank = c - np.where(first < nh, c[np.minimum(first, max(nh - 1, 0))], 0)[qi]
        keep &= rank < max_hits
    out_ho = np.zeros(nq + 1, np.uint64)
    np.cumsum(np.bincount(qi[keep], minlength=nq), out=out_ho[1:])
    return out_ho, pos[keep], dist[keep], lens[keep], found


def sources_near(ho, pos, start, e):
    """How many reads have a hit within e letters of their planted start."""
    nq = start.size
    qi = np.repeat(np.arange(nq, dtype=np.int64), np.diff(ho).astype(np.int64))
    near = np.abs(pos.astype(np.int64) - start.astype(np.int64)[qi]) <= e
    return int(np.count_nonzero(np.bincount(qi[near], minlength=nq)))


def report_legs(idx, nq, m, e, q, off, start, passes):
    """--report: the plain edit call + host_report against the reporting call, loci + best and loci + best + max_hits = 1."""
    box = {}

    def plain():
        r = idx.search_approx(q, off, e, edit=True)
        box["plain"] = r.host() + (r.lengths(),)
        r.close()

    t_plain = median_time(plain, passes)
    p_min, p_max = median_time.spread
    ho, pos, dist, st, lens = box["plain"]
    rec = {"plain": {"median_s": round(t_plain, 5), "min_s": round(p_min, 5), "max_s": round(p_max, 5), "spread_s": round(p_max - p_min, 5),
                     "n_hits": int(pos.size), "bytes_to_host": int((nq + 1) * 8 + nq + pos.size * 9),
                     "sources_near": sources_near(ho, pos, start, e)}}
    margin = max(0.03 * t_plain, p_max - p_min)
    for name, max_hits in (("loci_best", 0), ("loci_best_max1", 1)):
        def call():
            r = idx.search_approx(q, off, e, edit=True, loci=True, best=True, max_hits=max_hits)
            box["rep"] = r.host() + (r.lengths(), r.found())
            box["counts"] = r.counts()
            r.close()

        t = median_time(call, passes)
        t_min, t_max = median_time.spread
        t_filter = median_time(lambda: box.__setitem__("want", host_report(nq, e, ho, pos, dist, lens, max_hits)), passes)
        rho, rpos, rdist, rst, rlens, rfound = box["rep"]
        same = all(np.array_equal(x, y) for x, y in zip(box["want"], (rho, rpos, rdist, rlens, rfound))) and np.array_equal(rst, st)
        rec[name] = {"median_s": round(t, 5), "min_s": round(t_min, 5), "max_s": round(t_max, 5), "n_hits": int(rpos.size),
                     "hits_vs_plain": round(rpos.size / max(pos.size, 1), 4), "bytes_to_host": int((nq + 1) * 8 + nq + rpos.size * 9 + nq * 8),
                     "n_chunks": box["counts"]["n_chunks"], "reads_cut_by_cap": int(np.sum(rfound > np.diff(rho))),
                     "sources_near": sources_near(rho, rpos, start, e), "host_filter_median_s": round(t_filter, 5),
                     "plain_plus_host_filter_s": round(t_plain + t_filter, 5), "equals_host_filter": bool(same),
                     "vs_plain": round(t / t_plain, 3), "within_margin_of_plain": bool(t <= t_plain + margin)}
    return rec


def strand_legs(idx, text, leg, edit, args, comp):
    """The both-strand call and / or its two-call baseline on one leg's strand-planted reads."""
    nq, m, e, seed = LEGS[leg]
    n, sigma = text.size, 4
    gen = synth.planted_reads_edit_strands if edit else synth.planted_reads_strands
    q, off, strand, start = gen(seed, text, nq, m, sigma, e, comp)
    rec = {}
    box = {}
    if args.strands:
        def run():
            r = idx.search_approx(q, off, e, edit=edit, strands=True, complement=comp)
            box["host"] = r.host()
            box["strands"] = r.strands()
            if edit:
                box["lengths"] = r.lengths()
            box["counts"] = r.counts()
            r.close()

        t = median_time(run, args.passes)
        t_min, t_max = median_time.spread
        ho, pos, dist, st = box["host"]
        sb, c = box["strands"], box["counts"]
        rec["strands"] = {"median_s": round(t, 5), "min_s": round(t_min, 5), "max_s": round(t_max, 5), "reads_per_s": round(nq / t, 1),
                          "n_candidates": c["n_candidates"], "n_hits": c["n_hits"], "n_chunks": c["n_chunks"],
                          "hits_forward": int(np.sum(sb == 0)), "hits_reverse": int(np.sum(sb == 1)), "reads_reverse": int(strand.sum()),
                          "status_ok": int(np.sum(st == engine.Q_OK)), "sources_found_on_strand": sources_found_strands(ho, pos, sb, start, strand)}
    if args.baseline:
        def two_calls():
            t0 = time.perf_counter()
            r = idx.search_approx(q, off, e, edit=edit)
            f = r.host()[:3] + ((r.lengths(),) if edit else ())
            r.close()
            t1 = time.perf_counter()
            rc = synth.revcomp(q, off, comp)
            t2 = time.perf_counter()
            r = idx.search_approx(rc, off, e, edit=edit)
            v = r.host()[:3] + ((r.lengths(),) if edit else ())
            r.close()
            t3 = time.perf_counter()
            box["merged"] = host_merge(nq, f, v)
            t4 = time.perf_counter()
            box["parts"] = (t1 - t0 + t3 - t2, t2 - t1, t4 - t3)

        parts = []

        def timed():
            two_calls()
            parts.append(box["parts"])

        t = median_time(timed, args.passes)
        t_min, t_max = median_time.spread
        parts = np.array(parts[1:])                              # (without the warm-up)
        ho, pos, sb, _ = box["merged"]
        rec["baseline_two_calls"] = {"median_s": round(t, 5), "min_s": round(t_min, 5), "max_s": round(t_max, 5), "spread_s": round(t_max - t_min, 5),
                                     "reads_per_s": round(nq / t, 1), "two_searches_median_s": round(float(np.median(parts[:, 0])), 5),
                                     "host_revcomp_median_s": round(float(np.median(parts[:, 1])), 5),
                                     "host_merge_median_s": round(float(np.median(parts[:, 2])), 5), "n_hits": int(pos.size),
                                     "sources_found_on_strand": sources_found_strands(ho, pos, sb, start, strand)}
        if args.strands:
            same = np.array_equal(ho, box["host"][0]) and np.array_equal(pos, box["host"][1]) and np.array_equal(sb, box["strands"])
            rec["baseline_two_calls"]["equals_strands_call"] = bool(same)
            rec["strands"]["vs_baseline"] = round(rec["strands"]["median_s"] / t, 3)
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--legs", default="abc")
    ap.add_argument("--passes", type=int, default=5)
    ap.add_argument("--no-pieces", action="store_true", help="skip the piece-search-alone timing")
    ap.add_argument("--edit", action="store_true", help="also time the edit-distance search of every leg")
    ap.add_argument("--strands", action="store_true", help="time the both-strand search (kmx_search_approx_strands) of every leg")
    ap.add_argument("--baseline", action="store_true", help="time two plain calls + host reverse complement + host merge on the strand reads")
    ap.add_argument("--no-plain", action="store_true", help="skip the single-strand legs")
    ap.add_argument("--report", action="store_true", help="with --edit: time the reporting call (loci + best, + max_hits = 1) against the plain call")
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
    comp = np.array([3, 2, 1, 0], np.uint8)                   # ACGT
    for leg in args.legs:
        nq, m, e, seed = LEGS[leg]
        if args.no_plain:
            rec = {"nq": nq, "m": m, "e": e}
            rec["both_strands"] = strand_legs(idx, text, leg, False, args, comp)
            if args.edit:
                rec["both_strands_edit"] = strand_legs(idx, text, leg, True, args, comp)
            out["legs"][leg] = rec
            print(f"leg {leg}: m={m} e={e} {json.dumps(rec)}", flush=True)
            continue
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
            if args.report:
                rec["report"] = report_legs(idx, nq, m, e, q2, off2, start2, args.passes)
        if args.strands or args.baseline:
            rec["both_strands"] = strand_legs(idx, text, leg, False, args, comp)
            if args.edit:
                rec["both_strands_edit"] = strand_legs(idx, text, leg, True, args, comp)
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
