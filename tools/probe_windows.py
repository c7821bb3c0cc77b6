#!/usr/bin/env python3
"""kmx_search_windows against what a caller runs without it: the windows written out as separate queries (the expanded batch)
through kmx_search_batch / kmx_search_batch_device, with the host-side expansion timed separately.  BASELINE configs[1] index
(DNA4, n = 1e8, k = 10), 1e5 random reads of 150 letters, stride 1 (1.41e7 windows); median of 5 passes after a warm-up, for
the host form (call + host view) and the device form (call + stream synchronisation, inputs resident).  Checks that the
arrays of both forms equal the expanded batch's and writes profiles/windows_probe.json.  DESIGN.md section 7f."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from kmer_index_amd import engine, synth  # noqa: E402
from tests.windows_naive import expand  # noqa: E402


def timed(fn, passes):
    fn()                                                    # warm-up
    t = []
    for _ in range(passes):
        t0 = time.perf_counter()
        fn()
        t.append(1e3 * (time.perf_counter() - t0))
    return {"median_ms": float(np.median(t)), "min_ms": min(t), "max_ms": max(t), "passes_ms": t}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=100_000_000)
    ap.add_argument("--reads", type=int, default=100_000)
    ap.add_argument("--len", type=int, default=150)
    ap.add_argument("--stride", type=int, default=1)
    ap.add_argument("--passes", type=int, default=5)
    ap.add_argument("--json", default=os.path.join("profiles", "windows_probe.json"))
    a = ap.parse_args()
    import torch

    k = 10
    idx = engine.Index(synth.ranks(1002, a.n, 4), 4, [k])
    ranks = synth.ranks(3003, a.reads * a.len, 4)
    roff = np.arange(a.reads + 1, dtype=np.uint64) * np.uint64(a.len)
    t0 = time.perf_counter()
    q, qoff, win = expand(ranks, roff, k, a.stride)
    expand_ms = 1e3 * (time.perf_counter() - t0)
    nq = qoff.size - 1
    out = {"n": a.n, "k": k, "reads": a.reads, "read_len": a.len, "stride": a.stride, "windows": nq, "passes": a.passes,
           "host_expansion_ms": expand_ms, "bytes_up_windows": int(ranks.size + roff.size * 8), "bytes_up_expanded": int(q.size + qoff.size * 8)}

    # host forms: call + host view
    res_w, res_e = engine.Result(), engine.Result()
    out["host_windows"] = timed(lambda: idx.search_windows(ranks, roff, k, a.stride, result=res_w).host(copy=False), a.passes)
    out["host_expanded"] = timed(lambda: idx.search(q, qoff, result=res_e).host(copy=False), a.passes)
    got, want = res_w.host(copy=False), res_e.host(copy=False)
    out["host_arrays_equal"] = bool(all(np.array_equal(g, x) for g, x in zip(got, want)) and np.array_equal(res_w.window_offsets(), win))
    out["hits"] = int(want[0][-1])

    # device forms: inputs resident, call + synchronisation
    def up(x):
        return torch.from_numpy(x.view(np.int64) if x.dtype == np.uint64 else x).cuda()
    d_r, d_o, d_q, d_qo = up(ranks), up(roff), up(q), up(qoff)
    stream = torch.cuda.Stream()
    torch.cuda.synchronize()
    dev_w, dev_e = engine.Result(), engine.Result()

    def run_w():
        idx.search_windows_device(d_r.data_ptr(), d_o.data_ptr(), a.reads, k, a.stride, stream=stream.cuda_stream, result=dev_w)
        stream.synchronize()

    def run_e():
        idx.search_device(d_q.data_ptr(), d_qo.data_ptr(), nq, stream=stream.cuda_stream, result=dev_e)
        stream.synchronize()
    out["device_windows"] = timed(run_w, a.passes)
    out["device_expanded"] = timed(run_e, a.passes)
    got, want = dev_w.host(copy=False), dev_e.host(copy=False)
    out["device_arrays_equal"] = bool(all(np.array_equal(g, x) for g, x in zip(got, want)) and np.array_equal(dev_w.window_offsets(), win))
    for form in ("host", "device"):
        base, new = out[form + "_expanded"], out[form + "_windows"]
        margin = max(0.03 * base["median_ms"], base["max_ms"] - base["min_ms"])       # DESIGN 7c's rule
        out[form + "_margin_ms"] = margin
        out[form + "_within_margin_of_expanded"] = bool(new["median_ms"] <= base["median_ms"] + margin)
    os.makedirs(os.path.dirname(a.json) or ".", exist_ok=True)
    with open(a.json, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps({key: (v if not isinstance(v, dict) else {"median_ms": v["median_ms"], "min_ms": v["min_ms"], "max_ms": v["max_ms"]})
                      for key, v in out.items()}))


if __name__ == "__main__":
    main()
