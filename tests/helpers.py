"""Shared helpers for the parity tests."""
import numpy as np

from kmer_index_amd import synth
from tests import image_writer as iw

CASES = [
    # (name, sigma, n, ks, lengths)  — lengths stay inside the reference's correct envelope
    ("dna4_k5", 4, 100_000, [5], list(range(1, 16)) + [20]),
    ("dna4_k10", 4, 400_000, [10], list(range(4, 31)) + [40]),
    ("dna5_k10", 5, 400_000, [10], list(range(5, 31))),
    ("aa20_k5", 20, 300_000, [5], list(range(1, 16))),
    ("dna4_multi", 4, 400_000, [8, 10, 12], list(range(2, 30)) + [33, 35]),
    ("dna15_k3_multi", 15, 200_000, [3, 4, 5], list(range(1, 10))),
]


def make_queries(text, sigma, lengths, per_length, seed):
    """Per length: 1/3 uniform random, 1/3 planted at a random offset, 1/3 planted in the text's tail
    (the tail set is what catches a missing last-kmer fix-up, kmer_index.hpp:90-112)."""
    n = text.size
    qs = []
    z = synth.u64_stream(seed, len(lengths) * per_length * 2)
    zi = 0
    for m in lengths:
        for t in range(per_length):
            if m > n or t % 3 == 0:
                q = synth.ranks(seed * 1000003 + m * 131 + t, m, sigma)
            elif t % 3 == 1:
                s = int(z[zi] % np.uint64(n - m + 1))
                q = text[s:s + m].copy()
            else:
                back = int(z[zi] % np.uint64(min(14, n - m) + 1))
                s = n - m - back
                q = text[s:s + m].copy()
            zi += 1
            qs.append(q)
    return pack(qs)


def pack(qs):
    off = np.zeros(len(qs) + 1, np.uint64)
    if qs:
        off[1:] = np.cumsum([len(q) for q in qs])
    ranks = np.concatenate(qs).astype(np.uint8) if qs and off[-1] else np.zeros(0, np.uint8)
    return ranks, off


def digest(hit_off, positions):
    """Order-sensitive 64-bit digest of a whole batch result (FNV-style over counts and positions)."""
    h = np.uint64(1469598103934665603)
    with np.errstate(over="ignore"):
        for arr in (np.diff(hit_off).astype(np.uint64), positions.astype(np.uint64)):
            # chunked polynomial fold: weights are powers of the FNV prime
            for s in range(0, arr.size, 1 << 20):
                a = arr[s:s + (1 << 20)] + np.uint64(1)
                w = np.uint64(1099511628211) ** np.arange(a.size, 0, -1, dtype=np.uint64)
                h = h * (np.uint64(1099511628211) ** np.uint64(a.size)) + np.sum(a * w, dtype=np.uint64)
    return int(h)


def inside_envelope(plan, ks, m):
    """is a query of m letters inside the envelope in which the reference's search() is correct (and the line-by-line
    restatement, MODE_FAITHFUL, therefore equals ground truth)?  plan = orc.plan(ks): (use_multi, nk_sum).
    Single k: any m <= k, exact multiples of k, at most two full parts with a rest (kmer_index.hpp:314 breaks the others);
    multi-k sums: at most two summands (kmer_index.hpp:526, :535)."""
    multi, nk_sum = plan
    if m <= 0 or m >= len(nk_sum) or not nk_sum[m]:
        return True                                   # rejected / unservable lengths: both modes agree on the status
    if multi[m] and len(ks) > 1:
        return len(nk_sum[m]) <= 2
    k = nk_sum[m][0]
    return m <= k or m % k == 0 or m // k <= 2


def mutate(src, m, d, sigma, rng):
    """A read of m letters: d edits of seeded kinds (substitution, deletion, insertion) at seeded columns below m of src,
    then the first m letters, filled up with seeded letters where deletions left fewer."""
    q = [int(x) for x in src]
    for _ in range(d):
        c = int(rng.integers(0, max(1, min(m, len(q)))))
        kind = int(rng.integers(3))
        if kind == 0 and q:
            q[c] = (q[c] + 1 + int(rng.integers(sigma - 1))) % sigma
        elif kind == 1 and q:
            del q[c]
        else:
            q.insert(c, int(rng.integers(sigma)))
    q = q[:m]
    while len(q) < m:
        q.append(int(rng.integers(sigma)))
    return np.array(q, np.uint8)


def random_involution(sigma, seed):
    """A seeded involution of [0, sigma) that is not the identity: a shuffled alphabet paired off two by two (an odd one
    left maps to itself)."""
    perm = np.random.default_rng(seed).permutation(sigma)
    t = np.arange(sigma, dtype=np.uint8)
    for a, b in zip(perm[0:sigma - 1:2], perm[1:sigma:2]):
        t[a], t[b] = b, a
    return t


# ---- mutants of a valid index image, for the fuzz of the loader --------------------------------------------------
_EXTREME = [0, 1, 2, 31, 32, 63, 64, 255, 256, 65535, 65536, 0x7FFFFFFF, 0x80000000, 0xFFFFFFFE, 0xFFFFFFFF,
            1 << 32, (1 << 40) + 1, 1 << 62, (1 << 63) - 1, 1 << 63, (1 << 64) - 1]


def _sections(data, n_ks, sizes):
    """(offset, length) of every checksummed section of an image laid out with the ORIGINAL sizes."""
    out, at = [], 48
    for ln in sizes:
        out.append((at, ln))
        at += (ln + 7) // 8 * 8
    return out


def image_mutants(rng, text, elems, n):
    """n byte strings: the valid image with a few bytes / fields changed, the checksum made right again."""
    import io
    import os
    import tempfile
    fd, path = tempfile.mkstemp(suffix=".kmx")
    os.close(fd)
    iw.write_image(path, text, 4, elems)
    good = open(path, "rb").read()
    os.remove(path)
    kmax = max(e["k"] for e in elems)
    sizes = [72 * len(elems), kmax]
    for e in elems:
        sizes += [4 * e["positions"].size, 4 * e["offs"].size, 4 * e["atab"].size, 16 * e["slots"].size, 8 * e["ukeys"].size]
    secs = _sections(good, len(elems), sizes)
    head_end = secs[1][0] + 8                                 # header + element table + tail
    for _ in range(n):
        b = bytearray(good)
        for _ in range(int(rng.integers(1, 4))):
            how = int(rng.integers(0, 5))
            if how == 0:                                      # a 32-bit field of the header / element table
                at = int(rng.integers(2, head_end // 4)) * 4
                b[at:at + 4] = int(_EXTREME[int(rng.integers(0, len(_EXTREME)))] & 0xFFFFFFFF).to_bytes(4, "little")
            elif how == 1:                                    # a 64-bit field of the element table
                at = 48 + int(rng.integers(0, (head_end - 48) // 8)) * 8
                b[at:at + 8] = int(_EXTREME[int(rng.integers(0, len(_EXTREME)))]).to_bytes(8, "little")
            elif how == 2:                                    # a 32-bit word anywhere (positions, offsets, slots, keys)
                at = int(rng.integers(12, len(b) // 4)) * 4
                b[at:at + 4] = int(_EXTREME[int(rng.integers(0, len(_EXTREME)))] & 0xFFFFFFFF).to_bytes(4, "little")
            elif how == 3:                                    # one bit anywhere
                at = int(rng.integers(8, len(b)))
                b[at] ^= 1 << int(rng.integers(0, 8))
            else:                                             # a small change of a small field (k, table kind, counts +- 1)
                at = 48 + int(rng.integers(0, (head_end - 48) // 4)) * 4
                v = (int.from_bytes(b[at:at + 4], "little") + int(rng.integers(-2, 3))) & 0xFFFFFFFF
                b[at:at + 4] = v.to_bytes(4, "little")
        mx = iw.Mixer()
        for at, ln in secs:
            mx.add(bytes(b[at:at + ln]))
        b[40:48] = mx.h.to_bytes(8, "little")
        cut = int(rng.integers(0, 8))
        if cut == 0:
            b = b[:int(rng.integers(0, len(b)))]
        elif cut == 1:
            b += bytes(int(rng.integers(1, 64)))
        yield bytes(b)
