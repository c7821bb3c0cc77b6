"""Portable synthetic inputs: counter-based SplitMix64 -> multiply-shift ranks.

The reference's generator (benchmarks/input_generator.hpp:52-63) draws i.i.d. uniform ranks
from std::mt19937 + std::uniform_int_distribution<uint8_t>, whose output is implementation
defined; this generator keeps the distribution (i.i.d. uniform over [0, sigma)) and is
identical on every host.  Item i of stream `seed` is rank(mix64(seed + (i+1)*GOLDEN)).
"""
import numpy as np

GOLDEN = np.uint64(0x9E3779B97F4A7C15)
_M1 = np.uint64(0xBF58476D1CE4E5B9)
_M2 = np.uint64(0x94D049BB133111EB)


def mix64(z: np.ndarray) -> np.ndarray:
    z = z.astype(np.uint64, copy=True)
    z ^= z >> np.uint64(30)
    z *= _M1
    z ^= z >> np.uint64(27)
    z *= _M2
    z ^= z >> np.uint64(31)
    return z


def u64_stream(seed: int, n: int, start: int = 0) -> np.ndarray:
    with np.errstate(over="ignore"):
        i = np.arange(start + 1, start + n + 1, dtype=np.uint64)
        return mix64(np.uint64(seed) + i * GOLDEN)


def ranks(seed: int, n: int, sigma: int, chunk: int = 1 << 24) -> np.ndarray:
    """n i.i.d. uniform ranks in [0, sigma) as uint8."""
    out = np.empty(n, np.uint8)
    for s in range(0, n, chunk):
        m = min(chunk, n - s)
        z = u64_stream(seed, m, s)
        out[s:s + m] = (((z >> np.uint64(32)) * np.uint64(sigma)) >> np.uint64(32)).astype(np.uint8)
    return out


def uniform_queries(seed: int, nq: int, m: int, sigma: int):
    """nq queries of length m: (qranks[nq*m] u8, qoff[nq+1] u64)."""
    q = ranks(seed, nq * m, sigma)
    off = np.arange(nq + 1, dtype=np.uint64) * np.uint64(m)
    return q, off


def mixed_queries(seed: int, text: np.ndarray, nq: int, lengths, sigma: int, planted_frac: float = 0.5):
    """Queries with lengths drawn uniformly from `lengths`; a `planted_frac` share is copied from
    the text at a uniform offset (guaranteed hit), the rest are uniform random (cfg 3/5)."""
    lengths = np.asarray(lengths, np.uint64)
    z = u64_stream(seed, nq)
    lens = lengths[((z >> np.uint64(40)) % np.uint64(lengths.size)).astype(np.int64)]
    off = np.zeros(nq + 1, np.uint64)
    np.cumsum(lens, out=off[1:])
    total = int(off[-1])
    q = ranks(seed ^ 0x5DEECE66D, total, sigma)
    z2 = u64_stream(seed + 17, nq)
    planted = (z2 & np.uint64(0xFFFF)).astype(np.float64) < planted_frac * 65536.0
    n = text.size
    idx = np.nonzero(planted)[0]
    if idx.size:
        maxstart = (np.uint64(n) - lens[idx]).astype(np.uint64)
        start = ((z2[idx] >> np.uint64(16)) % (maxstart + np.uint64(1))).astype(np.int64)
        # vectorised ragged copy
        l = lens[idx].astype(np.int64)
        tot = int(l.sum())
        rep = np.repeat(np.arange(idx.size), l)
        within = np.arange(tot) - np.repeat(np.cumsum(l) - l, l)
        dst = off[idx].astype(np.int64)[rep] + within
        src = start[rep] + within
        q[dst] = text[src]
    return q, off


def planted_reads(seed: int, text: np.ndarray, nq: int, m: int, sigma: int, max_subst: int):
    """nq reads of m letters copied from the text at seeded offsets, each with a seeded number (0 .. max_subst) of
    substitutions at distinct letters — one in each of the first d of max_subst equal segments of the read — each to a
    different letter: (qranks[nq*m] u8, qoff[nq+1] u64)."""
    n = text.size
    if m > n:
        raise ValueError("planted_reads: m > text length")
    if max_subst > 0 and m < max_subst:
        raise ValueError("planted_reads: m < max_subst (a read cannot hold max_subst substitutions)")
    if max_subst > 0 and sigma < 2:
        raise ValueError("planted_reads: substitutions need sigma >= 2")
    z = u64_stream(seed, nq)
    start = (z % np.uint64(n - m + 1)).astype(np.int64)
    rows = start[:, None] + np.arange(m, dtype=np.int64)[None, :]
    q = text[rows].astype(np.uint8)
    if max_subst > 0:
        d = (u64_stream(seed + 1, nq) % np.uint64(max_subst + 1)).astype(np.int64)
        zz = u64_stream(seed + 2, nq * max_subst).reshape(nq, max_subst)
        seg = m // max_subst
        for k in range(max_subst):
            sel = np.nonzero(d > k)[0]
            if sel.size == 0:
                continue
            col = k * seg + (zz[sel, k] % np.uint64(seg)).astype(np.int64)
            shift = 1 + ((zz[sel, k] >> np.uint64(32)) % np.uint64(sigma - 1)).astype(np.int64)
            q[sel, col] = ((q[sel, col].astype(np.int64) + shift) % sigma).astype(np.uint8)
    off = np.arange(nq + 1, dtype=np.uint64) * np.uint64(m)
    return np.ascontiguousarray(q.reshape(-1)), off


def planted_reads_edit(seed: int, text: np.ndarray, nq: int, m: int, sigma: int, max_edits: int):
    """nq reads of m letters, each the first m letters of text[s, s + m + max_edits) after a seeded number (0 .. max_edits)
    of edits of seeded kinds (substitution to a different letter, deletion of a letter, insertion of a seeded letter), the
    k-th edit inside the k-th of max_edits equal segments of the read: the start s of every read is within that many edits
    of it.  (qranks[nq*m] u8, qoff[nq+1] u64, starts[nq] i64)"""
    n = text.size
    if m + max_edits > n:
        raise ValueError("planted_reads_edit: m + max_edits > text length")
    if max_edits > 0 and m < max_edits:
        raise ValueError("planted_reads_edit: m < max_edits (a read cannot hold max_edits edits)")
    if max_edits > 0 and sigma < 2:
        raise ValueError("planted_reads_edit: substitutions need sigma >= 2")
    z = u64_stream(seed, nq)
    start = (z % np.uint64(n - m - max_edits + 1)).astype(np.int64)
    width = m + max_edits + 1
    cols = np.arange(width, dtype=np.int64)[None, :]
    rows = np.minimum(start[:, None] + cols, n - 1)
    q = text[rows].astype(np.uint8)                      # (nq, width): the source and some slack for deletions
    if max_edits > 0:
        d = (u64_stream(seed + 1, nq) % np.uint64(max_edits + 1)).astype(np.int64)
        zz = u64_stream(seed + 2, nq * max_edits).reshape(nq, max_edits)
        seg = m // max_edits
        for k in range(max_edits):
            sel = np.nonzero(d > k)[0]
            if sel.size == 0:
                continue
            col = k * seg + (zz[sel, k] % np.uint64(seg)).astype(np.int64)
            kind = ((zz[sel, k] >> np.uint64(24)) % np.uint64(3)).astype(np.int64)       # 0 substitution, 1 deletion, 2 insertion
            shift = 1 + ((zz[sel, k] >> np.uint64(32)) % np.uint64(sigma - 1)).astype(np.int64)
            sub = q[sel]
            old = sub[np.arange(sel.size), col].astype(np.int64)
            # deletion: columns from col on take their right neighbour; insertion: columns behind col take their left one
            src = cols + ((kind[:, None] == 1) & (cols >= col[:, None])) - ((kind[:, None] == 2) & (cols > col[:, None]))
            sub = np.take_along_axis(sub, np.clip(src, 0, width - 1), axis=1)
            changed = kind != 1
            sub[np.nonzero(changed)[0], col[changed]] = ((old[changed] + shift[changed]) % sigma).astype(np.uint8)
            q[sel] = sub
    off = np.arange(nq + 1, dtype=np.uint64) * np.uint64(m)
    return np.ascontiguousarray(q[:, :m].reshape(-1)), off, start


def revcomp(qranks: np.ndarray, qoff: np.ndarray, complement: np.ndarray) -> np.ndarray:
    """Every query of the batch reverse-complemented in place of itself: rc(q)[i] = complement[q[m - 1 - i]] (same offsets)."""
    qranks = np.asarray(qranks, np.uint8)
    qoff = np.asarray(qoff, np.uint64).astype(np.int64)
    complement = np.asarray(complement, np.uint8)
    if qranks.size == 0:
        return qranks.copy()
    lens = np.diff(qoff)
    qi = np.repeat(np.arange(lens.size), lens)
    src = qoff[qi] + qoff[qi + 1] - 1 - np.arange(qranks.size, dtype=np.int64)
    return complement[qranks[src]]


def _flip_half(seed: int, q: np.ndarray, off: np.ndarray, complement: np.ndarray):
    """A seeded half of the reads replaced by their reverse complements: (qranks, strand[nq] u8)."""
    nq = off.size - 1
    strand = ((u64_stream(seed + 3, nq) >> np.uint64(17)) & np.uint64(1)).astype(np.uint8)
    rc = revcomp(q, off, complement)
    per_letter = np.repeat(strand, np.diff(off.astype(np.int64))).astype(bool)
    return np.where(per_letter, rc, q).astype(np.uint8), strand


def planted_reads_strands(seed: int, text: np.ndarray, nq: int, m: int, sigma: int, max_subst: int, complement: np.ndarray):
    """planted_reads with a seeded half of the reads reverse-complemented (as a sequencer reads the other strand): the
    reverse complement of read i lies within max_subst substitutions of text[start[i], start[i] + m) when strand[i] == 1,
    the read itself when strand[i] == 0.  (qranks[nq*m] u8, qoff[nq+1] u64, strand[nq] u8, start[nq] i64)"""
    q, off = planted_reads(seed, text, nq, m, sigma, max_subst)
    start = (u64_stream(seed, nq) % np.uint64(text.size - m + 1)).astype(np.int64)
    q, strand = _flip_half(seed, q, off, complement)
    return q, off, strand, start


def planted_reads_edit_strands(seed: int, text: np.ndarray, nq: int, m: int, sigma: int, max_edits: int, complement: np.ndarray):
    """planted_reads_edit with a seeded half of the reads reverse-complemented: start[i] is within max_edits edits of read i
    (strand[i] == 0) or of its reverse complement (strand[i] == 1).  (qranks, qoff, strand[nq] u8, start[nq] i64)"""
    q, off, start = planted_reads_edit(seed, text, nq, m, sigma, max_edits)
    q, strand = _flip_half(seed, q, off, complement)
    return q, off, strand, start
