"""The contract of kmx_placements_mapq in executable form, on the host arrays of a placements handle (strand, dist, second) and, for
paired reads, of a pairs handle (cls, score, second_score).  All arithmetic in Python integers.

q(d, s, B) = min(cap, per_edit * max(0, s' - d)) with s' = B + 1 when s is "none", else s.  An unplaced read (strand == 255) gets 0.
Otherwise q_se = q(dist[i], second[i], E), where 255 means none.  Without pairs, or when cls[i // 2] != CONCORDANT, mapq[i] = q_se;
for a concordant pair p, q_pe = q(score[p], second_score[p], 2 E), where 0xFFFF means none, and
mapq[i] = min(cap, max(q_se, min(q_pe, q_se + pair_bonus))).

n_zero counts the placed reads with mapq 0, n_cap the reads with mapq == cap.

mapq() returns (mapq[nr] u8, {"nr", "n_zero", "n_cap"})."""
import numpy as np

UNPLACED_STRAND, NONE8, NONE16, CONCORDANT = 255, 255, 0xFFFF, 1
DEFAULTS = dict(cap=60, per_edit=10, pair_bonus=40)


def q(d, s, none, budget, cap, per_edit):
    s1 = budget + 1 if s == none else s
    return min(cap, per_edit * max(0, s1 - d))


def mapq(strand, dist, second, max_edits, cap=60, per_edit=10, pair_bonus=40, cls=None, score=None, second_score=None):
    out = np.zeros(len(strand), np.uint8)
    n_zero = n_cap = 0
    for i in range(len(strand)):
        placed = int(strand[i]) != UNPLACED_STRAND
        v = 0
        if placed:
            v = q(int(dist[i]), int(second[i]), NONE8, max_edits, cap, per_edit)
            if cls is not None and int(cls[i // 2]) == CONCORDANT:
                q_pe = q(int(score[i // 2]), int(second_score[i // 2]), NONE16, 2 * max_edits, cap, per_edit)
                v = min(cap, max(v, min(q_pe, v + pair_bonus)))
        out[i] = v
        n_zero += placed and v == 0
        n_cap += v == cap
    return out, dict(nr=len(strand), n_zero=int(n_zero), n_cap=int(n_cap))
