"""Batches of exact-search queries whose hit lists put a chosen event on a chosen output slot (pure numpy).

k_fill cuts the concatenated hit lists of a batch into tiles of T = 256 * E output slots (E = 4, 8, 12 or 16), so what is a
boundary case for one variant is the middle of a tile for another.  The builder works from the text's own k-mer histogram
(computed here, without the engine or the oracle): the hit count of every query it emits is known, the running sum of the
counts is the slot the next query starts on, and filler queries of known size move that sum to wherever a layout wants it.
check_events() then verifies, against any hit_off array (the oracle's in the CPU test), that every event lies where it was
asked for.

Layouts (each takes the next free tile boundary b = t * T it can reach):
  bucket_starts_on_boundary      a bucket whose first slot is b
  bucket_ends_before_boundary    a bucket whose last slot is b - 1
  bucket_starts_on_last_slot     a bucket whose first slot is b - 1
  giant_covers_two_tiles         the bucket of the planted one-letter run, first slot b - 1: the tiles t and t + 1 hold no start
  dense_starts_and_empty_runs    150 buckets of 1 up to b, 300 absent k-mers, 300 buckets of 1 from b on, 300 absent k-mers, 50 of 1
  prefix_mid_on_boundary         a sub-k query (k - 1 letters, one tail position): its contiguous slice ends on b - 1, its tail is b
  prefix_mid_before_boundary     ... its slice ends on b - 2, its tail position is slot b - 1
  prefix_straddles               ... b lies in the middle of its slice
  prefix_runs_begin_on_last_slot a sub-k query of k - 3 letters (a slice of many runs, two tail positions), first slot b - 1
  prefix_runs_tails_straddle     ... its first tail position on b - 1, its second on b
  stitch_straddles               the 2k-mer of the one-letter run, first slot b - 5
  ("total", n)                   filler up to a total of exactly n hits (last layout of a list); n = None: up to a tile boundary
"""
import numpy as np

from kmer_index_amd import synth

SIGMA = 4
TILES = (1024, 2048, 3072, 4096)
EVENT_LAYOUTS = ["bucket_starts_on_boundary", "bucket_ends_before_boundary", "bucket_starts_on_last_slot", "giant_covers_two_tiles",
                 "dense_starts_and_empty_runs", "prefix_mid_on_boundary", "prefix_mid_before_boundary", "prefix_straddles",
                 "prefix_runs_begin_on_last_slot", "prefix_runs_tails_straddle"]
RUN_LETTERS = 9000


def make_text(seed=4242):
    """DNA4, about 60 000 letters: two stretches over {A, C, G} (729 6-mers, buckets of 30 to 110), between them a run of 9000 A
    (one bucket of about 9000 positions, more than two tiles of 4096), then 1500 letters over all four (k-mers with a T: a few
    hundred occur once or twice, thousands never), and an end "CACAC" so that the sub-k queries CACAC and CAC have tail positions."""
    body = synth.ranks(seed, 50_000, 3)
    rare = synth.ranks(seed + 1, 1500, 4)
    return np.ascontiguousarray(np.concatenate([body[:25_000], np.zeros(RUN_LETTERS, np.uint8), body[25_000:], rare,
                                                np.array([1, 0, 1, 0, 1], np.uint8)]))


def kmer_codes(text, k):
    """code[i] of the k-mer at i, first letter most significant, for i <= n - k."""
    n = text.size
    code = np.zeros(n - k + 1, np.int64)
    for j in range(k):
        code = code * SIGMA + text[j:n - k + 1 + j].astype(np.int64)
    return code


def decode(code, k):
    return np.array([(code >> (2 * (k - 1 - j))) & 3 for j in range(k)], np.uint8)


class Batch:
    def __init__(self, qs, counts, events, T, k):
        self.qs = qs
        self.k = k
        self.counts = np.asarray(counts, np.int64)             # expected hits per query, from the histogram
        self.events = events
        self.T = T
        self.qoff = np.zeros(len(qs) + 1, np.uint64)
        self.qoff[1:] = np.cumsum([len(q) for q in qs])
        self.qranks = np.concatenate(qs).astype(np.uint8)
        self.total = int(self.counts.sum())


class LayoutBuilder:
    def __init__(self, text, k):
        self.text, self.k, self.n = text, k, text.size
        self.hist = np.bincount(kmer_codes(text, k), minlength=SIGMA ** k)
        order = np.random.default_rng(99).permutation(SIGMA ** k)
        self.ones = [c for c in order if self.hist[c] == 1]
        self.twos = [c for c in order if self.hist[c] == 2]
        self.absent = [c for c in order if self.hist[c] == 0]
        self.medium = [c for c in order if 20 <= self.hist[c] <= 200]
        self.min_medium = min(self.hist[c] for c in self.medium)
        self.giant = int(np.argmax(self.hist))
        assert self.hist[self.giant] > 2 * 4096 and len(self.ones) >= 100 and len(self.twos) >= 50 and len(self.absent) >= 300
        # the sub-k queries: the last k - 1 letters of the text (one tail position) and the last k - 3 (two: the text ends XYXYX)
        self.p_long, self.p_runs = text[self.n - (k - 1):].copy(), text[self.n - (k - 3):].copy()

    def prefix_counts(self, q):
        """(positions of q that start a k-mer of the text, positions in the last k - 1 letters): slice length and tail count."""
        m = q.size
        win = np.ones(self.n - m + 1, bool)
        for j in range(m):
            win &= self.text[j:self.n - m + 1 + j] == q[j]
        at = np.nonzero(win)[0]
        return int((at <= self.n - self.k).sum()), int((at > self.n - self.k).sum())

    def build(self, T, layouts):
        k = self.k
        qs, counts, events = [], [], []
        cur = [0]
        rot = {"ones": 0, "twos": 0, "absent": 0, "medium": 0}

        def take(pool):
            lst = getattr(self, pool)
            c = lst[rot[pool] % len(lst)]
            rot[pool] += 1
            return int(c)

        def emit_code(c):
            qs.append(decode(c, k))
            counts.append(int(self.hist[c]))
            cur[0] += int(self.hist[c])
            return len(qs) - 1

        def emit_query(q, count):
            qs.append(np.asarray(q, np.uint8))
            counts.append(int(count))
            cur[0] += int(count)
            return len(qs) - 1

        def advance_to(slot):
            assert slot >= cur[0], (slot, cur[0])
            while cur[0] < slot:
                rem = slot - cur[0]
                if rem >= self.min_medium:
                    for _ in range(len(self.medium)):
                        c = take("medium")
                        if self.hist[c] <= rem:
                            emit_code(c)
                            break
                    else:
                        emit_code(take("ones"))
                elif rem >= 2:
                    emit_code(take("twos"))
                else:
                    emit_code(take("ones"))

        def boundary(lead):
            """The first tile boundary b = t * T with b - lead >= the current sum and t >= 1."""
            t = max(1, -(-(cur[0] + lead) // T))
            return t * T

        def medium_bucket():
            return take("medium")

        for lay in layouts:
            if isinstance(lay, tuple) and lay[0] == "total":
                for _ in range(3):
                    emit_code(take("absent"))
                total = boundary(T // 2) if lay[1] is None else int(lay[1])
                advance_to(total)
                for _ in range(3):
                    emit_code(take("absent"))
                events.append({"layout": "total", "total": total})
            elif lay == "bucket_starts_on_boundary":
                b = boundary(0)
                advance_to(b)
                events.append({"layout": lay, "q": emit_code(medium_bucket()), "first": b})
            elif lay == "bucket_ends_before_boundary":
                c = medium_bucket()
                b = boundary(int(self.hist[c]))
                advance_to(b - int(self.hist[c]))
                events.append({"layout": lay, "q": emit_code(c), "last": b - 1})
            elif lay == "bucket_starts_on_last_slot":
                b = boundary(1)
                advance_to(b - 1)
                events.append({"layout": lay, "q": emit_code(medium_bucket()), "first": b - 1})
            elif lay == "giant_covers_two_tiles":
                b = boundary(1)
                advance_to(b - 1)
                events.append({"layout": lay, "q": emit_code(self.giant), "first": b - 1, "empty_tiles": [b // T, b // T + 1]})
            elif lay == "dense_starts_and_empty_runs":
                b = boundary(150)
                advance_to(b - 150)
                for _ in range(150):
                    emit_code(take("ones"))
                e0 = len(qs)
                for _ in range(300):
                    emit_code(take("absent"))
                for _ in range(300):
                    emit_code(take("ones"))
                e1 = len(qs)
                for _ in range(300):
                    emit_code(take("absent"))
                for _ in range(50):
                    emit_code(take("ones"))
                events.append({"layout": lay, "tile": b // T, "empty_on_boundary": [e0, e0 + 300], "empty_inside": [e1, e1 + 300]})
            elif lay in ("prefix_mid_on_boundary", "prefix_mid_before_boundary", "prefix_straddles"):
                ln, tails = self.prefix_counts(self.p_long)
                assert ln >= 2 and tails == 1
                lead = {"prefix_mid_on_boundary": ln, "prefix_mid_before_boundary": ln + 1, "prefix_straddles": ln // 2}[lay]
                b = boundary(lead)
                advance_to(b - lead)
                events.append({"layout": lay, "q": emit_query(self.p_long, ln + tails), "first": b - lead, "mid": b - lead + ln, "tails": tails})
            elif lay in ("prefix_runs_begin_on_last_slot", "prefix_runs_tails_straddle"):
                ln, tails = self.prefix_counts(self.p_runs)
                assert ln >= 2 and tails == 2
                lead = 1 if lay == "prefix_runs_begin_on_last_slot" else ln + 1
                b = boundary(lead)
                advance_to(b - lead)
                events.append({"layout": lay, "q": emit_query(self.p_runs, ln + tails), "first": b - lead, "mid": b - lead + ln, "tails": tails})
            elif lay == "stitch_straddles":
                # the 2k-mer of the one-letter run: every start of the run's k-mer whose successor k letters on is the same k-mer
                letter = decode(self.giant, k)[0]
                q = np.full(2 * k, letter, np.uint8)
                b = boundary(5)
                advance_to(b - 5)
                events.append({"layout": lay, "q": emit_query(q, sum(self.prefix_counts(q))), "first": b - 5})
            else:
                raise ValueError(f"unknown layout {lay!r}")
        return Batch(qs, counts, events, T, k)


def check_events(batch, hit_off):
    """Every requested event lies where it was asked for, judged on hit_off alone (uint64[nq + 1])."""
    off = np.asarray(hit_off).astype(np.int64)
    T = batch.T
    assert off.size == len(batch.qs) + 1
    assert np.array_equal(np.diff(off), batch.counts), "the histogram's counts are not the hit counts"
    cnt = np.diff(off)
    seen = set()
    for ev in batch.events:
        lay = ev["layout"]
        seen.add(lay)
        if lay == "total":
            assert ev is batch.events[-1] and off[-1] == ev["total"] == batch.total, (int(off[-1]), ev["total"])
            continue
        if lay == "dense_starts_and_empty_runs":
            t = ev["tile"]
            starts = np.nonzero((off[:-1] >= t * T) & (off[:-1] < (t + 1) * T) & (cnt > 0))[0]
            assert starts.size > 256 and (cnt[starts] == 1).sum() > 256, (lay, starts.size)
            a, b = ev["empty_on_boundary"]
            assert b - a >= 300 and (cnt[a:b] == 0).all() and (off[a:b + 1] == t * T).all(), lay
            assert cnt[a - 1] == 1 and off[a] - 1 == t * T - 1 and cnt[b] == 1, lay      # a bucket ends on t*T - 1, the next starts on t*T
            a, b = ev["empty_inside"]
            assert b - a >= 300 and (cnt[a:b] == 0).all() and t * T < off[a] < (t + 1) * T, lay
            continue
        q = ev["q"]
        assert cnt[q] > 0, lay
        if "first" in ev:
            assert off[q] == ev["first"], (lay, int(off[q]), ev["first"])
        if "last" in ev:
            assert off[q + 1] - 1 == ev["last"] and (ev["last"] + 1) % T == 0, (lay, int(off[q + 1]), ev["last"])
        if lay == "bucket_starts_on_boundary":
            assert off[q] % T == 0 and off[q] > 0 and cnt[q] >= 2
        if lay in ("bucket_starts_on_last_slot", "giant_covers_two_tiles", "prefix_runs_begin_on_last_slot"):
            assert (off[q] + 1) % T == 0 and cnt[q] >= 2
        if lay == "giant_covers_two_tiles":
            for t in ev["empty_tiles"]:
                assert off[q] < t * T and off[q + 1] >= (t + 1) * T                       # the whole tile is this bucket's
                assert not ((off[:-1] >= t * T) & (off[:-1] < (t + 1) * T)).any()          # ... and no query starts in it
            assert len(ev["empty_tiles"]) >= 2
        if "mid" in ev:
            assert off[q + 1] - ev["mid"] == ev["tails"] and ev["mid"] - off[q] >= 2, lay
            if lay == "prefix_mid_on_boundary":
                assert ev["mid"] % T == 0
            if lay in ("prefix_mid_before_boundary", "prefix_runs_tails_straddle"):
                assert (ev["mid"] + 1) % T == 0
            if lay == "prefix_runs_tails_straddle":
                assert ev["tails"] == 2
            if lay == "prefix_straddles":
                assert off[q] // T < (ev["mid"] - 1) // T
        if lay == "stitch_straddles":
            assert off[q] // T < (off[q + 1] - 1) // T and len(batch.qs[q]) == 2 * batch.k
    return seen


def main_batch(lb, T):
    """Every event layout in one batch (no STITCH query: a batch that holds one keeps the next batch on its handle from
    filling speculatively), its total a whole number of tiles."""
    return lb.build(T, EVENT_LAYOUTS + [("total", None)])
