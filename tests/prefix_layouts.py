"""DNA4 texts in which chosen sub-k queries have an exact slice length, number of runs, run lengths and interleaving (pure numpy).

A query shorter than k is answered by merging the position lists ("runs") of the k-mers that start with it.  Which merger takes
a slice depends on len (its positions, without those of the text's last k-mer) and R (its runs); how hard the merge is depends
on how the runs interleave.  The texts here are planted so that all of that is chosen, not met by chance:

  * the background is random letters from {1, 2, 3}; letter 0 occurs only as the first letter of a planted occurrence;
  * slice j has the query 0 . code(j), code(j) = j in base 3 over {1, 2, 3}, M - 1 letters;
  * each occurrence is followed by one of R distinct suffixes of K - M letters over {1, 2, 3}: on an index with an OPEN table
    and no prefix levels these are the slice's R runs, in ascending order of the suffix (a DENSE table counts its 4^(K-M) keys,
    the empty ones too);
  * occurrences sit on slots K letters apart; which slot gets which run is the interleaving;
  * no plant touches the text's last K letters, except the tail occurrence a case asks for: the query followed by fewer than
    K - M letters ends the text — one position that starts no k-mer, counted in cnt but not in len.

The expected hit list of a slice is the sorted list of its plants (+ the tail position): the reference, independent of the oracle.

classify() restates the dispatcher's conditions and bands_fit() the arithmetic of k_prefix_bands.  The thresholds are the
kernels' macros as they stand, written down here beside where they come from: a changed macro makes the class assertions of
the tests fail, not the cases silently move.

Out of scope — the slices would be too large for tests of seconds: S_room > KMX_BAND_MAX (len above 512 * 6144 = 3.1 M: too
many bands, the chunks take the slice) and S2 > KMX_SPLIT_MAX (len above 1024 * 16384 = 16.7 M: too many bands to spread by value).
"""
import numpy as np

SIGMA = 4
K = 12
M = 6
N_QUERIES = 3 ** (M - 1)          # 243 slices per text at most
N_SUFFIXES = 3 ** (K - M)         # 729 runs per slice at most

# kmer_index_amd/csrc/kmx_kernels.hip:42-44, kmx_types.h:114-142
PSORT_PAIR_CAP = 512              # KMX_PSORT_PAIR_CAP (= KMX_PMERGE_REG_LEN, kmx_types.h:124)
PMERGE_REG_RUNS = 4               # KMX_PMERGE_REG_RUNS (= KMX_PSORT_MULTIWAY_RUNS, kmx_kernels.hip:44)
PMERGE_MIN_AVG = 8                # KMX_PMERGE_MIN_AVG, kmx_types.h:115
PSORT_MAX_RUNS = 32               # KMX_PSORT_MAX_RUNS, kmx_types.h:136
PSORT_CAP = 2048                  # KMX_PSORT_CAP, kmx_types.h:137
PSORT_MID_CAP = 8192              # KMX_PSORT_MID_CAP, kmx_types.h:142
PSORT_BLOCK_CAP = 32768           # KMX_PSORT_BLOCK_CAP, kmx_types.h:140
PM_TILE = 4096                    # KMX_PM_TILE, kmx_kernels.hip:49
# kmx_kernels.hip:4502-4506, :4710-4717
SPLIT = 16384                     # KMX_SPLIT
SPLIT_MAX = 1024                  # KMX_SPLIT_MAX
SPLIT_TILE = 8192                 # KMX_SPLIT_TILE
BAND_FULL = 7168                  # KMX_BAND_FULL
BAND = 6144                       # KMX_BAND
BAND_RUNS = 64                    # KMX_BAND_RUNS
BAND_MAX = 512                    # KMX_BAND_MAX
# kmx_types.h:148-163
SMALL_NQ = 256                    # KMX_SMALL_NQ
SMALL_BLOCKS = 32                 # KMX_SMALL_BLOCKS: batches beyond 32 * 256 queries never take the latency path
SMALL_WCAP = 1024                 # KMX_SMALL_WCAP
SMALL_WSLOW = 32                  # KMX_SMALL_WSLOW
SMALL_SORT = 4096                 # KMX_SMALL_SORT
SMALL_BSLOW = 8                   # KMX_SMALL_BSLOW
SMALL_POS = 49152                 # KMX_SMALL_POS

CLASSES = ("plain", "small", "merge_small", "mid", "one_chunk", "banded", "split", "chunked")
INTERLEAVINGS = ("below", "above", "round_robin", "random", "giant_singles_before", "giant_singles_behind", "giant_singles_spread")


def classify(length, runs, bands_fit=None):
    """The merger the dispatcher gives a slice of `length` positions in `runs` runs (k_lookup, kmx_kernels.hip:692-707;
    k_prefix_bands, :4779-4783, :4829-4845).  bands_fit: bands_fit()'s verdict, needed beyond one chunk at up to 64 runs."""
    if runs < 2 or length < 2:
        return "plain"
    if length <= PSORT_CAP:
        merge = (2 <= runs <= PSORT_MAX_RUNS and not (runs <= PMERGE_REG_RUNS and length <= PSORT_PAIR_CAP)
                 and length >= PMERGE_MIN_AVG * runs)
        return "merge_small" if merge else "small"
    if length <= PSORT_MID_CAP:
        return "mid"
    if length <= PSORT_BLOCK_CAP:
        return "one_chunk"
    s_room = -(-length // BAND)
    if runs <= BAND_RUNS and s_room <= BAND_MAX:
        assert bands_fit is not None
        return "banded" if bands_fit else "chunked"
    if runs > BAND_RUNS and -(-length // SPLIT) <= SPLIT_MAX:
        return "split"
    return "chunked"


def band_sizes(positions, n_text, target):
    """Positions per value band of k_prefix_bands at `target` positions a band: band s of S = ceil(len / target) holds the
    positions in [floor(s n / S), floor((s + 1) n / S))."""
    length = positions.size
    S = -(-length // target)
    thr = (np.arange(S + 1, dtype=np.int64) * n_text) // S
    below = np.searchsorted(positions, thr[1:S], side="left")          # positions < threshold s, s = 1 .. S - 1
    return np.diff(np.concatenate([[0], below, [length]]))


def bands_fit(positions, n_text):
    """k_prefix_bands cuts the slice when every band holds at most KMX_PSORT_MID_CAP positions at KMX_BAND_FULL, or else at KMX_BAND."""
    return any(int(band_sizes(positions, n_text, t).max()) <= PSORT_MID_CAP for t in (BAND_FULL, BAND))


def code_letters(j, width):
    out = np.zeros(width, np.uint8)
    for i in range(width - 1, -1, -1):
        out[i] = 1 + j % 3
        j //= 3
    assert j == 0
    return out


def run_lengths(length, runs, inter, rng):
    """Run lengths for an interleaving: one giant run (in the middle of the key order) + single positions, or uneven random ones."""
    if inter.startswith("giant"):
        lens = np.ones(runs, np.int64)
        lens[runs // 2] = length - (runs - 1)
        return lens
    if runs == 1:
        return np.array([length], np.int64)
    return 1 + rng.multinomial(length - runs, np.full(runs, 1.0 / runs)).astype(np.int64)


def run_of_slot(lens, inter, rng):
    """run_of[i] = the run (index in ascending key order) whose occurrence sits on the slice's i-th position in text order."""
    R, length = lens.size, int(lens.sum())
    if inter == "below":                                  # run r wholly below run r + 1
        return np.repeat(np.arange(R), lens)
    if inter == "above":                                  # run r wholly above run r + 1
        return np.repeat(np.arange(R)[::-1], lens[::-1])
    if inter == "round_robin":                            # element by element, while a run has positions left
        rounds = np.concatenate([np.arange(l) for l in lens])
        runs = np.repeat(np.arange(R), lens)
        return runs[np.lexsort((runs, rounds))]
    if inter == "random":
        return rng.permutation(np.repeat(np.arange(R), lens))
    g = R // 2
    singles = np.array([r for r in range(R) if r != g], np.int64)
    out = np.full(length, g, np.int64)
    if inter == "giant_singles_before":
        out[:R - 1] = rng.permutation(singles)
    elif inter == "giant_singles_behind":
        out[length - (R - 1):] = rng.permutation(singles)
    elif inter == "giant_singles_spread":
        at = ((np.arange(R - 1) * 2 + 1) * length) // (2 * (R - 1))
        assert np.unique(at).size == R - 1
        out[at] = rng.permutation(singles)
    else:
        raise ValueError(inter)
    return out


class Spec:
    """One slice to plant.  parts: None = spread evenly over the whole text, or [(count, lo, hi), ...] with letter positions as
    fractions (num, den) of the text length — `count` occurrences spread evenly over the free slots in [lo, hi)."""

    def __init__(self, name, length, runs, inter="random", parts=None, tail=False):
        assert runs <= min(length, N_SUFFIXES) and (parts is None or sum(p[0] for p in parts) == length)
        self.name, self.length, self.runs, self.inter, self.parts, self.tail = name, length, runs, inter, parts, tail


class Slice:
    def __init__(self, spec, j, query, positions, lens, tail_pos, n_text):
        self.name, self.inter, self.j, self.query = spec.name, spec.inter, j, query
        self.length, self.runs, self.run_lens = int(positions.size), int(lens.size), lens
        self.tail_pos = tail_pos
        self.cnt = self.length + (tail_pos is not None)
        self.expected = np.concatenate([positions, [tail_pos] if tail_pos is not None else []]).astype(np.uint32)
        fit = bands_fit(positions, n_text) if self.length > PSORT_BLOCK_CAP and self.runs <= BAND_RUNS else None
        self.cls = classify(self.length, self.runs, fit)

    def __repr__(self):
        return f"{self.name}[{self.inter}] len={self.length} R={self.runs} cnt={self.cnt} -> {self.cls}"


class Layout:
    def __init__(self, text, slices):
        self.text, self.slices, self.n = text, slices, text.size
        self.by_name = {s.name: s for s in slices}

    def fillers(self, count):
        """Exact k-mers that do not occur: they begin with two 0s, and the text never holds two 0s side by side."""
        out = []
        for i in range(count):
            q = np.zeros(K, np.uint8)
            for t in range(K - 1, 1, -1):
                q[t] = i % 4
                i //= 4
            out.append(q)
        return out

    def batch(self, names=None, fillers=0):
        """(qranks, qoff, slices): the named slices' queries (all by default), `fillers` absent k-mers behind them."""
        sl = self.slices if names is None else [self.by_name[n] for n in names]
        qs = [s.query for s in sl] + self.fillers(fillers)
        qoff = np.zeros(len(qs) + 1, np.uint64)
        qoff[1:] = np.cumsum([q.size for q in qs])
        return np.concatenate(qs).astype(np.uint8), qoff, sl

    def class_counts(self, sl):
        return {c: sum(s.cls == c for s in sl) for c in CLASSES}


def plant(specs, n_body, seed):
    """The text (n_body letters, + the tail occurrence when a spec asks for one) and its slices."""
    assert len(specs) <= N_QUERIES and sum(s.tail for s in specs) <= 1
    rng = np.random.default_rng(seed)
    tail_letters = 3                                       # letters behind the tail occurrence: fewer than K - M
    has_tail = any(s.tail for s in specs)
    n_text = n_body + (M + tail_letters if has_tail else 0)
    n_slots = (n_body - K) // K                            # slot s = letters [s K, s K + K): none touches the last K letters
    owner = np.full(n_slots, -1, np.int64)

    def take(count, lo_pos, hi_pos, j):
        s_lo, s_hi = -(-lo_pos // K), min(n_slots, -(-hi_pos // K))        # slots whose position lies in [lo_pos, hi_pos)
        free = s_lo + np.nonzero(owner[s_lo:s_hi] < 0)[0]
        assert free.size >= count, (specs[j].name, int(free.size), count)
        owner[free[((2 * np.arange(count) + 1) * free.size) // (2 * count)]] = j

    for j, sp in sorted(enumerate(specs), key=lambda t: -t[1].length):     # the clustered ones first, the longest before the others
        if sp.parts is not None:
            for count, lo, hi in sp.parts:
                take(count, lo[0] * n_text // lo[1], hi[0] * n_text // hi[1], j)
    even = [j for j, sp in enumerate(specs) if sp.parts is None]
    if even:
        # every slice evenly over the free slots: the ideal places (i + 1/2) / len of all of them, merged, in rank order
        key = np.concatenate([(np.arange(specs[j].length) + 0.5) / specs[j].length for j in even])
        who = np.concatenate([np.full(specs[j].length, j) for j in even])
        who = who[np.argsort(key, kind="stable")]
        free = np.nonzero(owner < 0)[0]
        assert free.size >= who.size, (int(free.size), int(who.size))
        owner[free[(np.arange(who.size) * free.size) // who.size]] = who

    text = rng.integers(1, 4, n_text).astype(np.uint8)
    slices = []
    for j, sp in enumerate(specs):
        slots = np.nonzero(owner == j)[0]
        assert slots.size == sp.length
        positions = slots * K
        lens = run_lengths(sp.length, sp.runs, sp.inter, rng)
        suffixes = np.sort(rng.choice(N_SUFFIXES, sp.runs, replace=False))
        run_of = run_of_slot(lens, sp.inter, rng)
        query = np.concatenate([[0], code_letters(j, M - 1)]).astype(np.uint8)
        suffix_letters = np.stack([code_letters(int(s), K - M) for s in suffixes])
        block = np.concatenate([np.tile(query, (sp.length, 1)), suffix_letters[run_of]], axis=1)
        text[(positions[:, None] + np.arange(K)[None, :]).ravel()] = block.ravel()
        tail_pos = None
        if sp.tail:
            tail_pos = n_body
            text[n_body:n_body + M] = query
        slices.append(Slice(sp, j, query, positions, lens, tail_pos, n_text))
    return Layout(np.ascontiguousarray(text), slices)


def scan(layout):
    """What the text itself holds, by a numpy k-mer scan (not the plant table): for every slice (len, run lengths in
    ascending k-mer order, positions that start a k-mer, positions in the last K - 1 letters)."""
    text, n = layout.text, layout.n
    at = np.nonzero(text == 0)[0]
    at = at[at <= n - M]
    mcode = np.zeros(at.size, np.int64)
    for t in range(M):
        mcode = mcode * SIGMA + text[at + t]
    body = at <= n - K
    kcode = np.zeros(at.size, np.int64)
    for t in range(K):
        kcode = kcode * SIGMA + text[np.minimum(at + t, n - 1)]
    out = []
    for s in layout.slices:
        qc = 0
        for letter in s.query:
            qc = qc * SIGMA + int(letter)
        hit = mcode == qc
        pos, tails = at[hit & body], at[hit & ~body]
        _, lens = np.unique(kcode[hit & body], return_counts=True)
        out.append((int(pos.size), lens.astype(np.int64), pos, tails))
    return out


# ---------------------------------------------------------------------------------------------------------------------
# The cases.  (name, len, R); every one comes once per interleaving its shape allows (a giant run + singles needs len > R).
BOUNDARY_CASES = (
    [(f"len{l}_R{r}", l, r) for l in (512, 513) for r in (2, 4)]                    # register pair merge | multi-way rank / merge small
    + [(f"len{l}_R{r}", l, r) for l in (2048, 2049) for r in (2, 5, 33)]            # one wave | mid block
    + [(f"len{l}_R{r}", l, r) for l in (8192, 8193) for r in (2, 64)]               # mid block | one big chunk
    + [(f"len{l}_R{r}", l, r) for l in (32768, 32769) for r in (2, 64, 65)]         # one chunk | bands (R <= 64), split (R = 65)
    + [("len513_R5", 513, 5), ("len2048_R4", 2048, 4)]                              # R = 4 | 5 at 513 and at 2048 (with the rows above)
    + [("len2048_R32", 2048, 32)]                                                   # R = 32 | 33 at 2048
    + [(f"len{l}_R{r}", l, r) for r in (5, 32) for l in (8 * r - 1, 8 * r)]         # len = 8 R - 1 | 8 R: bitonic in a wave | merge small
)
BOUNDARY_EXPECT = {
    "len512_R2": "small", "len512_R4": "small", "len513_R2": "merge_small", "len513_R4": "merge_small", "len513_R5": "merge_small",
    "len2048_R2": "merge_small", "len2048_R4": "merge_small", "len2048_R5": "merge_small", "len2048_R32": "merge_small", "len2048_R33": "small",
    "len2049_R2": "mid", "len2049_R5": "mid", "len2049_R33": "mid", "len8192_R2": "mid", "len8192_R64": "mid",
    "len8193_R2": "one_chunk", "len8193_R64": "one_chunk", "len32768_R2": "one_chunk", "len32768_R64": "one_chunk", "len32768_R65": "one_chunk",
    "len32769_R2": "banded", "len32769_R64": "banded", "len32769_R65": "split",
    "len39_R5": "small", "len40_R5": "merge_small", "len255_R32": "small", "len256_R32": "merge_small",
}
BOUNDARY_BODY = 3_600_000


def boundary_layout(inter):
    """Every (len, R) boundary of the dispatcher in one text, all slices interleaved the same way and spread evenly."""
    specs = [Spec(name, l, r, inter) for name, l, r in BOUNDARY_CASES]
    return plant(specs, BOUNDARY_BODY, seed=1000 + INTERLEAVINGS.index(inter))


BANDS_BODY = 4_800_000
BANDS_EXPECT = {"band_of_8192": "banded", "band_of_8193": "chunked", "half_8192": "one_chunk", "half_8193": "one_chunk",
                "first_tenth": "chunked", "empty_first_fifth": "banded"}


def bands_layout():
    """Slices on the edge of what k_prefix_bands cuts.  5 * 7168 positions make five bands at KMX_BAND_FULL; the second one,
    [n / 5, 2 n / 5), holds exactly KMX_PSORT_MID_CAP = 8192 of them (all below n / 3) — or 8193, which fits neither there nor in
    [n / 6, n / 3) of the six bands at KMX_BAND, so the chunks take the slice.  half_8192 / half_8193: 2 * 8192 positions in two
    runs with exactly 8192 (8193) below n / 2 — a slice of one chunk as the macros stand (bands start beyond KMX_PSORT_BLOCK_CAP):
    k_prefix_merge_block takes both, with its merge-path cut on the middle of the text.  first_tenth: 32769 positions of 64 runs in the first tenth of the text (a band
    overflows); empty_first_fifth: no occurrence in the first fifth (its first bands are empty)."""
    full = 5 * BAND_FULL
    fifth = [((i, 5), (i + 1, 5)) for i in range(5)]

    def five_bands(second):
        rest = full - second
        share = [rest // 4 + (i < rest % 4) for i in range(4)]
        return [(share[0],) + fifth[0], (second, (1, 5), (1, 3))] + [(share[i - 1],) + fifth[i] for i in (2, 3, 4)]

    specs = [Spec("band_of_8192", full, 16, "random", five_bands(PSORT_MID_CAP)),
             Spec("band_of_8193", full, 16, "random", five_bands(PSORT_MID_CAP + 1)),
             Spec("half_8192", 2 * 8192, 2, "random", [(8192, (0, 1), (1, 2)), (8192, (1, 2), (1, 1))]),
             Spec("half_8193", 2 * 8192, 2, "random", [(8193, (0, 1), (1, 2)), (8191, (1, 2), (1, 1))]),
             Spec("first_tenth", 32769, 64, "random", [(32769, (0, 1), (1, 10))]),
             Spec("empty_first_fifth", 36000, 16, "round_robin", [(36000, (1, 5), (1, 1))])]
    return plant(specs, BANDS_BODY, seed=2001)


SPLIT_BODY = 2_600_000
SPLIT_LONG = 2 * SPLIT * 2 + 5                            # just over 2 * 16384 * 2: five bands of the spread, nine tiles of 8192


def split_layout():
    """More than 64 runs beyond one chunk: spread by value (k_prefix_split_*), spread evenly over the text."""
    specs = [Spec(f"split_len{l}_R{r}", l, r, inter)
             for l in (PSORT_BLOCK_CAP + 1, SPLIT_LONG) for r, inter in ((65, "round_robin"), (700, "random"))]
    return plant(specs, SPLIT_BODY, seed=3001)


PASSES_BODY = 3_100_000
PASSES_LENS = (2 * PSORT_BLOCK_CAP, 2 * PSORT_BLOCK_CAP + 1, 3 * PSORT_BLOCK_CAP + PM_TILE + 1)


def passes_layout():
    """Chunks + merge passes: two full chunks, two and one position, three and a partial chunk whose last tile of 4096 is partial
    (two passes).  At most 64 runs, so the split declines them; each slice fills a stretch of the text slot by slot, so that a
    value band holds far more than 8192 positions and the bands decline them too."""
    specs, lo = [], 0
    n_text = PASSES_BODY
    for l, r, inter in zip(PASSES_LENS, (2, 64, 33), ("round_robin", "random", "above")):
        hi = lo + (l + 8) * K
        specs.append(Spec(f"passes_len{l}_R{r}", l, r, inter, [(l, (lo, n_text), (hi, n_text))]))
        lo = hi
    return plant(specs, PASSES_BODY, seed=4001)


TAIL_CASES = {512: (4, "small"), 2048: (5, "merge_small"), 8192: (64, "mid")}


def tail_layout(T):
    """A slice of len = T exactly whose query also ends the text: cnt = T + 1, on the other side of the threshold T."""
    runs, _ = TAIL_CASES[T]
    specs = [Spec(f"tail_len{T}", T, runs, "random", tail=True), Spec("beside", 100, 3, "round_robin")]
    return plant(specs, (T + 200) * K * 2, seed=5000 + T)


LATENCY_BODY = 1_400_000


def latency_layout():
    """Slices for the limits of k_small (kmx_kernels.hip:2277-2292, :2348): wave-sized slow queries (several runs, up to 1024
    positions), block-sized ones (up to 4096), and plain ones (one run: not slow) to move the hit total by one."""
    specs = [Spec("b4097", 4097, 5, "random"), Spec("one", 1, 1, "below"), Spec("two", 2, 1, "below")]
    specs += [Spec(f"w1024_{i}", 1024, 2 + i % 3, INTERLEAVINGS[i % 4]) for i in range(16)]
    specs += [Spec(f"b1025_{i}", 1025, 2 + i % 3, INTERLEAVINGS[i % 4]) for i in range(9)]
    specs += [Spec(f"b4096_{i}", 4096, 2 + i, INTERLEAVINGS[i % 4]) for i in range(8)]
    specs += [Spec(f"b2000_{i}", 2000, 3, INTERLEAVINGS[i % 4]) for i in range(9)]
    specs += [Spec(f"w40_{i}", 40, 2, INTERLEAVINGS[i % 7]) for i in range(33)]
    return plant(specs, LATENCY_BODY, seed=6001)


# (name, slices of the batch, does k_small answer).  One workgroup takes a batch of up to 256 queries; it declines when a slice
# holds more than KMX_SMALL_SORT positions, when more than KMX_SMALL_WSLOW slices of up to KMX_SMALL_WCAP positions or more than
# KMX_SMALL_BSLOW bigger ones want merging, or when the hit total exceeds KMX_SMALL_POS.  A single slice of 1025 positions is a
# block-sized one and still answered; nine of them are declined where nine of 1024 are not: there one position decides.
LATENCY_BATCHES = [
    ("one_of_1024", ["w1024_0"], True), ("one_of_1025", ["b1025_0"], True),
    ("nine_of_1024", [f"w1024_{i}" for i in range(9)], True), ("nine_of_1025", [f"b1025_{i}" for i in range(9)], False),
    ("one_of_4096", ["b4096_0"], True), ("one_of_4097", ["b4097"], False),
    ("wave_sized_32", [f"w40_{i}" for i in range(32)], True), ("wave_sized_33", [f"w40_{i}" for i in range(33)], False),
    ("block_sized_8", [f"b2000_{i}" for i in range(8)], True), ("block_sized_9", [f"b2000_{i}" for i in range(9)], False),
    ("total_49152", [f"b4096_{i}" for i in range(8)] + [f"w1024_{i}" for i in range(16)], True),
    ("total_49153", [f"b4096_{i}" for i in range(8)] + [f"w1024_{i}" for i in range(16)] + ["one"], False),
]


def small_answers(sl):
    """Whether k_small answers a batch of these slices alone (one workgroup): its conditions, restated."""
    slow = [s.length for s in sl if s.runs > 1 and s.length > 1]
    return (len(sl) <= SMALL_NQ and all(l <= SMALL_SORT for l in slow) and sum(l <= SMALL_WCAP for l in slow) <= SMALL_WSLOW
            and sum(l > SMALL_WCAP for l in slow) <= SMALL_BSLOW and sum(s.cnt for s in sl) <= SMALL_POS)


def all_layouts():
    """(id, builder, expected classes by slice name — None: whatever classify() says, plain and small sizes)."""
    out = [(f"boundary-{inter}", (lambda i=inter: boundary_layout(i)), BOUNDARY_EXPECT) for inter in INTERLEAVINGS]
    out += [("bands", bands_layout, BANDS_EXPECT), ("split", split_layout, {f"split_len{l}_R{r}": "split" for l in (32769, SPLIT_LONG) for r in (65, 700)}),
            ("passes", passes_layout, {f"passes_len{l}_R{r}": "chunked" for l, r in zip(PASSES_LENS, (2, 64, 33))})]
    out += [(f"tail-{T}", (lambda t=T: tail_layout(t)), {f"tail_len{T}": TAIL_CASES[T][1], "beside": "small"}) for T in TAIL_CASES]
    out += [("latency", latency_layout, None)]
    return out
