"""The views of every chain handle through the states of its lifecycle.  Table-driven over the _Handle subclasses of engine.py that
declare _view_of: ROWS says how a handle of each kind is filled from a Chain (the handles of one tiny batch, tests/chain_data.py:
tiny_pairs), how its call is refused after it has looked at the handle, and which C function that is; NULLS says, field by field,
when kmx_*_view_device hands out NULL, as include/kmx.h words it.  One handle of each kind is then
  1. filled by the batch (every field holds an entry at least),
  2. refilled by a quarter of the batch (the counts shrink, the device arrays stay where they are),
  3. refilled by three copies of the batch after its host view was taken (the page-locked arrays grow),
  4. refilled by the empty batch,
  5. refused after the call has looked at it (a mismatched upstream handle): it holds the empty result,
  6. refused before that (options NULL): it is as it was,
and in every state its counts(), the NULL pattern of device_ptrs(), the length of every array of host() and the bytes at every device
pointer against the host array are held against a handle of its own that the same batch has filled once.  kmx_windows_vote has no
refusal that looks at the loci handle (its refusals "after looking" look at the result): state 5 leaves a Loci as it was.
host() names its fields as _view_of declares them; a field that a class lists in _optional (ctg) is None there when the C view hands
out NULL for it: under the contig table of these tests only while it is empty, and always on an index without one (a test of its own).
ApproxResult is not a chain handle (no device view, no refill by a chain stage) and has no row."""
import collections
import contextlib
import ctypes as C

import numpy as np
import pytest

from tests.chain_checks import dev_array, differ, refused
from tests.chain_data import COMP4, K, LETTERS4, TINY_CHAIN, TINY_CONTIGS, TINY_E, TINY_INSERT, table_of, tiny_pairs, tiny_text
from tests.helpers import pack

pytestmark = pytest.mark.gpu

# when kmx_*_view_device hands out NULL for a field
LIVE = "NULL exactly when the field holds no element"
KEPT = "never NULL once a call has filled the handle"
FILLED = "an offset array: NULL exactly after a refusal or an error; the host view then holds the one offset 0"
NULLS = {
    "Loci": (KEPT, LIVE, LIVE, LIVE, KEPT),
    "Alignments": (LIVE, LIVE, LIVE, KEPT, KEPT),
    "Placements": (LIVE,) * 7,
    "Pairs": (LIVE,) * 4,
    "Rescues": (FILLED,) + (LIVE,) * 7,
    "Scripts": (FILLED, LIVE, FILLED, LIVE),
    "Clips": (LIVE,) * 7 + (FILLED, LIVE),
    "Md": (FILLED, LIVE),
    "Mapq": (LIVE,),
    "Located": (LIVE,) * 2,
    "Secondaries": (FILLED,) + (LIVE,) * 6,                    # (ctg: the index of these tests has a contig table)
    "Supplementaries": (FILLED,) + (LIVE,) * 12,
    "Pileup": (LIVE,),
    "Sites": (LIVE,) * 7,
}
GIVEN, REFUSED = "given", "refused"

# name: the attribute of a Chain; fill(c, h): the call that fills h from the handles of the Chain c; mismatch(c, o, h): that call with
# one upstream handle of the Chain o in the place of c's; fn: the C function both end in; keeps: a refusal leaves the handle as it was
Row = collections.namedtuple("Row", "name cls fn fill mismatch keeps", defaults=(False,))


def _fold(c, pl=None, pairs=None, al=None):
    e = c.engine
    return (al or c.al).fold_pairs(c.loci, **TINY_INSERT, stream=c.stream, placements=pl or c.keep(e.Placements()), pairs=pairs or c.keep(e.Pairs()))


def _rescue(c, h, reads=None):
    pl, pairs = _fold(c)
    return pairs.rescue(c.idx, reads or c.reads, c.loci, c.al, pl, **TINY_INSERT, max_edits=TINY_E, rescues=h)


ROWS = (
    Row("loci", "Loci", "kmx_windows_vote", lambda c, h: c.windows.vote(TINY_CHAIN["band"], TINY_CHAIN["min_votes"], loci=h),
        lambda c, o, h: o.plain.vote(TINY_CHAIN["band"], TINY_CHAIN["min_votes"], loci=h), True),
    Row("al", "Alignments", "kmx_loci_align_device",
        lambda c, h: c.loci.align_device(c.idx, c.d_ranks2, c.d_roff2, c.nr2, TINY_E, TINY_CHAIN["max_span"], stream=c.stream, alignments=h),
        lambda c, o, h: c.loci.align_device(c.idx, o.d_ranks2, o.d_roff2, o.nr2, TINY_E, TINY_CHAIN["max_span"], stream=c.stream, alignments=h)),
    Row("pl", "Placements", "kmx_alignments_fold_pairs", lambda c, h: _fold(c, pl=h), lambda c, o, h: _fold(c, pl=h, al=o.al)),
    Row("pairs", "Pairs", "kmx_alignments_fold_pairs", lambda c, h: _fold(c, pairs=h), lambda c, o, h: _fold(c, pairs=h, al=o.al)),
    Row("res", "Rescues", "kmx_pairs_rescue", _rescue, lambda c, o, h: _rescue(c, h, reads=o.reads)),
    Row("sc", "Scripts", "kmx_placements_scripts", lambda c, h: c.pl.scripts(c.idx, c.reads, c.loci, c.al, scripts=h),
        lambda c, o, h: c.pl.scripts(c.idx, c.reads, c.loci, o.al, scripts=h)),
    Row("cl", "Clips", "kmx_scripts_clip", lambda c, h: c.sc.clip(clips=h), lambda c, o, h: c.msc.clip(clips=h)),
    Row("realigned", "Clips", "kmx_scripts_realign_device",
        lambda c, h: c.sc.realign_device(c.idx, c.al, c.d_ranks2, c.d_roff2, c.nr2, stream=c.stream, clips=h),
        lambda c, o, h: c.sc.realign_device(c.idx, c.al, o.d_ranks2, o.d_roff2, o.nr2, stream=c.stream, clips=h)),
    Row("md", "Md", "kmx_clips_md", lambda c, h: c.cl.md(c.idx, c.sc, c.al, LETTERS4, md=h), lambda c, o, h: o.cl.md(c.idx, c.sc, c.al, LETTERS4, md=h)),
    Row("mapq", "Mapq", "kmx_placements_mapq", lambda c, h: c.pl.mapq(TINY_E, c.pairs, mapq=h), lambda c, o, h: c.pl.mapq(TINY_E, o.pairs, mapq=h)),
    Row("loc", "Located", "kmx_placements_locate", lambda c, h: c.pl.locate(c.idx, c.al, mates=True, located=h),
        lambda c, o, h: c.pl.locate(c.idx, o.al, mates=True, located=h)),
    Row("sec", "Secondaries", "kmx_placements_secondaries", lambda c, h: c.pl.secondaries(c.loci, c.al, 4, secondaries=h),
        lambda c, o, h: c.pl.secondaries(c.loci, o.al, 4, secondaries=h)),
    Row("sup", "Supplementaries", "kmx_clips_supplementaries",
        lambda c, h: c.acl.supplementaries(c.reads, c.loci, c.al, c.pl, c.asc, stream=c.stream, supplementaries=h),
        lambda c, o, h: c.acl.supplementaries(c.reads, c.loci, c.al, o.pl, c.asc, stream=c.stream, supplementaries=h)),
    Row("pu", "Pileup", "kmx_clips_pileup_device", lambda c, h: c.cl.pileup(c.idx, c.sc, c.al, c.reads, stream=c.stream, pileup=h),
        lambda c, o, h: o.cl.pileup(c.idx, c.sc, c.al, c.reads, stream=c.stream, pileup=h)),
    Row("sites", "Sites", "kmx_pileup_sites", lambda c, h: c.pu.sites(c.idx, sites=h), lambda c, o, h: o.hollow.sites(c.idx, sites=h)),
)
ROW = {r.name: r for r in ROWS}


class Chain:
    """One batch of interleaved mates through every stage, on the stream of its StrandReads: the handles that the rows fill from,
    and per row a handle that the row's own call has filled once (made(row): what a refilled handle must equal)."""

    def __init__(self, engine, idx, mates):
        self.engine, self.idx, self.held, self.once = engine, idx, [], {}
        keep = self.keep
        self.reads = keep(idx.strand_reads(*pack(mates), COMP4))
        self.d_ranks2, self.d_roff2, self.nr2, self.stream = self.reads.device_ptrs()
        self.windows = keep(idx.search_windows_device(self.d_ranks2, self.d_roff2, self.nr2, K, 1, stream=self.stream))
        self.loci = self.fresh(ROW["loci"])
        self.al = self.fresh(ROW["al"])
        self.pl, self.pairs = _fold(self)
        self.res = keep(self.pairs.rescue(idx, self.reads, self.loci, self.al, self.pl, **TINY_INSERT, max_edits=TINY_E))      # rewrites pl and pairs
        self.sc = self.fresh(ROW["sc"])
        self.msc = keep(self.pl.scripts(idx, self.reads, self.loci, self.al, m=True))
        self.cl = self.fresh(ROW["cl"])
        self.asc = keep(self.al.scripts_device(idx, self.loci, self.d_ranks2, self.d_roff2, self.nr2, all=True, stream=self.stream))
        self.acl = keep(self.asc.clip(stream=self.stream))
        self.pu = self.fresh(ROW["pu"])

    def keep(self, h):
        self.held.append(h)
        return h

    def fresh(self, row):
        h = self.keep(getattr(self.engine, row.cls)())
        row.fill(self, h)
        return h

    def made(self, row):
        if row.name not in self.once:
            self.once[row.name] = self.fresh(row)
        return self.once[row.name]

    def close(self):
        for h in reversed(self.held):
            h.close()


@pytest.fixture(scope="module")
def work(engine):
    """the index with its contig table and the four batches, each through the chain once: full, quarter, large, empty"""
    idx = engine.Index(tiny_text(), 4, [K], table=2)
    idx.set_contigs(table_of(TINY_CONTIGS))
    chains = {}
    try:
        for name, mates in (("full", tiny_pairs()), ("quarter", tiny_pairs()[:4]), ("large", tiny_pairs() * 3), ("empty", [])):
            chains[name] = Chain(engine, idx, mates)
        q = chains["quarter"]
        q.plain = q.keep(idx.search(tiny_text()[:K], np.asarray([0, K], np.uint64)))       # not a windows search: the vote refuses it
        q.hollow = chains["full"].fresh(ROW["pu"])                                          # a pileup that a refusal has emptied
        refused(engine, lambda: ROW["pu"].mismatch(chains["full"], q, q.hollow), ROW["pu"].fn)
        yield chains
    finally:
        for c in chains.values():
            c.close()
        idx.close()


def views(engine, h):
    """(counts, device pointers, host arrays) with one entry per field of _view_of, as the base class gives them"""
    return h.counts(), engine._Handle.device_ptrs(h), engine._Handle.host(h)


def check(engine, row, h, state, want=None):
    """The handle in one state; want: a handle that holds what this one must hold.  Returns the device pointers."""
    counts, ptrs, host = views(engine, h)
    fields = h._view_of[1]
    assert len(NULLS[row.cls]) == len(fields) == len(ptrs) == len(host), f"{row.cls}: NULLS has {len(NULLS[row.cls])} rules for {len(fields)} fields"
    assert host._fields == tuple(name for name, _, _ in fields), f"{row.cls}: the host view names {host._fields}"
    if row.cls == "Placements":
        front = h.host(best2=False)
        assert front._fields == host._fields[:6] and len(front) == 6, f"Placements.host(best2=False) names {front._fields}"
        assert all(np.array_equal(a, b) for a, b in zip(front, host)), "Placements.host(best2=False) is not the front of host()"
    if state == REFUSED:
        assert not any(counts.values()), f"{row.name}: counts {counts} after a refusal"
    if want is not None:
        w_counts, _, w_host = views(engine, want)
        assert counts == w_counts, f"{row.name}: counts {counts}, want {w_counts}"
        for (name, _, _), g, w in zip(fields, host, w_host):
            assert (g is None) == (w is None), f"{row.name}.{name}: {'no ' if g is None else 'a '}view, want {'none' if w is None else 'one'}"
            assert g is None or (g.dtype == w.dtype and np.array_equal(g, w)), differ(f"{row.name}.{name}", g, w)
    for (name, dtype, n), rule, p, g in zip(fields, NULLS[row.cls], ptrs, host):
        n = n(counts) if callable(n) else counts[n]
        if g is None:                                          # an _optional field whose host pointer is NULL: under a contig table, only while it is empty
            assert name in h._optional and n == 0 and p is None, f"{row.name}.{name} ({state}, {n} elements): no host view, device pointer {p!r}"
            continue
        assert g.dtype == dtype and g.size == n, f"{row.name}.{name}: the host view is {g.dtype}[{g.size}], want {np.dtype(dtype)}[{n}]"
        null = n == 0 if rule is LIVE else state == REFUSED if rule is FILLED else False
        assert (p is None) == null, f"{row.name}.{name} ({state}, {n} elements): the device pointer is {p!r}; {rule}"
        if p is not None:
            d = dev_array(p, n, dtype)
            assert np.array_equal(d, g), differ(f"{row.name}.{name} (device against host)", d, g)
        elif rule is FILLED:
            assert g.tolist() == [0], f"{row.name}.{name}: {g.tolist()} after a refusal, want the one offset 0"
    if row.cls == "Alignments":                                # ctg has a pair of views of its own
        (p, nc), g = h.contigs_device_ptr(), h.contigs_host()
        n = counts["n_loci"]
        assert (p is None) == (n == 0) and (nc == len(TINY_CONTIGS)) == (state != REFUSED), f"{row.name}.ctg ({state}, {n} loci): pointer {p!r}, nc {nc}"
        if state != REFUSED:
            assert g.dtype == np.uint32 and g.size == n and np.array_equal(dev_array(p, n, np.uint32), g), f"{row.name}.ctg: {g}"
            assert want is None or np.array_equal(g, want.contigs_host()), f"{row.name}.ctg: {g}, want {want.contigs_host()}"
        else:
            assert g is None, f"{row.name}.ctg: a host view after a refusal"
    return ptrs


@contextlib.contextmanager
def without_options(engine, fn):
    """the C function fn called with NULL in the place of its options struct"""
    L = engine.lib()
    real = getattr(L, fn)

    def call(*args):
        return real(*[None if isinstance(getattr(a, "_obj", None), C.Structure) else a for a in args])

    setattr(L, fn, call)
    try:
        yield
    finally:
        setattr(L, fn, real)


def test_every_declared_handle_has_a_row(engine):
    declared = {c.__name__ for c in vars(engine).values() if isinstance(c, type) and issubclass(c, engine._Handle) and c._view_of is not None}
    assert declared - {"ApproxResult"} == {r.cls for r in ROWS} == set(NULLS), "a _Handle subclass with _view_of joins ROWS and NULLS"


def test_an_optional_field_is_none_without_a_contig_table(engine):
    """The Secondaries of the tiny batch on the index before set_contigs: ctg, which the class declares _optional, is None in host() and
    NULL on the device; every other field is the device array under its name."""
    declared = {c.__name__: c._optional for c in vars(engine).values() if isinstance(c, type) and issubclass(c, engine._Handle) and c._optional}
    assert declared == {"Secondaries": ("ctg",), "Supplementaries": ("ctg",), "Sites": ("ctg",)}, declared
    assert not any("host" in vars(getattr(engine, name)) for name in declared), "a class with _optional has a host() of its own"
    with contextlib.ExitStack() as opened:
        keep = lambda h: opened.enter_context(contextlib.closing(h))
        idx = keep(engine.Index(tiny_text(), 4, [K], table=2))
        reads = keep(idx.strand_reads(*pack(tiny_pairs()), COMP4))
        d_ranks2, d_roff2, nr2, stream = reads.device_ptrs()
        windows = keep(idx.search_windows_device(d_ranks2, d_roff2, nr2, K, 1, stream=stream))
        loci = keep(windows.vote(TINY_CHAIN["band"], TINY_CHAIN["min_votes"]))
        al = keep(loci.align_device(idx, d_ranks2, d_roff2, nr2, TINY_E, TINY_CHAIN["max_span"], stream=stream))
        assert al.contigs_host() is None
        pl = keep(engine.Placements())
        al.fold_pairs(loci, **TINY_INSERT, stream=stream, placements=pl, pairs=keep(engine.Pairs()))
        sec = keep(pl.secondaries(loci, al, 4))
        counts, ptrs, host = views(engine, sec)
        fields = sec._view_of[1]
        assert counts["n_sec"] > 0, "the tiny batch has no secondary place"
        assert host._fields == sec.host()._fields == tuple(name for name, _, _ in fields)
        assert host.ctg is None and sec.host().ctg is None and ptrs[host._fields.index("ctg")] is None, "a ctg view without a contig table"
        for (name, dtype, n), p, g in zip(fields, ptrs, host):
            if name != "ctg":
                n = n(counts) if callable(n) else counts[n]
                assert g is getattr(host, name) and g.dtype == dtype and g.size == n > 0, f"{name}: the host view is {g.dtype}[{g.size}], want {np.dtype(dtype)}[{n}]"
                assert np.array_equal(dev_array(p, n, dtype), g), differ(f"{name} (device against host)", dev_array(p, n, dtype), g)


@pytest.mark.parametrize("row", ROWS, ids=[r.name for r in ROWS])
def test_a_handle_through_every_state(engine, work, row):
    full, quarter, large, empty = (work[k] for k in ("full", "quarter", "large", "empty"))
    h = getattr(engine, row.cls)()
    try:
        row.fill(full, h)                                      # 1. filled
        first = check(engine, row, h, GIVEN, full.made(row))
        assert all(x.size for x in engine._Handle.host(h)), f"{row.name}: a field of the full batch holds no entry"
        row.fill(quarter, h)                                   # 2. a smaller batch into the same handle
        second = check(engine, row, h, GIVEN, quarter.made(row))
        assert all(a == b for a, b in zip(first, second) if a and b), f"{row.name}: a device array moved when its handle took a smaller batch"
        row.fill(large, h)                                     # 3. a larger one, after the host view was taken
        check(engine, row, h, GIVEN, large.made(row))
        row.fill(empty, h)                                     # 4. the empty batch
        check(engine, row, h, GIVEN, empty.made(row))
        row.fill(full, h)                                      # 5. a refusal that has looked at the handle
        refused(engine, lambda: row.mismatch(full, quarter, h), row.fn)
        check(engine, row, h, GIVEN if row.keeps else REFUSED, full.made(row) if row.keeps else None)
        row.fill(full, h)                                      # 6. a refusal that has not
        before = views(engine, h)
        with without_options(engine, row.fn):
            refused(engine, lambda: row.fill(full, h), row.fn)
        after = views(engine, h)
        assert before[:2] == after[:2] and all(np.array_equal(a, b) for a, b in zip(before[2], after[2])), f"{row.name}: changed by a refusal of NULL options"
        check(engine, row, h, GIVEN, full.made(row))
    finally:
        h.close()
