"""GPU suite: the shape of what the chain builders return.  Index.map_reads_strands and Index.map_pairs return a positional tuple whose
elements depend on scripts / tags / secondaries / clip (and rescue); every other chain test consumes a few of these shapes by
position.  Here every combination is pinned: the exact sequence of element types, the None fields of a SamTags, and that every handle
keeps the StrandReads (whose stream it was filled on) alive through _reads."""
import itertools

import numpy as np
import pytest

from kmer_index_amd import synth
from tests.helpers import pack

pytestmark = pytest.mark.gpu

K = 10
COMP = np.array([3, 2, 1, 0], np.uint8)
CHAIN = dict(band=8, min_votes=2, max_edits=4)
INSERT = dict(min_insert=100, max_insert=1000)      # pair 2 lies forward at 1700 and reverse up to 2328: a template of 628 letters

# scripts, tags, secondaries, clip: clip only where scripts is on
STRAND_CASES = [c for c in itertools.product((False, True), (False, True), (0, 2), (None, {})) if c[0] or c[3] is None]
PAIR_CASES = [c + (r,) for c in STRAND_CASES for r in (False, True)]
assert len(STRAND_CASES) == 12 and len(PAIR_CASES) == 24


@pytest.fixture(scope="module")
def mapped(engine):
    """(index, ranks, roff): a 4000-letter text and eight reads cut from it as four interleaved pairs, two of them reverse
    complements and one with two substitutions"""
    text = synth.ranks(1501, 4000, 4)
    cuts = [(100, 60), (400, 75), (800, 90), (1200, 101), (1700, 117), (2200, 128), (2800, 139), (3400, 150)]
    reads = [text[a:a + m].copy() for a, m in cuts]
    for i in (2, 5):
        reads[i] = COMP[reads[i][::-1]]
    reads[6][[40, 90]] = (reads[6][[40, 90]] + 1) % 4
    idx = engine.Index(text, 4, [K], device=0)
    yield (idx,) + pack(reads)
    idx.close()


def expected_types(engine, scripts, tags, secondaries, clip, paired=False, rescue=False):
    e = engine
    return ([e.StrandReads, e.Loci, e.Alignments, e.Placements] + [e.Pairs] * paired + [e.Scripts] * (scripts or tags) + [e.Rescues] * rescue
            + [e.SamTags] * tags + [e.Secondaries] * bool(secondaries) + [e.Clips] * (clip is not None) + [e.Clips] * (clip is not None and rescue))


def check_and_close(engine, out, want, rescue, paired):
    """the types of `out`, the fields of its SamTags, the _reads of every handle in it; then everything is closed, the reads last"""
    handles = []
    try:
        assert isinstance(out, tuple)
        for x in out:
            if isinstance(x, engine.SamTags):
                handles += [h for h in x if h is not None]
            else:
                handles.append(x)
                if isinstance(x, engine.Clips) and x.scripts is not None:
                    handles.append(x.scripts)
        assert [type(x) for x in out] == want
        for x in out:
            if isinstance(x, engine.SamTags):
                assert type(x.mapq) is engine.Mapq and type(x.md) is engine.Md
                if rescue:
                    assert type(x.rescue_scripts) is engine.Scripts and type(x.rescue_md) is engine.Md
                else:
                    assert x.rescue_scripts is None and x.rescue_md is None
            elif isinstance(x, engine.Clips):
                assert type(x.scripts) is engine.Scripts
        reads = out[0]
        assert reads.counts() == {"nr": 8, "nr2": 16}
        if paired:
            assert out[4].counts()["np"] == 4 and out[4].counts()["n_concordant"] >= 1
        else:
            assert out[3].counts()["n_placed"] == 8
        for h in handles[1:]:
            assert h._reads is reads, type(h).__name__
    finally:
        seen = set()
        for h in reversed(handles):
            if id(h) not in seen:
                seen.add(id(h))
                h.close()


@pytest.mark.parametrize("scripts,tags,secondaries,clip", STRAND_CASES)
def test_map_reads_strands_returns(engine, mapped, scripts, tags, secondaries, clip):
    idx, ranks, roff = mapped
    out = idx.map_reads_strands(ranks, roff, K, COMP, **CHAIN, scripts=scripts, tags=tags, letters="ACGT" if tags else None,
                                secondaries=secondaries, clip=clip)
    check_and_close(engine, out, expected_types(engine, scripts, tags, secondaries, clip), False, False)


@pytest.mark.parametrize("scripts,tags,secondaries,clip,rescue", PAIR_CASES)
def test_map_pairs_returns(engine, mapped, scripts, tags, secondaries, clip, rescue):
    idx, ranks, roff = mapped
    out = idx.map_pairs(ranks, roff, K, COMP, **INSERT, **CHAIN, scripts=scripts, rescue=rescue, tags=tags, letters="ACGT" if tags else None,
                        secondaries=secondaries, clip=clip)
    check_and_close(engine, out, expected_types(engine, scripts, tags, secondaries, clip, True, rescue), rescue, True)
