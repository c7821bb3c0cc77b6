"""The SAM text layer of the mapping chain: CIGAR, XA and SA strings, the SAM lines of a batch and its header, from host arrays.

Pure Python / numpy: nothing here loads the library, knows a handle class or needs a device.  The `*_host` arguments are what the
handles of engine.py return from host(); plain tuples of arrays in the same order serve as well.  engine.py re-exports every name."""
import numpy as np

# mirrored from include/kmx.h; engine.py takes them from here
CIGAR_OPS = "MIDNSHP=X"
PAIR_CONCORDANT = 1
NO_CONTIG = 0xFFFFFFFF


def _runs_strings(cig_off, cigar):
    """One CIGAR string per entry from the offsets and the runs (len << 4 | op)."""
    runs = [f"{int(v) >> 4}{CIGAR_OPS[int(v) & 15]}" for v in cigar]
    return ["".join(runs[int(a):int(b)]) for a, b in zip(cig_off[:-1], cig_off[1:])]


def _letters_table(letters):
    """The rank -> output byte table as a contiguous uint8 array."""
    if isinstance(letters, str):
        letters = letters.encode("ascii")
    if isinstance(letters, (bytes, bytearray)):
        return np.frombuffer(bytes(letters), np.uint8).copy()
    return np.ascontiguousarray(letters, np.uint8)


def _clip_fields(entry, clips_host):
    """entry[nr]: the entry of every public read among those of clips_host (Clips.host()), -1 for none -> (tl i64, nm i64,
    score i64, has bool)"""
    entry = np.asarray(entry, np.int64)
    score, _, _, tl, _, nm, _, _, _ = clips_host
    has = entry >= 0
    at = np.where(has, entry, 0)
    if score.size == 0:
        zero = np.zeros(entry.size, np.int64)
        return zero, zero.copy(), zero.copy(), np.zeros(entry.size, bool)
    return tuple(np.where(has, a.astype(np.int64)[at], 0) for a in (tl, nm, score)) + (has,)


def _first_given(strings):
    """A list of strings, or several lists of equal length (the placements', then the rescue's): per read the first that is not empty."""
    if strings and not isinstance(strings[0], str):
        return [next((s for s in group if s), "") for group in zip(*strings)]
    return list(strings)


def _reference(who, located, rname, ctgs, whose):
    """How the records of `who` name their reference: where(start, ctg, k) -> (name, 1-based position) of record k.
    located=(names, ctg_off): the name of the record's contig and a contig-local position, which needs every array of `ctgs`
    (`whose` says in the refusal where they come from); otherwise `rname` and the position in the text."""
    if located is None and rname is None:
        raise ValueError(f"{who}: give rname, or located=(names, ctg_off)")
    if located is None:
        return lambda start, ctg, k: (rname, int(start[k]) + 1)
    if any(c is None for c in ctgs):
        raise ValueError(f"{who}: located needs the ctg of {whose}")
    names, ctg_off = located
    return lambda start, ctg, k: (names[int(ctg[k])], int(start[k]) - int(ctg_off[int(ctg[k])]) + 1)


def _seq(who, i, ranks, roff, sigma, table, comp, reverse):
    """SEQ of read i: its letters by `table`, those of the reverse complement under `comp` when reverse; * for an empty read."""
    q = ranks[int(roff[i]):int(roff[i + 1])]
    if (q >= sigma).any():
        raise ValueError(f"{who}: read {i} holds a letter outside the alphabet")
    return table[comp[q[::-1]] if reverse else q].tobytes().decode("latin-1") or "*"


def xa_strings(sec_off, dist, start, ctg, cigars, strand_names="+-", located=None, rname=None, shift=None):
    """The XA:Z: value of every public read from the host arrays of a Secondaries and one CIGAR per entry: "" or items
    rname,<strand><pos>,CIGAR,NM; in bwa's form, pos 1-based.  located=(names, ctg_off) with ctg: the entry's contig name and a
    contig-local pos; otherwise rname and the position in the text.  shift: the text letters clipped off the left of every entry
    (the tl of a Clips; dist and cigars then are the clipped nm and strings), added to its position.  Pure Python: no device is
    needed."""
    sec_off = np.asarray(sec_off, np.uint64)
    if shift is not None:
        start = np.asarray(start, np.int64) + np.asarray(shift, np.int64)
    where = _reference("xa", located, rname, (ctg,), "a Secondaries made under a contig table")
    out = []
    for i in range((sec_off.size - 1) // 2):
        items = []
        for s in (0, 1):
            for e in range(int(sec_off[2 * i + s]), int(sec_off[2 * i + s + 1])):
                name, pos = where(start, ctg, e)
                items.append(f"{name},{strand_names[s]}{pos},{cigars[e] or '*'},{int(dist[e])};")
        out.append("".join(items))
    return out


def supplementary_mapq(score, second_score, cap=60):
    """The MAPQ of every part from its score and its runner-up's: 0 where second_score >= score, else
    min(cap, cap (score - second_score) // score).  A stated gap rule like kmx_placements_mapq's, not a calibrated one.  Pure numpy."""
    score = np.asarray(score, np.int64)
    second = np.asarray(second_score, np.int64)
    q = np.minimum(cap, cap * (score - second) // np.maximum(score, 1))
    return np.where(second >= score, 0, q).astype(np.uint8)


def sa_strings(sup_off, primary, entries, located=None, rname=None, strand_names="+-"):
    """The SA:Z: values of the records of every public read.  primary = (pos, strand, cigars, mapq, nm[, ctg]) with one value per
    public read, entries = (pos, strand, cigars, mapq, nm[, ctg]) with one per entry of a Supplementaries (sup_off counts them per
    read): pos the 0-based position of the clipped record in the text (start + tl; t0), cigars the clipped CIGARs.  The records of a
    read are its primary and then its entries, each as rname,pos,strand,CIGAR,mapQ,NM; with pos 1-based; located=(names, ctg_off)
    with ctg: the contig's name and a contig-local pos, otherwise `rname` and the position in the text.  Returns per read the list
    [the primary's value, entry 0's, ...]: every record's value is the other records of its read, in that order ("" for the primary
    of a read without entries).  Pure Python: no device is needed."""
    sup_off = np.asarray(sup_off, np.uint64)
    primary, entries = (tuple(src[:6]) + (None,) * (6 - len(src)) for src in (primary, entries))       # ctg may be left out
    where = _reference("sa", located, rname, (primary[-1], entries[-1]), "the primaries and of the entries")

    def record(src, k):
        pos, strand, cigars, mapq, nm, ctg = src
        name, at = where(pos, ctg, k)
        return f"{name},{at},{strand_names[int(strand[k])]},{cigars[k] or '*'},{int(mapq[k])},{int(nm[k])};"

    out = []
    for i in range(sup_off.size - 1):
        a, b = int(sup_off[i]), int(sup_off[i + 1])
        if a == b:
            out.append([""])
            continue
        recs = [record(primary, i)] + [record(entries, x) for x in range(a, b)]
        out.append(["".join(r for k, r in enumerate(recs) if k != j) for j in range(len(recs))])
    return out


def sam_supplementary_lines(primary_lines, ranks, roff, letters, complement, sigma, sup_host, cigars, mds, mapq, sa, rname=None, located=None):
    """The supplementary SAM lines (FLAG 0x800, no newline) of a batch, read after read in the order of the entries.
    primary_lines: the lines of sam_lines for the same reads (QNAME, the pair bits of FLAG, RNEXT and PNEXT are taken from them);
    sup_host: Supplementaries.host(); cigars, mds, mapq: one per entry (Supplementaries.cigars / .mds / .mapq); sa: what sa_strings
    returned.  A line has FLAG 0x800, plus 0x10 on strand 1, plus the primary's pair bits (0x1, 0x8, 0x20, 0x40, 0x80: not 0x2);
    RNAME and POS of the part (located=(names, ctg_off): its contig and a contig-local POS, else `rname` and t0 + 1); the entry's
    MAPQ; the clipped CIGAR with its S runs (soft, not hard: SEQ is the whole read, reverse-complemented on strand 1); RNEXT and
    PNEXT as on the primary line (= only where the mate lies on the part's own reference); TLEN 0; NM:i:, MD:Z:, AS:i: and SA:Z:.
    Pure Python / numpy: no device is needed."""
    table = _letters_table(letters)
    comp = np.ascontiguousarray(complement, np.uint8)
    ranks = np.asarray(ranks, np.uint8)
    roff = np.asarray(roff, np.uint64)
    sup_off, _, _, strand, _, _, t0, _, score, _, nm, ctg, _ = sup_host
    where = _reference("sam_supplementary_lines", located, rname, (ctg,), "a Supplementaries made under a contig table")
    if not (roff.size - 1 == len(primary_lines) == len(sa) == sup_off.size - 1) or not (len(cigars) == len(mds) == len(mapq) == strand.size):
        raise ValueError("sam_supplementary_lines: the arrays disagree in the number of reads or of entries")
    lines = []
    for i in range(sup_off.size - 1):
        a, b = int(sup_off[i]), int(sup_off[i + 1])
        if a == b:
            continue
        first = primary_lines[i].split("\t")
        mate_name = first[2] if first[6] == "=" else first[6]
        for j, x in enumerate(range(a, b)):
            name, pos = where(t0, ctg, x)
            flag = 0x800 | (0x10 if strand[x] == 1 else 0) | (int(first[1]) & (0x1 | 0x8 | 0x20 | 0x40 | 0x80))
            seq = _seq("sam_supplementary_lines", i, ranks, roff, sigma, table, comp, strand[x] == 1)
            rnext = "*" if mate_name == "*" else "=" if mate_name == name else mate_name
            lines.append("\t".join([first[0], str(flag), name, str(pos), str(int(mapq[x])), cigars[x] or "*", rnext, first[7], "0", seq, "*",
                                    f"NM:i:{int(nm[x])}", f"MD:Z:{mds[x]}", f"AS:i:{int(score[x])}", f"SA:Z:{sa[i][j + 1]}"]))
    return lines


def sam_pair_fields(strand, start, cls, tlen):
    """The SAM fields that a pair decides, per read, from the host arrays of a Placements (strand, start: 2 np entries, mates
    interleaved) and a Pairs (cls, tlen: np entries): (FLAG u16, POS i64, PNEXT i64, TLEN i32).  FLAG carries 0x1, 0x2 (the pair is
    concordant), 0x4 / 0x8 (the read / its mate is unplaced), 0x10 / 0x20 (the read / its mate lies on the reverse strand) and
    0x40 / 0x80 (mate 1 / mate 2); POS is 1-based, an unplaced read takes its mate's and 0 when both are unplaced; PNEXT is the
    mate's POS; TLEN is tlen for mate 1 and -tlen for mate 2.  Pure numpy: no device is needed."""
    strand = np.asarray(strand, np.uint8)
    start = np.asarray(start, np.uint32)
    cls = np.asarray(cls, np.uint8)
    tlen = np.asarray(tlen, np.int32)
    mate = np.arange(strand.size) ^ 1
    placed = strand != 255
    flag = np.full(strand.size, 0x1, np.uint16)
    flag[np.repeat(cls == PAIR_CONCORDANT, 2)] |= 0x2
    flag[~placed] |= 0x4
    flag[~placed[mate]] |= 0x8
    flag[placed & (strand == 1)] |= 0x10
    flag[placed[mate] & (strand[mate] == 1)] |= 0x20
    flag[0::2] |= 0x40
    flag[1::2] |= 0x80
    own = np.where(placed, start.astype(np.int64) + 1, 0)
    pos = np.where(placed, own, own[mate])
    t = np.repeat(tlen, 2)
    t[1::2] = -t[1::2]
    return flag, pos, pos[mate], t.astype(np.int32)


def concat_sequences(seqs):
    """The text of a multi-sequence reference: (ranks uint8, ctg_off uint64[len(seqs) + 1]) with sequence c at
    ranks[ctg_off[c]:ctg_off[c + 1]], ready for Index(...) and Index.set_contigs.  An empty sequence is refused (a contig table
    has none).  Pure numpy: no device is needed."""
    seqs = [np.ascontiguousarray(q, np.uint8).ravel() for q in seqs]
    if any(q.size == 0 for q in seqs):
        raise ValueError("concat_sequences: an empty sequence")
    ctg_off = np.zeros(len(seqs) + 1, np.uint64)
    if seqs:
        ctg_off[1:] = np.cumsum([q.size for q in seqs], dtype=np.uint64)
    return (np.concatenate(seqs) if seqs else np.zeros(0, np.uint8)), ctg_off


def sam_header(names, ctg_off):
    """The header lines (no newlines) of a SAM file over a contig table: "@HD\tVN:1.6\tSO:unsorted" and one
    "@SQ\tSN:<name>\tLN:<length>" per contig."""
    ctg_off = np.asarray(ctg_off, np.uint64)
    if ctg_off.size != len(names) + 1:
        raise ValueError("sam_header: ctg_off needs one entry more than there are names")
    return ["@HD\tVN:1.6\tSO:unsorted"] + [f"@SQ\tSN:{nm}\tLN:{int(b) - int(a)}" for nm, a, b in zip(names, ctg_off[:-1], ctg_off[1:])]


def sam_lines(qnames, ranks, roff, letters, complement, sigma, rname, placements_host, cigars, mds, mapq, pairs_host=None, located_host=None,
              xa=None, clip_fields=None, sa=None):
    """One SAM line (no newline) per public read from host arrays: the reads (ranks, roff), the rank -> letter table, the rank
    complement table, Placements.host(), the CIGAR and MD strings per read (Placements.cigars / .mds; a tuple of two lists, the
    placements' and the rescue's, gives a rescued read those of the rescue), Mapq.host() and, for paired reads, Pairs.host().
    FLAG / POS / PNEXT / TLEN come from sam_pair_fields when pairs_host is given; otherwise FLAG is 0 / 4 / 16, POS is start + 1 and
    there is no mate.  CIGAR is * when the read is unplaced, RNEXT = or *, SEQ the reverse complement for a reverse placement,
    QUAL *; placed reads carry NM:i: (the distance) and MD:Z:.  located_host (Located.host(): ctg, pos) switches to contig
    coordinates: rname then is a sequence of one name per contig, RNAME the read's contig (an unplaced read with a placed mate takes
    the mate's), POS and PNEXT are contig-local, RNEXT is = for the same contig and the mate's contig name otherwise.  xa
    (Secondaries.xa(): one string per read) appends XA:Z:<string> behind MD:Z: to every placed read whose string is not empty; None
    leaves the lines as they were.  clip_fields (Placements.clip_fields(); a tuple of two, the placements' and the rescue's, like
    cigars) writes soft-clipped records: cigars and mds then are the clipped ones (Clips.strings(), Clips.md()), a read's POS is
    start + tl, and so are its contig-local POS and its mate's PNEXT, NM:i: is the clipped nm, and AS:i:<score> follows MD:Z:.  TLEN
    stays the pair fold's, measured between the UNCLIPPED outer ends.  None leaves every line as it was.  sa (what sa_strings or
    Supplementaries.sa returned: per read a list whose first value is the primary's) appends SA:Z:<value> behind XA:Z: to every
    placed read whose value is not empty; None leaves every line as it was (the FLAG 0x800 lines: sam_supplementary_lines).  Pure
    Python / numpy: no device is needed."""
    table = _letters_table(letters)
    comp = np.ascontiguousarray(complement, np.uint8)
    if table.size < sigma or comp.size < sigma:
        raise ValueError("sam_lines: letters and complement need sigma entries")
    ranks = np.asarray(ranks, np.uint8)
    roff = np.asarray(roff, np.uint64)
    strand, dist, start = (np.asarray(a) for a in placements_host[1:4])
    cls, tlen = (None, None) if pairs_host is None else pairs_host[:2]
    nr = strand.size
    cigars, mds = _first_given(cigars), _first_given(mds)
    mapq = np.asarray(mapq, np.uint8)
    if not (roff.size - 1 == len(qnames) == len(cigars) == len(mds) == mapq.size == nr):
        raise ValueError("sam_lines: the arrays disagree in the number of reads")
    if xa is not None and len(xa) != nr:
        raise ValueError("sam_lines: xa disagrees in the number of reads")
    if sa is not None and len(sa) != nr:
        raise ValueError("sam_lines: sa disagrees in the number of reads")
    placed = strand != 255
    shift = nm = score = has = None
    if clip_fields is not None:
        groups = clip_fields if len(clip_fields) == 2 else (clip_fields,)
        if any(len(g) != 4 or any(np.asarray(a).size != nr for a in g) for g in groups):
            raise ValueError("sam_lines: clip_fields is (tl, nm, score, has) per read, or a tuple of two of them")
        shift, nm, score, has = (np.asarray(a) for a in groups[0])
        for g in groups[1:]:                                   # a rescued read takes the rescue's
            take = ~has & np.asarray(g[3], bool)
            shift, nm, score = (np.where(take, np.asarray(b), a) for a, b in zip((shift, nm, score), g[:3]))
            has = has | take
        has = np.asarray(has, bool) & placed
        shift = np.where(has, shift, 0).astype(np.int64)
        start = (start.astype(np.int64) + shift).astype(np.uint32)
    if pairs_host is not None:
        flag, pos, pnext, tlen = sam_pair_fields(strand, start, cls, tlen)
    else:
        flag = np.where(placed, np.where(strand == 1, 0x10, 0), 0x4)
        pos = np.where(placed, start.astype(np.int64) + 1, 0)
        pnext, tlen = np.zeros(nr, np.int64), np.zeros(nr, np.int32)
    names = nextname = None
    if located_host is not None:
        ctg, lpos = (np.asarray(a, np.uint32) for a in located_host)
        if ctg.size != nr or lpos.size != nr:
            raise ValueError("sam_lines: the located arrays disagree in the number of reads")
        if (placed & (ctg == NO_CONTIG)).any():
            raise ValueError("sam_lines: a placed read has no contig (n_mismatched of the Located is not 0)")
        if (ctg[placed] >= len(rname)).any():
            raise ValueError("sam_lines: a contig without a name")
        own = np.where(placed, lpos.astype(np.int64) + 1 + (shift if shift is not None else 0), 0)
        if pairs_host is not None:
            mate = np.arange(nr) ^ 1
            rc = np.where(placed, ctg, ctg[mate])              # an unplaced read takes its mate's contig and POS
            pos = np.where(placed, own, own[mate])
            pnext = pos[mate]
            names = [rname[int(c)] if c != NO_CONTIG else "*" for c in rc]
            nextname = ["*" if rc[j] == NO_CONTIG else "=" if rc[j] == rc[i] else names[j] for i, j in enumerate(mate)]
        else:
            pos = own
            names = [rname[int(c)] if c != NO_CONTIG else "*" for c in ctg]
            nextname = ["*"] * nr
    lines = []
    for i in range(nr):
        seq = _seq("sam_lines", i, ranks, roff, sigma, table, comp, placed[i] and strand[i] == 1)
        fields = [str(qnames[i]), str(int(flag[i])), (rname if pos[i] else "*") if names is None else names[i], str(int(pos[i])), str(int(mapq[i])),
                  (cigars[i] or "*") if placed[i] else "*", ("=" if pnext[i] else "*") if names is None else nextname[i], str(int(pnext[i])),
                  str(int(tlen[i])), seq, "*"]
        if placed[i]:
            fields += [f"NM:i:{int(nm[i]) if has is not None and has[i] else int(dist[i])}", f"MD:Z:{mds[i]}"]
            if has is not None and has[i]:
                fields.append(f"AS:i:{int(score[i])}")
            if xa is not None and xa[i]:
                fields.append(f"XA:Z:{xa[i]}")
            if sa is not None and sa[i][0]:
                fields.append(f"SA:Z:{sa[i][0]}")
        lines.append("\t".join(fields))
    return lines
