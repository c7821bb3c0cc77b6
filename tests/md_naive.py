"""The contract of kmx_scripts_md / kmx_rescues_md in executable form, on the host arrays of a scripts handle (sel, cig_off, cigar),
the start / end arrays that sel indexes (of the alignments, or of the rescue jobs) and the text.

Entry e: l = sel[e], s = start[l], t = end[l], the runs cigar[cig_off[e] .. cig_off[e + 1]) as len << 4 | op with I = 1, D = 2,
'=' = 7, X = 8.  A match counter c = 0 and a text cursor j = s; the runs in order: '=': c += len, j += len; 'I': nothing; 'X': for
each letter emit decimal(c), letters[text[j]], then c = 0, j += 1; 'D': emit decimal(c), '^', letters[text[j .. j + len)], then c = 0,
j += len; at the end emit decimal(c).

An entry without runs has an empty MD and is not counted.  An entry has an empty MD and is counted as mismatched when l >= bound, when
not s <= t <= n, when it has another op, when its = X D lengths do not sum to t - s, or when the MD would take 2^32 bytes or more.

md() returns (md_off[n_sel + 1] u64, md u8, n_mismatched)."""
import re

import numpy as np

OP_I, OP_D, OP_EQ, OP_X = 1, 2, 7, 8
GRAMMAR = re.compile(r"[0-9]+(([A-Z]|\^[A-Z]+)[0-9]+)*\Z")


def byte_count(runs):
    """The bytes of the MD from the run lengths alone (the text is not needed); None when a run has an op other than = X I D."""
    c = n = 0
    for v in runs:
        length, op = int(v) >> 4, int(v) & 15
        if op == OP_EQ:
            c += length
        elif op == OP_X:
            if length:
                n += len(str(c)) + 1 + 2 * (length - 1)
                c = 0
        elif op == OP_D:
            n += len(str(c)) + 1 + length
            c = 0
        elif op != OP_I:
            return None
    return n + len(str(c))


def md_one(runs, text, s, letters):
    """The MD bytes of one valid entry whose text substring starts at s."""
    out, c, j = bytearray(), 0, int(s)
    for v in runs:
        length, op = int(v) >> 4, int(v) & 15
        if op == OP_EQ:
            c += length
            j += length
        elif op == OP_X:
            for _ in range(length):
                out += str(c).encode() + bytes([letters[int(text[j])]])
                c = 0
                j += 1
        elif op == OP_D:
            out += str(c).encode() + b"^" + bytes(letters[int(x)] for x in text[j:j + length])
            c = 0
            j += length
    return bytes(out + str(c).encode())


def md(sel, cig_off, cigar, start, end, text, letters, bound=None):
    """letters: sigma output bytes by rank (bytes, str or uint8 array); bound: the entries of start / end that sel may index."""
    letters = letters.encode("latin-1") if isinstance(letters, str) else bytes(bytearray(letters))
    bound = len(start) if bound is None else bound
    n = len(text)
    md_off, out, bad = [0], bytearray(), 0
    for e, l in enumerate(sel):
        runs = cigar[int(cig_off[e]):int(cig_off[e + 1])]
        if len(runs):
            ok = int(l) < bound
            if ok:
                s, t = int(start[int(l)]), int(end[int(l)])
                ok = s <= t <= n
            count = byte_count(runs)
            if ok:
                ok = count is not None and count < 2 ** 32 and sum(int(v) >> 4 for v in runs if (int(v) & 15) != OP_I) == t - s
            if ok:
                one = md_one(runs, text, s, letters)
                assert len(one) == count
                out += one
            else:
                bad += 1
        md_off.append(len(out))
    return np.asarray(md_off, np.uint64), np.frombuffer(bytes(out), np.uint8).copy(), bad


def strings(md_off, md_bytes):
    raw = np.asarray(md_bytes, np.uint8).tobytes()
    return [raw[int(a):int(b)].decode("latin-1") for a, b in zip(md_off[:-1], md_off[1:])]


def rebuild(seq, runs, md_string):
    """The reference substring from SEQ (a str: the read as it aligns to the forward text), the CIGAR runs and the MD string alone;
    raises ValueError when the three disagree."""
    cols = []                                                  # per reference column: None (equal to the read), a letter, or ('^', letter)
    for num, dele, sub in re.findall(r"([0-9]+)|\^([A-Z]+)|([A-Z])", md_string):
        if num:
            cols += [None] * int(num)
        elif dele:
            cols += [("^", x) for x in dele]
        else:
            cols.append(sub)
    ref, i, k = [], 0, 0
    for v in runs:
        length, op = int(v) >> 4, int(v) & 15
        for _ in range(length):
            if op == OP_I:
                i += 1
                continue
            if k >= len(cols):
                raise ValueError("the MD ends before the CIGAR")
            col = cols[k]
            k += 1
            if op == OP_D:
                if not isinstance(col, tuple):
                    raise ValueError("a D without a deletion in the MD")
                ref.append(col[1])
            else:
                if isinstance(col, tuple) or i >= len(seq) or (op == OP_EQ and col is not None) or (op == OP_X and col is None):
                    raise ValueError("CIGAR and MD disagree")
                ref.append(seq[i] if col is None else col)
                i += 1
    if k != len(cols) or i != len(seq):
        raise ValueError("CIGAR, MD and SEQ differ in length")
    return "".join(ref)
