"""kmer_index_amd/sam.py, the SAM text layer: it stands without the binding, engine.py re-exports its names, and its writers take
plain tuples for their *_host arguments.  The one hand-made read of the writers' tests: ACGT, placed forward at position 3 of the
text, which is position 1 of the contig c1 = text[2:10)."""
import ast
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SAM_PY = os.path.join(ROOT, "kmer_index_amd", "sam.py")
MOVED = ("xa_strings", "sa_strings", "supplementary_mapq", "sam_supplementary_lines", "sam_pair_fields", "sam_header", "sam_lines",
         "concat_sequences", "_runs_strings", "_letters_table", "_clip_fields", "_first_given")
CONSTANTS = ("CIGAR_OPS", "NO_CONTIG", "PAIR_CONCORDANT")
FORBIDDEN = ("ctypes", "kmer_index_amd.engine", "kmer_index_amd.build")

CHILD = """
import importlib.util, sys
import numpy                                                    # (numpy brings in what it likes; the question is what sam.py adds)
before = set(sys.modules)
spec = importlib.util.spec_from_file_location("sam_alone", sys.argv[1])
sam = importlib.util.module_from_spec(spec)
spec.loader.exec_module(sam)
assert sam.sam_header(["c0"], [0, 7]) == ["@HD\\tVN:1.6\\tSO:unsorted", "@SQ\\tSN:c0\\tLN:7"]
print(sorted(set(sys.modules) - before - {"sam_alone"}))
print([m for m in ("kmer_index_amd", "kmer_index_amd.engine", "kmer_index_amd.build") if m in sys.modules])
"""


def test_sam_py_imports_numpy_and_the_standard_library_only():
    """by its source: no relative import, and nothing absolute but numpy and standard-library modules other than ctypes"""
    with open(SAM_PY) as f:
        tree = ast.parse(f.read())
    imported = set()
    for node in ast.walk(tree):
        if isinstance(node, ast.ImportFrom):
            assert node.level == 0, f"sam.py line {node.lineno}: a relative import"
            imported.add(node.module.split(".")[0])
        elif isinstance(node, ast.Import):
            imported.update(a.name.split(".")[0] for a in node.names)
        elif isinstance(node, ast.Call):
            assert getattr(node.func, "id", getattr(node.func, "attr", "")) not in ("__import__", "import_module"), f"sam.py line {node.lineno}: an import by call"
    assert "numpy" in imported and "ctypes" not in imported and "kmer_index_amd" not in imported, imported
    assert imported - {"numpy"} <= set(sys.stdlib_module_names), imported


def test_sam_py_loads_alone_in_a_fresh_process():
    """loaded by its path (the package's __init__ would bring engine.py along), it works and adds no module at all beyond numpy's"""
    out = subprocess.run([sys.executable, "-c", CHILD, SAM_PY], capture_output=True, text=True, timeout=120, cwd=os.path.dirname(ROOT))
    assert out.returncode == 0, out.stderr
    added, package = out.stdout.strip().splitlines()
    assert not any(m == bad or m.startswith(bad + ".") for m in ast.literal_eval(added) for bad in FORBIDDEN), f"loading sam.py imported {added}"
    assert package == "[]", f"loading sam.py by path left {package} in sys.modules"


def test_engine_reexports_the_text_layer(engine):
    from kmer_index_amd import sam
    for name in MOVED + CONSTANTS:
        assert getattr(engine, name) is getattr(sam, name), f"engine.{name} is not sam.{name}"
    assert (sam.CIGAR_OPS, sam.NO_CONTIG, sam.PAIR_CONCORDANT) == ("MIDNSHP=X", 0xFFFFFFFF, 1)
    with open(engine.__file__) as f:
        defined = {n.name for n in ast.parse(f.read()).body if isinstance(n, ast.FunctionDef)}
    assert not defined & set(MOVED), f"engine.py still defines {sorted(defined & set(MOVED))}"


# ---- the writers on plain tuples ----------------------------------------------------------------------------------------------------------------
u8, u32 = (lambda *v: np.asarray(v, np.uint8)), (lambda *v: np.asarray(v, np.uint32))
READ = dict(qnames=["r0"], ranks=u8(0, 1, 2, 3), roff=np.asarray([0, 4], np.uint64), letters="ACGT", complement=u8(3, 2, 1, 0), sigma=4)
PLACEMENTS = (u32(0), u8(0), u8(0), u32(3), u32(7), u8(255))    # locus, strand, dist, start, end, second: forward at 3
LOCATED = (("c0", "c1"), np.asarray([0, 2, 10], np.uint64))     # (names, ctg_off)


def but_name_and_pos(record, sep, name_at, pos_at):
    fields = record.rstrip(";").split(sep)
    return [f for k, f in enumerate(fields) if k not in (name_at, pos_at)]


def test_sam_lines_takes_plain_tuples():
    from kmer_index_amd import sam
    assert type(PLACEMENTS) is tuple
    by_rname = sam.sam_lines(**READ, rname="chr", placements_host=PLACEMENTS, cigars=["4="], mds=["4"], mapq=u8(60))
    by_contig = sam.sam_lines(**READ, rname=LOCATED[0], placements_host=PLACEMENTS, cigars=["4="], mds=["4"], mapq=u8(60), located_host=(u32(1), u32(1)))
    assert by_rname == ["r0\t0\tchr\t4\t60\t4=\t*\t0\t0\tACGT\t*\tNM:i:0\tMD:Z:4"]
    assert by_contig == ["r0\t0\tc1\t2\t60\t4=\t*\t0\t0\tACGT\t*\tNM:i:0\tMD:Z:4"]
    assert but_name_and_pos(by_rname[0], "\t", 2, 3) == but_name_and_pos(by_contig[0], "\t", 2, 3)


def test_xa_strings_takes_plain_arrays():
    from kmer_index_amd import sam
    sec = dict(sec_off=np.asarray([0, 1, 1], np.uint64), dist=u8(1), start=u32(3), ctg=u32(1), cigars=["4="])   # one entry, forward at 3
    by_rname, by_contig = sam.xa_strings(**sec, rname="chr"), sam.xa_strings(**sec, located=LOCATED)
    assert by_rname == ["chr,+4,4=,1;"] and by_contig == ["c1,+2,4=,1;"]
    assert by_rname[0].split(",")[2:] == by_contig[0].split(",")[2:] and by_rname[0].split(",")[1][0] == by_contig[0].split(",")[1][0] == "+"


def test_sa_strings_takes_plain_tuples():
    from kmer_index_amd import sam
    sup_off = np.asarray([0, 1], np.uint64)
    primary = (u32(3), u8(0), ["4="], u8(60), u8(0), u32(1))                    # pos, strand, cigars, mapq, nm, ctg: the read at 3
    entries = (u32(8), u8(1), ["2S2="], u8(30), u8(0), u32(1))                  # one part, reverse at 8
    by_rname, by_contig = sam.sa_strings(sup_off, primary, entries, rname="chr"), sam.sa_strings(sup_off, primary, entries, located=LOCATED)
    assert by_rname == [["chr,9,-,2S2=,30,0;", "chr,4,+,4=,60,0;"]]            # every record's value is the other record
    assert by_contig == [["c1,7,-,2S2=,30,0;", "c1,2,+,4=,60,0;"]]
    assert sam.sa_strings(sup_off, primary[:5], entries[:5], rname="chr") == by_rname          # ctg may be left out without located
    for a, b in zip(by_rname[0], by_contig[0]):
        assert but_name_and_pos(a, ",", 0, 1) == but_name_and_pos(b, ",", 0, 1)


def test_sam_supplementary_lines_takes_a_plain_tuple():
    from kmer_index_amd import sam
    primary = ["r0\t0\tchr\t4\t60\t4=\t*\t0\t0\tACGT\t*\tNM:i:0\tMD:Z:4"]
    # sup_off, ent, locus, strand, q0, q1, t0, t1, score, second_score, nm, ctg, more: one part, forward at 3
    sup_host = (np.asarray([0, 1], np.uint64), u32(0), u32(0), u8(0), np.asarray([0], np.uint16), np.asarray([4], np.uint16), u32(3), u32(7),
                np.asarray([4], np.int32), np.asarray([0], np.int32), np.asarray([0], np.uint16), u32(1), u8(0))
    assert type(sup_host) is tuple
    reads = {k: READ[k] for k in ("ranks", "roff", "letters", "complement", "sigma")}
    rest = dict(sup_host=sup_host, cigars=["4="], mds=["4"], mapq=u8(60), sa=[["X;", "Y;"]])
    by_rname = sam.sam_supplementary_lines(primary, **reads, **rest, rname="chr")
    by_contig = sam.sam_supplementary_lines(primary, **reads, **rest, located=LOCATED)
    assert by_rname == ["r0\t2048\tchr\t4\t60\t4=\t*\t0\t0\tACGT\t*\tNM:i:0\tMD:Z:4\tAS:i:4\tSA:Z:Y;"]
    assert by_contig == ["r0\t2048\tc1\t2\t60\t4=\t*\t0\t0\tACGT\t*\tNM:i:0\tMD:Z:4\tAS:i:4\tSA:Z:Y;"]
    assert but_name_and_pos(by_rname[0], "\t", 2, 3) == but_name_and_pos(by_contig[0], "\t", 2, 3)
