"""GPU tests of bin/kmers-matrix-distance-folder and bin/kmers-matrix-distance-merge: the files
they create and every file's lines (compared as sets: the reference prints hash order) against
oracle_matrix_distance run once per problem on the CPU, with the score text
'%g' % float32(count) / float32(len1 + len2) over the first-record length of each id."""
import os
import subprocess

import numpy as np
import pytest

import oracle_ref
from conftest import ROOT
from test_gpu_matrix import make_db, queries

import oracle.front_ref as fr  # noqa: E402  (test infrastructure)

pytestmark = pytest.mark.gpu

BIN = os.path.join(ROOT, "bin")
FOLDER, MERGE = "kmers-matrix-distance-folder", "kmers-matrix-distance-merge"


class Env:
    pass


@pytest.fixture(scope="module")
def env(skm, gpu, tmp_path_factory):
    """A data directory written by hand (kmer_data.mph/.dat by mph_build, function.index) and
    family-sorted query records to cut input files from."""
    for t in (FOLDER, MERGE):
        if not os.path.exists(os.path.join(BIN, t)):
            subprocess.check_call(["make", "-C", ROOT, "-j8", "tools"])
            break
    e = Env()
    data = tmp_path_factory.mktemp("data")
    e.data = str(data)
    _, e.funcs, base = make_db(skm, data)
    with open(os.path.join(e.data, "function.index"), "w") as fh:
        fh.write("".join(f"{i}\t{f}\n" for i, f in enumerate(e.funcs)))
    e.bdz = oracle_ref.Bdz(open(base + ".mph", "rb").read())
    e.dat = open(base + ".dat", "rb").read()
    e.hypo = e.funcs.index("hypothetical protein")
    q = queries(1500)
    order = np.argsort(q.labels, kind="stable")
    e.recs = [(b"fig|83333.1.peg.%d" % s, q.residues[int(q.seq_off[s]):int(q.seq_off[s]) + int(q.seq_len[s])].tobytes())
              for s in order]
    return e


def fasta(recs, width=60):
    out = []
    for rid, seq in recs:
        out.append(b">" + rid + b" some definition\n")
        out += [seq[i:i + width] + b"\n" for i in range(0, len(seq), width)]
    return b"".join(out)


def expected_lines(e, inputs):
    """The line set of one problem; None when no input file is usable (no output file)."""
    usable = [p for p in inputs if os.path.isfile(p) and os.path.getsize(p) > 0]
    if not usable:
        return None
    recs = [r for p in usable for r in fr.parse_fasta(open(p, "rb").read())]
    ids, first_len = {}, []
    for r in recs:
        if r[0] not in ids:
            ids[r[0]] = len(ids)
            first_len.append(len(r[2]))
    if not recs:
        return set()
    idx = np.array([ids[r[0]] for r in recs], np.uint32)
    names = list(ids)
    res, off, ln = fr.records_arrays(recs)
    pairs = oracle_ref.matrix_distance(e.bdz, e.dat, res, off, ln, idx, e.hypo)
    return {"%s\t%s\t%d\t%s" % (names[a].decode(), names[b].decode(), c,
                                "%g" % float(np.float32(c) / np.float32(first_len[a] + first_len[b])))
            for a, b, c in pairs}


def file_lines(path):
    txt = open(path).read()
    assert txt == "" or txt.endswith("\n")
    lines = txt.split("\n")[:-1]
    assert len(lines) == len(set(lines))
    return set(lines)


def run(tool, *args):
    p = subprocess.run([os.path.join(BIN, tool), *args], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr
    return p


def test_folder(env, tmp_path):
    inp, out = tmp_path / "in", tmp_path / "out"
    inp.mkdir()
    out.mkdir()
    r = env.recs
    files = {"famA": r[0:30], "famB": r[30:42], "famC": r[400:401], "famD": r[600:640], "done": r[700:710]}
    # a repeated id: one index, the first record's length in the score
    files["rep"] = r[800:810] + [(r[800][0], r[800][1][7:])] + r[810:815]
    for name, recs in files.items():
        (inp / name).write_bytes(fasta(recs))
    (inp / "noid").write_bytes(fasta(r[900:905]) + b">\n" + r[905][1] + b"\n" + fasta(r[906:912]))
    (inp / "empty").write_bytes(b"")
    (inp / "sub").mkdir()
    (inp / "sub" / "inner").write_bytes(fasta(r[0:5]))
    (out / "done").write_text("seeded\n")
    names = ["famA", "famB", "famC", "famD", "rep", "noid"]
    want = {n: expected_lines(env, [str(inp / n)]) for n in names}
    assert len(want["famA"]) > 50 and len(want["rep"]) > 10 and len(want["noid"]) > 10 and want["famC"] == set()
    assert any(line.startswith(r[800][0].decode() + "\t") for line in want["rep"])

    p = run(FOLDER, env.data, str(inp), str(out), "--verbose", "-j", "4")
    assert sorted(os.listdir(out)) == sorted(names + ["done"])  # none for the empty input, no leftovers
    assert (out / "done").read_text() == "seeded\n"
    first = {n: (out / n).read_bytes() for n in names}
    for n in names:
        assert file_lines(out / n) == want[n], n
    listed = [os.path.basename(x) for x in fr.list_files(str(inp)) if os.path.basename(x) != "done"]
    work = [line for line in p.stderr.split("\n") if line.startswith('"')]
    assert work == [f'"{inp}/{n}" "{out}/{n}"' for n in listed]
    assert f"{inp}/famA Start all to all comparison\n" in p.stderr and f"{inp}/famA all to all done\n" in p.stderr
    assert f'Skip compute "{inp}/empty"\n' in p.stderr and "kmer_hit_map size " in p.stderr

    # the same work in at least three batches (famA and famD alone exceed 3000 windows, and a batch
    # of several problems stays below them): identical files
    out2 = tmp_path / "out2"
    out2.mkdir()
    (out2 / "done").write_text("seeded\n")
    run(FOLDER, "-d", env.data, "--input-dir", str(inp), "--output-dir", str(out2), "--batch-windows", "3000")
    assert sorted(os.listdir(out2)) == sorted(names + ["done"])
    for n in names:
        assert (out2 / n).read_bytes() == first[n], n

    # a complete output directory: only the empty input is listed again, nothing changes
    stamp = {n: os.stat(out / n).st_mtime_ns for n in names}
    p = run(FOLDER, env.data, str(inp), str(out))
    assert p.stderr == f'"{inp}/empty" "{out}/empty"\n'
    assert sorted(os.listdir(out)) == sorted(names + ["done"])
    assert {n: os.stat(out / n).st_mtime_ns for n in names} == stamp


def test_merge(env, tmp_path):
    base, out = tmp_path / "genus.data", tmp_path / "out"
    out.mkdir()
    r = env.recs
    genera = ["Alpha", "Beta", "Gamma"]
    for g in genera + ["NoDefs"]:
        (base / g / "fasta_by_function").mkdir(parents=True)
    for g in genera:
        (base / g / "local.family.defs").write_text("x\n")
    (base / "stray_file").write_text("x\n")
    fam = {g: base / g / "fasta_by_function" for g in genera + ["NoDefs"]}
    # family 0: in all three genera; NoDefs is not a genus directory
    for k, g in enumerate(genera + ["NoDefs"]):
        (fam[g] / "0").write_bytes(fasta(r[10 * k:10 * k + 10]))
    # family 1: missing in Beta
    (fam["Alpha"] / "1").write_bytes(fasta(r[400:415]))
    (fam["Gamma"] / "1").write_bytes(fasta(r[415:425]))
    # family 2: only empty files -> no output file
    for g in genera:
        (fam[g] / "2").write_bytes(b"")
    # family 3: the same id in two genera, with different lengths: one index, the first length
    (fam["Alpha"] / "3").write_bytes(fasta(r[600:610]))
    (fam["Beta"] / "3").write_bytes(fasta([(r[600][0], r[600][1][9:]), (r[603][0], r[603][1][:-11])] + r[610:620]))
    (fam["Gamma"] / "3").write_bytes(fasta(r[620:625]))
    # family 4: one genus only
    (fam["Beta"] / "4").write_bytes(fasta(r[800:820]))
    # the tool's genus order: readdir order of the base directory's sub-directories
    with os.scandir(base) as it:
        order = [e.name for e in it if e.is_dir() and os.path.isfile(os.path.join(base, e.name, "local.family.defs"))]
    assert sorted(order) == sorted(genera)
    inputs = lambda f: [str(base / g / "fasta_by_function" / f) for g in order]  # noqa: E731
    want = {f: expected_lines(env, inputs(f)) for f in "01234"}
    assert want["2"] is None and all(len(want[f]) > 10 for f in "0134")

    p = run(MERGE, env.data, str(base), str(out), "0", "1", "2", "3", "4", "--verbose")
    assert sorted(os.listdir(out)) == ["0", "1", "3", "4"]
    for f in "0134":
        assert file_lines(out / f) == want[f], f
    assert f'Skip compute "{inputs("2")[0]}"\n' in p.stderr
    assert ",".join(p for p in inputs("1") if os.path.isfile(p)) + " Start all to all comparison\n" in p.stderr

    # no ids: every function index is tried, files only for the families that have input
    assert len(env.funcs) > 5
    out2 = tmp_path / "out2"
    out2.mkdir()
    p = run(MERGE, "--verbose", env.data, str(base), str(out2), "--batch-windows", "2000")
    assert sorted(os.listdir(out2)) == ["0", "1", "3", "4"]
    for f in "0134":
        assert (out2 / f).read_bytes() == (out / f).read_bytes(), f
    assert p.stderr.count("Skip compute ") == len(env.funcs) - 4
    assert f'Skip compute "{inputs(str(len(env.funcs) - 1))[0]}"\n' in p.stderr
