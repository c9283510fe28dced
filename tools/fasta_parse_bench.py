"""Measurements of the device FASTA parse (skm_annotate_fasta, kmers-call-functions --fasta-parse
device) against the host parse path it stands beside (parse_fasta_files + annotate_batch ->
skm_annotate), on FASTA files from synth.write_dirs_parallel.

One process, the files read into memory first, a warm-up of each path, then the paths alternating
for --repeats timed repeats:

  in_process   library calls on one DB, host clock around calls that end in a device synchronise:
               annotate_arrays  FunctionCaller.process_seqs on the files' records already parsed and
                                packed (upload of the residues + device pipeline + calls download).
                                The host parse and the front end's packing copy are NOT in it: the
                                library has no Python binding of the host parser.  They are in the
                                CLI's phases below.
               annotate_fasta   FunctionCaller.process_fasta on the raw bytes (upload of the bytes +
                                device parse + device pipeline + table and calls download)
               parse_device_ms  the parse's own device time (skm_fasta_table.parse_ms)
               and the calls of the two paths compared byte for byte.
  cli          bin/kmers-call-functions on the same directory with --fasta-parse host and device,
               alternating: the wall of the process, and the busy seconds of the parse and device
               stages from its "phases:" line (host: parse = read + full host parse, device =
               packing copy + skm_annotate; device: parse = read + headers-only host parse, device =
               skm_annotate_fasta + the check against the host's lengths); output files compared.

Every figure is reported as mean, standard deviation and [min, max] over the repeats.  Writes
--out (default profiles/fasta_parse_ab.json), stamped with bench.src_sha16().

usage: python tools/fasta_parse_bench.py [--seqs 1000000] [--families 4000] [--per-file 4000]
                                         [--repeats 5] [--threads 16] [--out FILE] [--section NAME]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def stats(xs):
    xs = [float(x) for x in xs]
    return {"mean": statistics.fmean(xs), "stdev": statistics.stdev(xs) if len(xs) > 1 else 0.0, "min": min(xs),
            "max": max(xs), "all": xs}


def phases_of(stderr: str) -> dict:
    line = [ln for ln in stderr.splitlines() if ln.startswith("phases: ")][-1].split()
    return {line[i]: float(line[i + 1]) for i in range(1, len(line) - 1, 2)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seqs", type=int, default=1_000_000)
    ap.add_argument("--families", type=int, default=4000)
    ap.add_argument("--per-file", type=int, default=4000)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fasta_parse_ab.json"))
    ap.add_argument("--section", default=None)
    a = ap.parse_args()
    assert a.repeats >= 5, "at least five alternating repeats"

    import bench
    import signature_kmers_amd as skm
    from signature_kmers_amd import synth
    if skm.device_count() < 1:
        raise SystemExit("no HIP device: nothing is measured without one")

    with tempfile.TemporaryDirectory() as tmp:
        info = synth.write_dirs_parallel(os.path.join(tmp, "in"), a.seqs, a.families, per_file=a.per_file,
                                         workers=a.threads)
        paths = [os.path.join(info["seqs_dir"], g) for g in info["files"]]
        # the DB of the same proteins, built and opened on the device; its files for the CLI
        p = synth.generate_arrays(a.seqs, a.families, per_file=a.per_file)
        r, o, l, f, i, funcs = synth.build_inputs(p)
        kd = os.path.join(tmp, "kd")
        os.makedirs(kd)
        b = skm.SignatureBuilder(len(funcs))
        b.add_batch(r, o, l, f, i)
        b.run()
        db = b.mph_db(release_work=True, mph_path=os.path.join(kd, "kmer_data.mph"),
                      dat_path=os.path.join(kd, "kmer_data.dat"))
        b.close()
        del p, r, o, l, f, i
        with open(os.path.join(kd, "function.index"), "w") as fh:
            for k, name in enumerate(funcs):
                fh.write(f"{k}\t{name}\n")
        caller = skm.FunctionCaller(db, funcs)

        blobs = [open(q, "rb").read() for q in paths]
        data = np.frombuffer(b"".join(blobs), dtype=np.uint8)
        foff = np.zeros(len(blobs) + 1, np.uint64)
        foff[1:] = np.cumsum([len(x) for x in blobs], dtype=np.uint64)
        del blobs
        # the host path's input: the records parsed and packed (one 0 after each), as annotate_batch
        # hands them to skm_annotate
        tab = skm.fasta_parse_device((data, foff), want_residues=True)
        seq_len = tab.seq_len
        seq_off = np.zeros(len(seq_len), np.uint64)
        seq_off[1:] = np.cumsum(seq_len[:-1].astype(np.uint64) + 1)
        residues = tab.residues

        def arrays():
            t = time.perf_counter()
            out = caller.process_seqs(residues, seq_off, seq_len)
            return time.perf_counter() - t, out, 0.0

        def fasta():
            t = time.perf_counter()
            out = caller.process_fasta((data, foff))
            return time.perf_counter() - t, out[3:], caller.last_fasta.parse_ms

        want = arrays()[1]  # warm-up of each path, and the results compared
        got = fasta()[1]
        same = bool(np.array_equal(want[0], got[0]) and want[1].tobytes() == got[1].tobytes())
        t_arr, t_fa, ms = [], [], []
        for _ in range(a.repeats):
            t_arr.append(arrays()[0])
            dt, _, pm = fasta()
            t_fa.append(dt)
            ms.append(pm)
        section = {
            "workload": {"proteins": int(tab.n_recs), "files": len(paths), "fasta_bytes": int(len(data)),
                         "residues": int(tab.n_residues), "query_windows": int(tab.n_windows), "repeats": a.repeats},
            "in_process": {"annotate_arrays_s": stats(t_arr), "annotate_fasta_s": stats(t_fa),
                           "parse_device_ms": stats(ms), "calls_identical": same,
                           "note": "annotate_arrays excludes the host parse and the packing copy (see cli)"},
        }
        db.close()

        # the CLI in both modes on the same directory, alternating after a warm-up of each
        exe = os.path.join(ROOT, "bin", "kmers-call-functions")
        outs = {m: os.path.join(tmp, f"calls.{m}") for m in ("host", "device")}

        def cli(mode):
            t = time.perf_counter()
            pr = subprocess.run([exe, kd] + paths + ["-o", outs[mode], "-j", str(a.threads), "--fasta-parse", mode],
                                capture_output=True, text=True)
            wall = time.perf_counter() - t
            if pr.returncode != 0:
                raise SystemExit(f"kmers-call-functions --fasta-parse {mode} failed: {pr.stderr[-2000:]}")
            return wall, phases_of(pr.stderr)

        for m in outs:
            cli(m)
        res = {m: {"wall": [], "parse": [], "device": [], "pipeline_wall": []} for m in outs}
        for _ in range(a.repeats):
            for m in outs:
                wall, ph = cli(m)
                res[m]["wall"].append(wall)
                res[m]["parse"].append(ph["parse"])
                res[m]["device"].append(ph["device"])
                res[m]["pipeline_wall"].append(ph["wall"])
        section["cli_kmers_call_functions"] = {
            m: {"process_wall_s": stats(v["wall"]), "parse_stage_busy_s": stats(v["parse"]),
                "device_stage_busy_s": stats(v["device"]), "pipeline_wall_s": stats(v["pipeline_wall"])}
            for m, v in res.items()}
        section["cli_kmers_call_functions"]["outputs_identical"] = \
            open(outs["host"], "rb").read() == open(outs["device"], "rb").read()
        section["cli_kmers_call_functions"]["threads"] = a.threads

    section["src_sha16"] = bench.src_sha16()
    name = a.section or f"seqs_{a.seqs}"
    out = {}
    if os.path.exists(a.out):
        with open(a.out) as fh:
            out = json.load(fh)
    out[name] = section
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")
    print(json.dumps({name: section}), flush=True)


if __name__ == "__main__":
    main()
