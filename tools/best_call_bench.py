"""Measurements of the batched best call (skm_best_calls_host, skm_annotate_best,
kmers-call-functions --best-call device) against the paths it stands beside, on FASTA files from
synth.write_dirs_parallel and the DB of the same proteins.  The method of tools/fasta_parse_bench.py:
one process, a warm-up of each path, then the paths alternating for --repeats timed repeats.

  in_process   library calls on one DB, host clock around calls that end in a device synchronise:
               calls_then_host   FunctionCaller.process_seqs (upload + device pipeline + download of
                                 the calls) followed by best_calls_host on --threads threads
               best_seqs         FunctionCaller.best_seqs (upload + device pipeline + the best-call
                                 kernel + download of 16 B per sequence)
               python_loop       for reference, the per-sequence ctypes loop over find_best_call on a
                                 10,000-sequence sample, SCALED to the whole batch (labelled scaled)
               and the results of the two batch paths compared byte for byte.
  kernel       the best-call kernel's own device ms per batch, and the bytes that come back per batch
               in both modes (host: 24 B per call + 8 B per sequence + 8; device: 16 B per sequence)
  cli          bin/kmers-call-functions on the same directory with --best-call host and device,
               alternating: the wall of the process, and the busy seconds of the device and
               best_call stages from its "phases:" line; output files compared.

Every figure is mean, standard deviation and [min, max] over the repeats.  Writes --out (default
profiles/best_call_ab.json), stamped with bench.src_sha16().

usage: python tools/best_call_bench.py [--seqs 1000000] [--families 4000] [--per-file 4000]
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "best_call_ab.json"))
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
        print("inputs written", flush=True)
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
        print("DB built", flush=True)
        caller = skm.FunctionCaller(db, funcs)
        host_tables = skm.FunctionIndexTables(funcs, device=-1)
        caller.tables()

        blobs = [open(q, "rb").read() for q in paths]
        data = np.frombuffer(b"".join(blobs), dtype=np.uint8)
        foff = np.zeros(len(blobs) + 1, np.uint64)
        foff[1:] = np.cumsum([len(x) for x in blobs], dtype=np.uint64)
        del blobs
        tab = skm.fasta_parse_device((data, foff), want_residues=True)
        seq_len = tab.seq_len
        seq_off = np.zeros(len(seq_len), np.uint64)
        seq_off[1:] = np.cumsum(seq_len[:-1].astype(np.uint64) + 1)
        residues = tab.residues
        del data

        def host_path():
            t = time.perf_counter()
            off, calls = caller.process_seqs(residues, seq_off, seq_len)
            t1 = time.perf_counter()
            best = skm.best_calls_host(off, calls, host_tables, n_threads=a.threads)
            t2 = time.perf_counter()
            return t2 - t, t1 - t, t2 - t1, best, (off, calls)

        def device_path():
            t = time.perf_counter()
            best = caller.best_seqs(residues, seq_off, seq_len)
            return time.perf_counter() - t, best

        _, _, _, want, (off, calls) = host_path()  # warm-up of each path, and the results compared
        _, got = device_path()
        same = want.best.tobytes() == got.best.tobytes()
        n_seqs, n_calls = int(want.n_seqs), int(want.n_calls)
        # the per-sequence Python loop a caller had to write before, on a sample
        ns = min(10_000, n_seqs)
        t = time.perf_counter()
        for s in range(ns):
            caller.find_best_call(calls[int(off[s]):int(off[s + 1])])
        loop_s = time.perf_counter() - t
        del off, calls
        t_host, t_annot, t_bhost, t_dev, k_ms = [], [], [], [], []
        for _ in range(a.repeats):
            th, ta, tb, _, _ = host_path()
            t_host.append(th)
            t_annot.append(ta)
            t_bhost.append(tb)
            td, best = device_path()
            t_dev.append(td)
            k_ms.append(best.kernel_ms)
        print("in-process done", flush=True)
        section = {
            "workload": {"proteins": n_seqs, "files": len(paths), "calls": n_calls, "residues": int(tab.n_residues),
                         "query_windows": int(tab.n_windows), "repeats": a.repeats, "threads": a.threads,
                         "functions": len(funcs)},
            "in_process": {"calls_then_host_s": stats(t_host), "of_it_process_seqs_s": stats(t_annot),
                           "of_it_best_calls_host_s": stats(t_bhost), "best_seqs_s": stats(t_dev),
                           "results_identical": bool(same), "n_deferred": int(got.n_deferred),
                           "python_loop_scaled_s": loop_s / ns * n_seqs,
                           "python_loop_note": f"scaled from {ns} sequences ({loop_s:.3f} s), not measured on the whole batch"},
            "kernel": {"best_call_kernel_ms": stats(k_ms),
                       "download_bytes_host_mode": 24 * n_calls + 8 * (n_seqs + 1) + 8,
                       "download_bytes_device_mode": 16 * n_seqs},
        }
        db.close()

        exe = os.path.join(ROOT, "bin", "kmers-call-functions")
        outs = {m: os.path.join(tmp, f"calls.{m}") for m in ("host", "device")}

        def cli(mode):
            t = time.perf_counter()
            pr = subprocess.run([exe, kd] + paths + ["-o", outs[mode], "-j", str(a.threads), "--best-call", mode],
                                capture_output=True, text=True)
            wall = time.perf_counter() - t
            if pr.returncode != 0:
                raise SystemExit(f"kmers-call-functions --best-call {mode} failed: {pr.stderr[-2000:]}")
            return wall, phases_of(pr.stderr)

        for m in outs:
            cli(m)
        res = {m: {"wall": [], "device": [], "best_call": [], "pipeline_wall": [], "deferred": []} for m in outs}
        for _ in range(a.repeats):
            for m in outs:
                wall, ph = cli(m)
                res[m]["wall"].append(wall)
                res[m]["device"].append(ph["device"])
                res[m]["best_call"].append(ph["best_call"])
                res[m]["pipeline_wall"].append(ph["wall"])
                res[m]["deferred"].append(ph["deferred"])
        section["cli_kmers_call_functions"] = {
            m: {"process_wall_s": stats(v["wall"]), "device_stage_busy_s": stats(v["device"]),
                "best_call_stage_busy_s": stats(v["best_call"]), "pipeline_wall_s": stats(v["pipeline_wall"]),
                "deferred": int(v["deferred"][-1])}
            for m, v in res.items()}
        section["cli_kmers_call_functions"]["outputs_identical"] = \
            open(outs["host"], "rb").read() == open(outs["device"], "rb").read()

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
