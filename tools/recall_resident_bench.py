"""Measurements of the recall pass over a build's resident sequences (skm_build_recall,
kmers-build-signatures --recall-source device) against the path it stands beside, which packs
and uploads every training protein a second time; on the C2 size (1 M proteins), one MI355X.

  in_process   SignatureBuilder.recall(db, tables) against FunctionCaller.best_seqs over the same
               proteins from host arrays, the DB being kept_db() of the same build; a warm-up of
               each path, then the paths alternating for --repeats timed repeats.  Per path the wall
               time of the call; for the resident path also its device time (view + lookup + calls +
               best, skm_recall_stats).  The two results compared byte for byte.
  cli          bin/kmers-build-signatures with --recall-source host and device, both with
               --recall-db device --perfect-hash-source device --final-kmers-source device; a warm-up
               of each, then the modes alternating.  Per mode: the wall of the process, the `recall`
               and `recall_device` phases of its "phases:" line, and the child's peak resident set
               (ru_maxrss of that child alone, from wait4).  Every output file of the two modes
               compared byte for byte.

Every repeated figure is reported as mean, standard deviation and [min, max].  No threshold: the
yardstick is the host mode of the same binary.  Writes --out (default
profiles/recall_resident_ab.json), stamped with bench.src_sha16().

usage: python tools/recall_resident_bench.py [--seqs 1000000] [--families 4000] [--per-file 4000]
                                             [--repeats 5] [--threads 16] [--tmp DIR] [--out FILE] [--section NAME]
                                             [--skip-cli]
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


def tree_bytes(root):
    out = {}
    for d, _, names in os.walk(root):
        for n in names:
            p = os.path.join(d, n)
            with open(p, "rb") as fh:
                out[os.path.relpath(p, root)] = fh.read()
    return out


def run_in_process(a, skm, synth):
    p = synth.generate_arrays(a.seqs, a.families, per_file=a.per_file)
    r, o, l, f, i, funcs = synth.build_inputs(p)
    b = skm.SignatureBuilder(len(funcs))
    b.add_batch(r, o, l, f, i)
    b.run()
    db = b.kept_db()
    caller = skm.FunctionCaller(db, funcs)
    tables = caller.tables()
    t_up, t_res, dev_res = [], [], {k: [] for k in ("view_ms", "lookup_ms", "calls_ms", "best_ms")}
    last = {}
    for rep in range(a.repeats + 1):  # rep 0 is the warm-up of each path
        t0 = time.perf_counter()
        last["upload"] = caller.best_seqs(r, o, l)
        dt_up = time.perf_counter() - t0
        t0 = time.perf_counter()
        last["resident"] = b.recall(db, tables)
        dt_res = time.perf_counter() - t0
        if rep:
            t_up.append(dt_up)
            t_res.append(dt_res)
            for k in dev_res:
                dev_res[k].append(last["resident"].stats[k])
    equal = bool(np.array_equal(last["upload"].best.view(np.uint8), last["resident"].best.view(np.uint8)))
    st = last["resident"].stats
    sec = {
        "workload": {"proteins": int(len(l)), "kept_kmers": int(b.counters()["kept"]), "windows": int(st["n_windows"]),
                     "resident_bytes": int(st["resident_bytes"]), "batches": int(st["n_batches"]), "repeats": a.repeats},
        "wall_s": {"best_seqs_from_host_arrays": stats(t_up), "recall_resident": stats(t_res)},
        "recall_resident_device_ms": {k: stats(v) for k, v in dev_res.items()},
        "recall_resident_device_total_ms": stats([sum(v[j] for v in dev_res.values()) for j in range(a.repeats)]),
        "best_kernel_ms_upload_path": float(last["upload"].kernel_ms),
        "deferred": int(st["n_deferred"]),
        "results_equal": equal,
    }
    db.close()
    b.close()
    return sec, equal


def run_cli(a, synth, tmp):
    info = synth.write_dirs_parallel(os.path.join(tmp, "in"), a.seqs, a.families, per_file=a.per_file, workers=a.threads)
    exe = os.path.join(ROOT, "bin", "kmers-build-signatures")
    outs = {m: os.path.join(tmp, "kd_" + m) for m in ("host", "device")}

    def cli(mode):
        cmd = [exe, "-D", info["ann_dir"], "-F", info["seqs_dir"], "--kmer-data-dir", outs[mode], "--final-kmers",
               "final.kmers", "--perfect-hash", "kmer_data.mph", "--perfect-hash-data", "kmer_data.dat", "--n-threads",
               str(a.threads), "--recall-db", "device", "--perfect-hash-source", "device", "--final-kmers-source",
               "device", "--recall-source", mode]
        with open(os.path.join(tmp, "stdout_" + mode), "wb") as so, open(os.path.join(tmp, "stderr"), "wb") as se:
            t = time.perf_counter()
            pr = subprocess.Popen(cmd, stdout=so, stderr=se)
            _, status, ru = os.wait4(pr.pid, 0)  # this child's own rusage
            wall = time.perf_counter() - t
        err = open(os.path.join(tmp, "stderr"), errors="replace").read()
        if os.waitstatus_to_exitcode(status) != 0:
            raise SystemExit(f"kmers-build-signatures --recall-source {mode} failed: {err[-2000:]}")
        return wall, phases_of(err), ru.ru_maxrss * 1024  # Linux: kilobytes

    for m in outs:
        cli(m)
    keys = ("wall", "recall", "recall_device", "total", "rss")
    res = {m: {k: [] for k in keys} for m in outs}
    ph = {}
    for _ in range(a.repeats):
        for m in outs:
            wall, ph[m], rss = cli(m)
            res[m]["wall"].append(wall)
            res[m]["recall"].append(ph[m]["recall"])
            res[m]["recall_device"].append(ph[m]["recall_device"])
            res[m]["total"].append(ph[m]["total"])
            res[m]["rss"].append(rss)
    same_files = tree_bytes(outs["host"]) == tree_bytes(outs["device"])
    same_stdout = open(os.path.join(tmp, "stdout_host"), "rb").read() == open(os.path.join(tmp, "stdout_device"), "rb").read()
    sec = {
        "workload": {"proteins": a.seqs, "files": len(info["files"]), "repeats": a.repeats, "threads": a.threads,
                     "other_sources": "--recall-db device --perfect-hash-source device --final-kmers-source device "
                                      "in both modes"},
        "modes": {m: {"process_wall_s": stats(v["wall"]), "recall_phase_s": stats(v["recall"]),
                      "recall_device_phase_s": stats(v["recall_device"]), "total_phase_s": stats(v["total"]),
                      "child_peak_rss_bytes": stats(v["rss"]),
                      "recall_resident_seqs": int(ph[m].get("recall_resident_seqs", 0)),
                      "recall_uploaded_seqs": int(ph[m].get("recall_uploaded_seqs", 0)),
                      "recall_batches": int(ph[m].get("recall_batches", 0))} for m, v in res.items()},
        "output_files_identical": same_files,
        "stdout_identical": same_stdout,
    }
    return sec, same_files and same_stdout


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seqs", type=int, default=1_000_000)
    ap.add_argument("--families", type=int, default=4000)
    ap.add_argument("--per-file", type=int, default=4000)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--tmp", default=None, help="directory for the input tree and the outputs (default: the system's)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "recall_resident_ab.json"))
    ap.add_argument("--section", default=None)
    ap.add_argument("--skip-cli", action="store_true", help="the in-process comparison only")
    a = ap.parse_args()
    assert a.repeats >= 5, "at least five alternating repeats"

    import bench
    import signature_kmers_amd as skm
    from signature_kmers_amd import synth
    if skm.device_count() < 1:
        raise SystemExit("no HIP device: nothing is measured without one")
    skm.warm_device(0)
    section, ok = {}, True
    section["in_process"], same = run_in_process(a, skm, synth)
    ok = ok and same
    if not a.skip_cli:
        with tempfile.TemporaryDirectory(dir=a.tmp) as tmp:
            section["cli_kmers_build_signatures"], same = run_cli(a, synth, tmp)
        ok = ok and same
    section["src_sha16"] = bench.src_sha16()
    name = a.section or ("c2" if a.seqs == 1_000_000 else f"seqs_{a.seqs}")
    res = {}
    if os.path.exists(a.out):
        with open(a.out) as fh:
            res = json.load(fh)
    res[name] = section
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")
    print(json.dumps({name: section}), flush=True)
    if not ok:
        sys.exit("the two paths' results differ")


if __name__ == "__main__":
    main()
