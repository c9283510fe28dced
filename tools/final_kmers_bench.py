"""Measurements of final.kmers written from the resident arena (skm_build_write_final_kmers,
kmers-build-signatures --final-kmers-source device) against the host writer it stands beside
(skm_build_finish + the CLI's write_final_kmers), on the C2 tree (1 M proteins as FASTA
directories from synth.write_dirs_parallel).

  cli          bin/kmers-build-signatures with --final-kmers-source host and device, both with
               --recall-db device and --perfect-hash-source device (so the device mode holds no host
               copy of the kept set and the host mode holds it for final.kmers alone); a warm-up of
               each, then the modes alternating for --repeats timed repeats.  Per mode: the wall of
               the process, the `finish` and `final_kmers` phases and kept_host_bytes of its
               "phases:" line, and the child's peak resident set (ru_maxrss of that child alone, from
               wait4).  final.kmers of the two modes compared byte for byte.
  in_process   SignatureBuilder.write_final_kmers on the same proteins, once to a file (its file
               system is named) and once to /dev/null, which separates sort + format + D2H from the
               file system; the statistics of both calls as returned.

Every repeated figure is reported as mean, standard deviation and [min, max].  No threshold: the
yardstick is the host mode of the same binary.  Writes --out (default
profiles/final_kmers_ab.json), stamped with bench.src_sha16().

usage: python tools/final_kmers_bench.py [--seqs 1000000] [--families 4000] [--per-file 4000]
                                         [--repeats 5] [--threads 16] [--tmp DIR] [--out FILE] [--section NAME]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def stats(xs):
    xs = [float(x) for x in xs]
    return {"mean": statistics.fmean(xs), "stdev": statistics.stdev(xs) if len(xs) > 1 else 0.0, "min": min(xs),
            "max": max(xs), "all": xs}


def phases_of(stderr: str) -> dict:
    line = [ln for ln in stderr.splitlines() if ln.startswith("phases: ")][-1].split()
    return {line[i]: float(line[i + 1]) for i in range(1, len(line) - 1, 2)}


def file_system_of(path: str) -> str:
    """The type of the file system that holds path (the longest mount point that is a prefix)."""
    path = os.path.realpath(path)
    best, kind = "", "unknown"
    try:
        with open("/proc/self/mounts") as fh:
            for ln in fh:
                f = ln.split()
                if len(f) >= 3 and (path == f[1] or path.startswith(f[1].rstrip("/") + "/")) and len(f[1]) >= len(best):
                    best, kind = f[1], f[2]
    except OSError:
        pass
    return kind


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seqs", type=int, default=1_000_000)
    ap.add_argument("--families", type=int, default=4000)
    ap.add_argument("--per-file", type=int, default=4000)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--tmp", default=None, help="directory for the input tree and the outputs (default: the system's)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "final_kmers_ab.json"))
    ap.add_argument("--section", default=None)
    a = ap.parse_args()
    assert a.repeats >= 5, "at least five alternating repeats"

    import bench
    import signature_kmers_amd as skm
    from signature_kmers_amd import synth
    if skm.device_count() < 1:
        raise SystemExit("no HIP device: nothing is measured without one")

    with tempfile.TemporaryDirectory(dir=a.tmp) as tmp:
        info = synth.write_dirs_parallel(os.path.join(tmp, "in"), a.seqs, a.families, per_file=a.per_file,
                                         workers=a.threads)
        exe = os.path.join(ROOT, "bin", "kmers-build-signatures")
        outs = {m: os.path.join(tmp, "kd_" + m) for m in ("host", "device")}

        def cli(mode):
            cmd = [exe, "-D", info["ann_dir"], "-F", info["seqs_dir"], "--kmer-data-dir", outs[mode],
                   "--final-kmers", "final.kmers", "--perfect-hash", "kmer_data.mph", "--perfect-hash-data",
                   "kmer_data.dat", "--n-threads", str(a.threads), "--recall-db", "device", "--perfect-hash-source",
                   "device", "--final-kmers-source", mode]
            with open(os.path.join(tmp, "stdout"), "wb") as so, open(os.path.join(tmp, "stderr"), "wb") as se:
                t = time.perf_counter()
                pr = subprocess.Popen(cmd, stdout=so, stderr=se)
                _, status, ru = os.wait4(pr.pid, 0)  # this child's own rusage
                wall = time.perf_counter() - t
            pr.returncode = os.waitstatus_to_exitcode(status)
            err = open(os.path.join(tmp, "stderr"), errors="replace").read()
            if pr.returncode != 0:
                raise SystemExit(f"kmers-build-signatures --final-kmers-source {mode} failed: {err[-2000:]}")
            return wall, phases_of(err), ru.ru_maxrss * 1024  # Linux: kilobytes

        for m in outs:
            cli(m)
        res = {m: {"wall": [], "finish": [], "final_kmers": [], "total": [], "rss": [], "kept_host_bytes": []} for m in outs}
        for _ in range(a.repeats):
            for m in outs:
                wall, ph, rss = cli(m)
                res[m]["wall"].append(wall)
                res[m]["finish"].append(ph["finish"])
                res[m]["final_kmers"].append(ph["final_kmers"])
                res[m]["total"].append(ph["total"])
                res[m]["rss"].append(rss)
                res[m]["kept_host_bytes"].append(ph["kept_host_bytes"])
        fk = {m: os.path.join(outs[m], "final.kmers") for m in outs}
        same = open(fk["host"], "rb").read() == open(fk["device"], "rb").read()
        section = {
            "workload": {"proteins": a.seqs, "files": len(info["files"]), "repeats": a.repeats, "threads": a.threads,
                         "final_kmers_bytes": os.path.getsize(fk["device"]),
                         "other_sources": "--recall-db device --perfect-hash-source device in both modes",
                         "output_file_system": file_system_of(tmp)},
            "cli_kmers_build_signatures": {
                m: {"process_wall_s": stats(v["wall"]), "finish_phase_s": stats(v["finish"]),
                    "final_kmers_phase_s": stats(v["final_kmers"]), "total_phase_s": stats(v["total"]),
                    "child_peak_rss_bytes": stats(v["rss"]), "kept_host_bytes": int(v["kept_host_bytes"][0])}
                for m, v in res.items()},
        }
        c = section["cli_kmers_build_signatures"]
        c["final_kmers_identical"] = same
        c["peak_rss_host_minus_device_bytes"] = c["host"]["child_peak_rss_bytes"]["mean"] - \
            c["device"]["child_peak_rss_bytes"]["mean"]

        # in process: the call's own statistics, to a file and to /dev/null
        p = synth.generate_arrays(a.seqs, a.families, per_file=a.per_file)
        r, o, l, f, i, funcs = synth.build_inputs(p)
        b = skm.SignatureBuilder(len(funcs))
        b.add_batch(r, o, l, f, i)
        b.run()
        del p, r, o, l, f, i
        target = os.path.join(tmp, "in_process.kmers")
        b.write_final_kmers("/dev/null")  # warm-up (pinned allocations, first launches)
        st_file = b.write_final_kmers(target)
        st_null = b.write_final_kmers("/dev/null")
        t = time.perf_counter()
        kept = b.finish()
        finish_s = time.perf_counter() - t
        n = len(kept.keys)
        # the file against the host formatter over finish()'s arrays of the same handle (the CLI's
        # files number the functions through its FunctionMap, so they are not comparable with it)
        same_in_process = open(target, "rb").read() == skm.final_kmers_host(kept.keys, kept.data)
        del kept
        b.close()
        section["in_process"] = {
            "kept_kmers": n, "to_file": st_file, "to_dev_null": st_null, "file_system": file_system_of(target),
            "file_equals_host_formatter_over_finish": same_in_process,
            "finish_s_same_handle": finish_s,
            "c3": "not measured at C3",
        }

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
    if not same:
        raise SystemExit("final.kmers differs between the modes")
    if not same_in_process:
        raise SystemExit("the in-process final.kmers differs from the host formatter over finish()")


if __name__ == "__main__":
    main()
