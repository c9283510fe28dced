"""Measurements of the build's input from FASTA bytes (skm_build_add_fasta, kmers-build-signatures
--fasta-parse device) against the host path it stands beside (the host parse of the sequence
bodies + skm_build_add_batch), on the C2 tree (1 M proteins as FASTA directories from
synth.write_dirs_parallel).  Both legs run to a finished prepare, with the device idle at the start.

  in_process   one process, a new SignatureBuilder per repeat (its creation is not timed), the two
               paths alternating after a warm-up of each:
                 arrays  add_batch over the files' records as arrays + prepare -- the parent's code
                         path from the point where the host parse has produced its arrays, WITHOUT
                         that parse (the parser is the CLI's front end, not the library's), with its
                         add_pack_us / add_dma_wait_us counters;
                 fasta   add_fasta over the files' bytes in groups of --group-mb + prepare, with its
                         add_fasta_us counter (the parse's device time) and the bytes/s that gives.
               The resident input of the two is compared once (debug_input).
  cli          bin/kmers-build-signatures --recall-source device with --fasta-parse host and device,
               alternating after a warm-up of each: the phases parse_files (the host parser's
               threads: the whole parse, or headers only), parse, add, prepare of the "phases:" line,
               their sum to a finished prepare, and add_fasta / host_residue_bytes of the device mode.
               This is where the host parse times come from: the parser is the CLI's front end.

Every repeated figure is reported as median, mean and [min, max].  No threshold: the yardstick is
the host path in the same process / the same binary.  C3 is not measured.  Writes --out (default
profiles/build_fasta_ab.json), stamped with bench.src_sha16().

usage: python tools/build_fasta_bench.py [--seqs 1000000] [--families 4000] [--per-file 4000] [--repeats 5]
                                         [--cli-repeats 3] [--group-mb 256] [--threads 16] [--tmp DIR] [--out FILE]
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
    return {"median": statistics.median(xs), "mean": statistics.fmean(xs), "min": min(xs), "max": max(xs), "all": xs}


def phases_of(stderr: str) -> dict:
    line = [ln for ln in stderr.splitlines() if ln.startswith("phases: ")][-1].split()
    return {line[i]: float(line[i + 1]) for i in range(1, len(line) - 1, 2)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seqs", type=int, default=1_000_000)
    ap.add_argument("--families", type=int, default=4000)
    ap.add_argument("--per-file", type=int, default=4000)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--cli-repeats", type=int, default=3)
    ap.add_argument("--group-mb", type=float, default=256)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--tmp", default=None, help="directory for the input tree and the outputs (default: the system's)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "build_fasta_ab.json"))
    ap.add_argument("--section", default=None)
    a = ap.parse_args()

    import bench
    import signature_kmers_amd as skm
    from signature_kmers_amd import synth
    if skm.device_count() < 1:
        raise SystemExit("no HIP device: nothing is measured without one")

    with tempfile.TemporaryDirectory(dir=a.tmp) as tmp:
        info = synth.write_dirs_parallel(os.path.join(tmp, "in"), a.seqs, a.families, per_file=a.per_file,
                                         workers=a.threads)
        p = synth.generate_arrays(a.seqs, a.families, per_file=a.per_file)
        _, _, _, f, i, funcs = synth.build_inputs(p)  # the records' functions and ids
        del p
        # the files' bytes in groups of whole files, each with its records' rec_func / rec_id
        groups, cur, cur_bytes, rec = [], [], 0, 0
        budget = int(a.group_mb * (1 << 20))
        n_file = [min(a.per_file, a.seqs - k * a.per_file) for k in range(len(info["files"]))]
        for g, n in zip(info["files"], n_file):
            with open(os.path.join(info["seqs_dir"], g), "rb") as fh:
                blob = fh.read()
            if cur and cur_bytes + len(blob) > budget:
                groups.append(cur)
                cur, cur_bytes = [], 0
            cur.append((blob, rec, rec + n))
            cur_bytes += len(blob)
            rec += n
        groups.append(cur)
        assert rec == len(f)
        packed = []
        for grp in groups:
            data = np.frombuffer(b"".join(b for b, _, _ in grp), np.uint8)
            off = np.zeros(len(grp) + 1, np.uint64)
            off[1:] = np.cumsum([len(b) for b, _, _ in grp], dtype=np.uint64)
            packed.append(((data, off), f[grp[0][1]:grp[-1][2]], i[grp[0][1]:grp[-1][2]]))
        total_bytes = int(sum(len(d[0][0]) for d in packed))
        del groups
        # the arrays leg's input: the files' own records (what the host parse hands to add_batch),
        # taken once from the device parser, which the tests pin against the reference's
        rs, ls = [], []
        for blobs, _, _ in packed:
            tab = skm.fasta_parse_device(blobs, want_residues=True)
            rs.append(tab.residues)
            ls.append(tab.seq_len)
        r, l = np.concatenate(rs), np.concatenate(ls)
        assert len(l) == len(f)
        o = np.zeros(len(l), np.uint64)
        base, at = 0, 0
        for x, y in zip(rs, ls):  # record s of a group at sum over t < s of (len[t] + 1)
            o[at:at + len(y)] = base + np.concatenate([[0], np.cumsum(y[:-1].astype(np.uint64) + np.uint64(1))])
            base += len(x)
            at += len(y)
        del rs, ls

        def leg(kind, keep=False):
            skm.warm_device(0)  # the device idle at the start
            b = skm.SignatureBuilder(len(funcs))
            b.reserve(len(r), len(l))  # as the CLI reserves before its first add (not timed there either)
            t0 = time.perf_counter()
            if kind == "arrays":
                b.add_batch(r, o, l, f, i)
            else:
                for blobs, gf, gi in packed:
                    tab = b.add_fasta(blobs, gf, gi)
                    assert tab.n_recs == len(gf)
            t1 = time.perf_counter()
            b.prepare()
            t2 = time.perf_counter()
            c = b.counters()
            got = b.debug_input() if keep else None
            b.close()
            return {"add_s": t1 - t0, "prepare_s": t2 - t1, "to_prepared_s": t2 - t0, "add_pack_us": c["add_pack_us"],
                    "add_dma_wait_us": c["add_dma_wait_us"], "add_fasta_us": c["add_fasta_us"],
                    "add_batch_us": c["add_batch_us"]}, got

        _, in_a = leg("arrays", keep=True)
        _, in_f = leg("fasta", keep=True)
        same_input = in_a[0].tobytes() == in_f[0].tobytes() and in_a[1].tobytes() == in_f[1].tobytes()
        resident_bytes = len(in_a[0])
        del in_a, in_f
        res = {"arrays": [], "fasta": []}
        for _ in range(a.repeats):
            for kind in res:
                res[kind].append(leg(kind)[0])
        in_process = {k: {name: stats([x[name] for x in v]) for name in v[0]} for k, v in res.items()}
        us = in_process["fasta"]["add_fasta_us"]["median"]
        in_process["fasta"]["device_parse_bytes_per_s"] = total_bytes / (us * 1e-6) if us else 0.0
        in_process["resident_input_identical"] = same_input
        # (not an end-to-end figure: the arrays leg has no host parse in it; the cli section has)
        in_process["ratio_arrays_without_host_parse_over_fasta_to_prepared"] = \
            in_process["arrays"]["to_prepared_s"]["median"] / in_process["fasta"]["to_prepared_s"]["median"]
        del packed, r, o, l, f, i

        exe = os.path.join(ROOT, "bin", "kmers-build-signatures")

        def cli(mode):
            out = os.path.join(tmp, "kd_" + mode)
            cmd = [exe, "-D", info["ann_dir"], "-F", info["seqs_dir"], "--kmer-data-dir", out, "--n-threads", str(a.threads),
                   "--recall-source", "device", "--recall-db", "device", "--fasta-parse", mode, "--fasta-group-mb",
                   str(a.group_mb)]
            pr = subprocess.run(cmd, capture_output=True)
            if pr.returncode != 0:
                raise SystemExit(f"kmers-build-signatures --fasta-parse {mode} failed: {pr.stderr.decode()[-2000:]}")
            ph = phases_of(pr.stderr.decode(errors="replace"))
            ph["to_prepared"] = ph["parse"] + ph["add"] + ph["prepare"]
            return ph

        cli_res = {"host": [], "device": []}
        if a.cli_repeats:
            for m in cli_res:
                cli(m)
            for _ in range(a.cli_repeats):
                for m in cli_res:
                    cli_res[m].append(cli(m))
        names = ("parse_files", "parse", "add", "prepare", "to_prepared", "total", "add_fasta", "host_residue_bytes")
        cli_out = {m: {n: stats([x[n] for x in v]) for n in names if v and n in v[0]} for m, v in cli_res.items()}
        if a.cli_repeats:  # the end-to-end figure: host parse + add_batch + prepare against headers-only + add_fasta + prepare
            cli_out["device_faster_to_prepared"] = \
                cli_out["device"]["to_prepared"]["median"] < cli_out["host"]["to_prepared"]["median"]

    section = {
        "workload": {"proteins": a.seqs, "files": len(info["files"]), "fasta_bytes": total_bytes,
                     "resident_bytes": resident_bytes, "group_mb": a.group_mb, "repeats": a.repeats,
                     "cli_repeats": a.cli_repeats, "threads": a.threads},
        "in_process": in_process,
        "cli_kmers_build_signatures": cli_out,
        "c3": "not measured at C3",
        "src_sha16": bench.src_sha16(),
    }
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
    if not same_input:
        raise SystemExit("the resident input differs between add_batch and add_fasta")


if __name__ == "__main__":
    main()
