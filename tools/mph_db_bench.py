"""Measurements of the BDZ signature DB built and opened on the device from a finished build
(skm_build_mph_db) against the host path it stands beside (skm_build_finish +
skm_mph_build_device + skm_db_open).

  --c2   1 M proteins (the inputs of tests/test_gpu_scale.py's c2), one process: seconds from a
         finished run to an open BDZ DB by
           host          finish() + mph_build_device(files) + CmphKmerDb(files)   (the yardstick)
           device_files  mph_db(mph_path, dat_path)
           device        mph_db()
         each path once as a warm-up, then the paths alternating for --repeats timed repeats;
         mean, standard deviation, min and max of each, the phase times of the builders, the files
         of the two writing paths compared byte for byte, the lookups of the three DBs compared
         over a sample of the kept set, one mph_db(verify=True) outside the timing, and the plan's
         numbers beside the free device memory before and after.
  --c3   50 M proteins on one GPU (bench.py's generator): mph_db(release_work=True, verify=True)
         with no files -- its seconds and phase times, the free device memory before and after,
         and skm_mph_db_plan's [2] / [3] beside what was observed.

Each mode writes its own section of --out (default profiles/mph_db_ab.json, kept if the other
section is already there), stamped with bench.src_sha16().

usage: python tools/mph_db_bench.py --c2 [--repeats 5] | --c3 [--seqs 50000000] [--out FILE] [--tmp DIR]
"""
import argparse
import hashlib
import os
import shutil
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from kept_db_bench import stats, write_section  # noqa: E402

SEED = 1
PHASES = ("upload_s", "peel_s", "assign_s", "rank_s", "place_s", "verify_s", "write_s", "total_s")


def sha(path):
    h = hashlib.sha256()
    with open(path, "rb") as fh:
        for blk in iter(lambda: fh.read(1 << 24), b""):
            h.update(blk)
    return h.hexdigest()


def phase_stats(rows):
    out = {k: stats([r[k] for r in rows]) for k in PHASES}
    for k in ("n_keys", "n_vertices", "attempts", "peel_rounds"):
        out[k] = int(rows[-1][k])
    return out


def run_c2(a):
    import signature_kmers_amd as skm
    from signature_kmers_amd import synth
    p = synth.generate_arrays(1_000_000, 4000, per_file=4000)
    r, o, l, f, i, funcs = synth.build_inputs(p)
    b = skm.SignatureBuilder(len(funcs))
    b.add_batch(r, o, l, f, i)
    b.run()
    n = b.counters()["kept"]
    tmp = tempfile.mkdtemp(prefix="mph_db_bench_", dir=a.tmp)
    stems = {k: os.path.join(tmp, k) for k in ("host", "device_files")}
    phases = {"host": [], "device_files": [], "device": []}
    finish_s = []

    def open_host():
        t0 = time.perf_counter()
        kept = b.finish()
        finish_s.append(time.perf_counter() - t0)
        st = skm.mph_build_device(kept.keys, kept.data, stems["host"] + ".mph", stems["host"] + ".dat", seed=SEED,
                                  verify=False)
        del kept
        t0 = time.perf_counter()
        db = skm.CmphKmerDb(stems["host"])
        st["open_s"] = time.perf_counter() - t0
        return db, st

    def open_device_files():
        db = b.mph_db(seed=SEED, mph_path=stems["device_files"] + ".mph", dat_path=stems["device_files"] + ".dat")
        return db, db.stats

    def open_device():
        db = b.mph_db(seed=SEED)
        return db, db.stats

    paths = (("host", open_host), ("device_files", open_device_files), ("device", open_device))
    try:
        free0 = skm.device_mem_info(0)[0]
        times = {k: [] for k, _ in paths}
        for rep in range(a.repeats + 1):
            for name, fn in paths:
                t0 = time.perf_counter()
                db, st = fn()
                dt = time.perf_counter() - t0
                db.close()
                if rep:  # rep 0 is the warm-up of each path
                    times[name].append(dt)
                    phases[name].append(st)
        finish_timed = finish_s[1:]  # without the warm-up; the comparison below calls finish() once more
        files_equal = all(sha(stems["host"] + e) == sha(stems["device_files"] + e) for e in (".mph", ".dat"))
        # the three DBs over a sample of the kept set (members of one output slice) and strangers
        sample = b.finish_slice(8, 3).keys.copy()
        strangers = np.random.default_rng(5).integers(1, 2**63, size=1_000_000, dtype=np.uint64)
        dbs = {name: fn()[0] for name, fn in paths}
        free_open = skm.device_mem_info(0)[0]
        look = {k: (d.lookup_keys(sample), d.lookup_keys(strangers), d.lookup_fm(sample)) for k, d in dbs.items()}
        lookups_equal = all(np.array_equal(x, y) for k in look for x, y in zip(look["host"], look[k]))
        for d in dbs.values():
            d.close()
        # the on-device check at this size (the rank scan's tile offsets run over more than one chunk)
        t0 = time.perf_counter()
        vdb = b.mph_db(seed=SEED, verify=True)
        verify = {"seconds": time.perf_counter() - t0, "verified": int(vdb.stats["verified"]),
                  "verify_s": vdb.stats["verify_s"]}
        vdb.close()
        b.close()
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    plan = skm.mph_db_plan(n)
    section = {
        "workload": {"proteins": int(len(l)), "kept_kmers": int(n), "repeats": a.repeats, "seed": SEED},
        "open_db_s": {"finish_plus_mph_build_device_plus_CmphKmerDb": stats(times["host"]),
                      "mph_db_with_files": stats(times["device_files"]), "mph_db": stats(times["device"])},
        "host_path_parts_s": {"finish": stats(finish_timed), "open": stats([s["open_s"] for s in phases["host"]])},
        "phases_s": {k: phase_stats(v) for k, v in phases.items()},
        "files_equal": files_equal,
        "lookups_equal": lookups_equal,
        "sample_keys": int(len(sample)),
        "verify_run": verify,
        "plan": {"r": plan[0], "vertices": plan[1], "db_bytes": plan[2], "peak_bytes": plan[3]},
        "free_bytes_before": int(free0), "free_bytes_with_three_dbs_open": int(free_open),
        "observed_bytes_per_open_db": (int(free0) - int(free_open)) / 3.0,
    }
    write_section(a.out, "c2", section)
    if not (files_equal and lookups_equal and verify["verified"] == 1):
        sys.exit("the paths disagree")


def run_c3(a):
    import bench
    import signature_kmers_amd as skm
    from signature_kmers_amd import synth
    cores = bench.host_cores()
    workers = min(16, cores["usable"])
    files = (a.seqs + bench.PER_FILE - 1) // bench.PER_FILE
    t0 = time.time()
    c3 = bench.gen(synth, a.seqs, 4000, 0, files, workers)
    funcs = synth.functions(4000)
    sec = {"workload": {"proteins": c3.n_seqs, "windows": c3.n_windows, "generate_s": time.time() - t0}}
    skm.warm_device(0)
    b = skm.SignatureBuilder(len(funcs))
    c3.add_to(b)
    b.prepare()
    t0 = time.perf_counter()
    b.run()
    sec["build_run_s"] = time.perf_counter() - t0
    ctr = b.counters()
    sec["kept_kmers"], sec["passes"] = ctr["kept"], ctr["passes"]
    plan = skm.mph_db_plan(ctr["kept"])
    sec["plan"] = {"r": plan[0], "vertices": plan[1], "db_bytes": plan[2], "peak_bytes": plan[3]}
    sec["free_bytes_before"], sec["device_total_bytes"] = skm.device_mem_info(0)
    write_section(a.out, "c3", sec)
    t0 = time.perf_counter()
    try:
        db = b.mph_db(seed=SEED, release_work=True, verify=True)
    except skm.SkmError as e:
        sec["mph_db_error"] = str(e)
        sec["free_bytes_after_failure"] = skm.device_mem_info(0)[0]
        sec["status"] = "mph_db failed at this size"
        write_section(a.out, "c3", sec)
        return
    sec["mph_db_s"] = time.perf_counter() - t0
    sec["free_bytes_after"] = skm.device_mem_info(0)[0]
    sec["phases_s"] = {k: db.stats[k] for k in PHASES}
    sec["stats"] = {k: int(db.stats[k]) for k in ("n_keys", "n_vertices", "attempts", "peel_rounds", "verified")}
    sec["hash_size"] = db.hash_size()
    db.close()
    sec["free_bytes_after_close"] = skm.device_mem_info(0)[0]
    sec["observed_db_bytes"] = sec["free_bytes_after_close"] - sec["free_bytes_after"]
    sec["status"] = "measured"
    b.close()
    write_section(a.out, "c3", sec)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--c2", action="store_true")
    ap.add_argument("--c3", action="store_true")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--seqs", type=int, default=50_000_000, help="--c3: proteins of the proteome")
    ap.add_argument("--tmp", default=None, help="--c2: directory for the .mph / .dat files of the timed paths")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mph_db_ab.json"))
    a = ap.parse_args()
    if a.c2 == a.c3:
        sys.exit("one of --c2 / --c3")
    (run_c2 if a.c2 else run_c3)(a)


if __name__ == "__main__":
    main()
