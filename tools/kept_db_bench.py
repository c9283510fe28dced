"""Measurements of the exact kept-k-mer DB built on the device from a finished build
(skm_build_kept_db) against the host path it stands beside (skm_build_finish + skm_db_open_kept).

  --c2   1 M proteins (the inputs of tests/test_gpu_scale.py's c2), one process, the paths
         alternating after a warm-up of each, --repeats timed repeats:
         (a) seconds from a finished run to an open DB: finish() + KeptKmerDb(...) vs kept_db()
         (b) recall device time over the 1 M proteins (skm_query_last_timings) on the host path's
             power-of-two table and on the range-reduced table at load 0.5 and 0.6 (--loads)
         and the calls of the three DBs compared byte for byte.
  --c3   50 M proteins on one GPU (bench.py's generator and options for the headline):
         kept_db(release_work=True), table_info, the free device memory before and after, the
         seconds to build the table, a recall over the 50 M proteins (seconds, k-mers/s), and the
         calls of every 250th protein (200,000) against oracle_ref.annotate_exact_par over a
         finish_slice-assembled kept set restricted to the k-mers of those proteins' windows (the
         whole kept set is 52 GB on the host; a k-mer outside the sample's windows is never looked
         up, so the restriction changes no call).

Each mode writes its own section of --out (default profiles/kept_db_ab.json, kept if the other
section is already there), stamped with bench.src_sha16().

usage: python tools/kept_db_bench.py --c2 [--repeats 5] [--loads 50,60] [--section NAME] | --c3 [--seqs 50000000] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def stats(xs):
    xs = [float(x) for x in xs]
    return {"mean": statistics.fmean(xs), "stdev": statistics.stdev(xs) if len(xs) > 1 else 0.0, "min": min(xs),
            "max": max(xs), "all": xs}


def write_section(path, name, section):
    import bench
    res = {}
    if os.path.exists(path):
        with open(path) as fh:
            res = json.load(fh)
    section["src_sha16"] = bench.src_sha16()
    res[name] = section
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")
    print(json.dumps({name: section}), flush=True)


def same_calls(a, b):
    return bool(np.array_equal(a[0], b[0]) and np.array_equal(a[1].view(np.uint8), b[1].view(np.uint8)))


def run_c2(a):
    import signature_kmers_amd as skm
    from signature_kmers_amd import synth
    p = synth.generate_arrays(1_000_000, 4000, per_file=4000)
    r, o, l, f, i, funcs = synth.build_inputs(p)
    hypo = funcs.index("hypothetical protein")
    b = skm.SignatureBuilder(len(funcs))
    b.add_batch(r, o, l, f, i)
    b.run()
    n = b.counters()["kept"]

    def open_host():
        kept = b.finish()
        return skm.KeptKmerDb(kept.keys, kept.data)

    def open_device(pct=0):
        return b.kept_db(load_pct=pct)

    # (a) finished run -> open DB, alternating
    t_host, t_dev = [], []
    for rep in range(a.repeats + 1):
        for fn, ts in ((open_host, t_host), (open_device, t_dev)):
            t0 = time.perf_counter()
            db = fn()
            dt = time.perf_counter() - t0
            db.close()
            if rep:  # rep 0 is the warm-up of each path
                ts.append(dt)
    # (b) recall device time on the three tables, alternating
    dbs = {"host_pow2": open_host()}
    for pct in a.loads:
        dbs[f"device_load{pct}"] = open_device(pct)
    info = {k: list(d.table_info()) for k, d in dbs.items()}
    qbs = {k: skm.QueryBatch(d, r, o, l) for k, d in dbs.items()}
    look = {k: [] for k in dbs}
    total = {k: [] for k in dbs}
    for rep in range(a.repeats + 1):
        for k, qb in qbs.items():
            qb.run(hypo_index=hypo)
            if rep:
                t = qb.timings()
                look[k].append(t["lookup"])
                total[k].append(t["total"])
    calls = {k: qb.calls() for k, qb in qbs.items()}
    equal = all(same_calls(calls["host_pow2"], calls[k]) for k in calls)
    windows = int(np.maximum(l.astype(np.int64) - 7, 0).sum())
    for qb in qbs.values():
        qb.close()
    for d in dbs.values():
        d.close()
    b.close()
    write_section(a.out, a.section or "c2", {
        "workload": {"proteins": int(len(l)), "kept_kmers": int(n), "query_windows": windows, "repeats": a.repeats},
        "open_db_s": {"finish_plus_KeptKmerDb": stats(t_host), "kept_db": stats(t_dev)},
        "table_info": info,
        "recall_lookup_ms": {k: stats(v) for k, v in look.items()},
        "recall_total_ms": {k: stats(v) for k, v in total.items()},
        "calls": int(len(calls["host_pow2"][1])),
        "calls_equal": equal,
    })
    if not equal:
        sys.exit("calls differ between the DBs")


def run_c3(a):
    import bench
    import oracle_ref
    import signature_kmers_amd as skm
    from signature_kmers_amd import synth
    stride, slice_bits = 250, 6
    cores = bench.host_cores()
    workers = min(16, cores["usable"])
    files = (a.seqs + bench.PER_FILE - 1) // bench.PER_FILE
    t0 = time.time()
    c3 = bench.gen(synth, a.seqs, 4000, 0, files, workers)
    funcs = synth.functions(4000)
    hypo = funcs.index("hypothetical protein")
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
    sec["plan_slots_bytes"] = list(skm.kept_db_plan(ctr["kept"], load_pct=a.load_pct))
    sec["free_bytes_before"], sec["device_total_bytes"] = skm.device_mem_info(0)
    write_section(a.out, "c3", sec)
    t0 = time.perf_counter()
    try:
        db = b.kept_db(load_pct=a.load_pct, release_work=True)
    except skm.SkmError as e:
        sec["kept_db_error"] = str(e)
        sec["free_bytes_after_failure"] = skm.device_mem_info(0)[0]
        sec["status"] = "the table did not fit: the C3 recall is still open"
        write_section(a.out, "c3", sec)
        return
    sec["kept_db_s"] = time.perf_counter() - t0
    sec["free_bytes_after"] = skm.device_mem_info(0)[0]
    sec["table_info"] = list(db.table_info())
    write_section(a.out, "c3", sec)

    # recall over every protein, in batches of whole files; the calls of every stride-th protein kept
    per_batch = 500  # files: 2 M proteins
    wall = dev_lookup = dev_total = 0.0
    n_calls = first = 0
    samp_seqs, samp_off, samp_calls = [], [0], []
    for p0 in range(0, len(c3.parts), per_batch):
        r, o, l, _, _ = bench.Shard(c3.parts[p0:p0 + per_batch]).packed()
        t0 = time.perf_counter()
        qb = skm.QueryBatch(db, r, o, l)
        qb.run(hypo_index=hypo)
        off, calls = qb.calls()
        wall += time.perf_counter() - t0
        t = qb.timings()
        dev_lookup += t["lookup"]
        dev_total += t["total"]
        qb.close()
        n_calls += len(calls)
        for s in range((-first) % stride, len(l), stride):
            samp_seqs.append(r[int(o[s]):int(o[s]) + int(l[s])].tobytes())
            samp_calls.append(calls[int(off[s]):int(off[s + 1])])
            samp_off.append(samp_off[-1] + len(samp_calls[-1]))
        first += len(l)
    sec["recall"] = {"wall_s": wall, "device_lookup_s": dev_lookup / 1e3, "device_total_s": dev_total / 1e3,
                     "kmers_per_s_wall": c3.n_windows / wall, "kmers_per_s_device": c3.n_windows / (dev_total / 1e3),
                     "calls": n_calls}
    write_section(a.out, "c3", sec)
    db.close()

    # parity of the sample against the oracle over the kept k-mers of its windows
    t0 = time.time()
    lens = np.array([len(s) for s in samp_seqs], np.uint32)
    offs = np.zeros(len(lens), np.uint64)
    offs[1:] = np.cumsum(lens[:-1], dtype=np.uint64)
    res = np.frombuffer(b"".join(samp_seqs), np.uint8)
    w = np.unique(np.ascontiguousarray(np.lib.stride_tricks.sliding_window_view(res, 8)).view(np.uint64).ravel())
    ws = (oracle_ref.slice_hash(w) >> np.uint64(64 - slice_bits)).astype(np.int64)
    order = np.argsort(ws, kind="stable")
    w, ws = w[order], ws[order]
    bounds = np.searchsorted(ws, np.arange((1 << slice_bits) + 1))
    keys, data = [], []
    for s in range(1 << slice_bits):
        sl = b.finish_slice(slice_bits, s)
        q = w[bounds[s]:bounds[s + 1]]
        pos = np.minimum(np.searchsorted(sl.keys, q), max(len(sl.keys) - 1, 0))
        hit = (sl.keys[pos] == q) if len(sl.keys) else np.zeros(len(q), bool)
        keys.append(sl.keys[pos[hit]].copy())
        data.append(sl.data[pos[hit]].copy())
        del sl
    b.close()
    keys, data = np.concatenate(keys), np.concatenate(data)
    order = np.argsort(keys)
    keys, data = keys[order], data[order]
    ooff, ocalls = oracle_ref.annotate_exact_par(keys, data, res, offs, lens, cores["usable"], hypo_index=hypo)
    got = (np.array(samp_off, np.uint64), np.concatenate(samp_calls) if samp_calls else ocalls[:0])
    sec["sample_parity"] = {"proteins": int(len(lens)), "stride": stride, "calls": int(len(got[1])),
                            "reference": "oracle_ref.annotate_exact_par over a finish_slice-assembled kept set "
                                         "(64 slices) restricted to the k-mers of the sample's windows",
                            "kept_kmers_in_sample_windows": int(len(keys)), "equal": same_calls(got, (ooff, ocalls)),
                            "seconds": time.time() - t0}
    sec["status"] = "measured"
    write_section(a.out, "c3", sec)
    if not sec["sample_parity"]["equal"]:
        sys.exit("the sample's calls differ from the oracle's")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--c2", action="store_true")
    ap.add_argument("--c3", action="store_true")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--loads", type=lambda v: [int(x) for x in v.split(",")], default=[50, 60],
                    help="--c2: load_pct of the range-reduced tables of the recall comparison")
    ap.add_argument("--section", default=None, help="name of the section written (default: c2 / c3)")
    ap.add_argument("--seqs", type=int, default=50_000_000, help="--c3: proteins of the proteome")
    ap.add_argument("--load-pct", type=int, default=0, help="--c3: the table's load (0 = the library's default)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "kept_db_ab.json"))
    a = ap.parse_args()
    if a.c2 == a.c3:
        sys.exit("one of --c2 / --c3")
    (run_c2 if a.c2 else run_c3)(a)


if __name__ == "__main__":
    main()
