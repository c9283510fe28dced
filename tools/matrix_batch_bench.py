"""A/B of the batched matrix distance against the per-problem loop it replaces.

Workload: a small signature DB (3000 training sequences, 30 families, as the matrix tests build
it) and 2000 problems of 50 synthetic query sequences each, cut from the family-sorted queries (a
problem is one family's members, like a per-family FASTA file of a family build).
  (a) batch: MatrixDistanceBatch(...).compute() over all problems      -- one device pass
  (b) loop:  MatrixDistance(...).compute() per problem                  -- the path that existed
Both are timed end to end from the packed host arrays to the host pair arrays (handle creation,
upload, device pipeline, download, close), after one untimed warm-up each; the median of the
repeats is reported, and the results of (a) and (b) are checked to be equal.

usage: python tools/matrix_batch_bench.py [--problems 2000] [--size 50] [--repeats 5] [--loop-repeats 3]
                                          [--out profiles/matrix_batch_ab.json]
"""
import argparse
import glob
import hashlib
import json
import os
import statistics
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def src_sha16() -> str:
    """Hash of libskm's device sources (as bench.py stamps its profiles)."""
    h = hashlib.sha256()
    d = os.path.join(ROOT, "signature_kmers_amd", "csrc")
    for f in sorted(glob.glob(os.path.join(d, "*.hip")) + glob.glob(os.path.join(d, "*.h"))):
        h.update(os.path.basename(f).encode())
        h.update(open(f, "rb").read())
    return h.hexdigest()[:16]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--problems", type=int, default=2000)
    ap.add_argument("--size", type=int, default=50)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--loop-repeats", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "matrix_batch_ab.json"))
    a = ap.parse_args()

    import oracle_ref
    import signature_kmers_amd as skm
    from signature_kmers_amd import synth

    fam, seed = 30, 41
    p = synth.generate_arrays(3000, fam, per_file=500, seed=seed)
    r, o, l, f, i, funcs = synth.build_inputs(p)
    ref = oracle_ref.build(r, o, l, f, i, len(funcs))
    n = a.problems * a.size
    per = 500
    nf = (n + per - 1) // per
    q = synth.generate_arrays((20 + nf) * per, fam, per_file=per, first_file=20, n_files=nf, seed=seed, extras=True)
    order = np.argsort(q.labels[:n], kind="stable")
    seq_off, seq_len = q.seq_off[order], q.seq_len[order]
    prob_seq = np.arange(a.problems + 1, dtype=np.uint64) * a.size

    with tempfile.TemporaryDirectory() as d:
        base = os.path.join(d, "kmer_data")
        skm.mph_build(ref["keys"], ref["data"], base + ".mph", base + ".dat", seed=7)
        db = skm.CmphKmerDb(base)

        state = {}

        def run_batch():
            mb = skm.MatrixDistanceBatch(db, funcs, q.residues, seq_off, seq_len, prob_seq)
            out = mb.compute()
            if not state:  # once: the stage timings and counters, and a second run on the resident queries
                t0 = time.perf_counter()
                mb.run()
                state["rerun_s"] = time.perf_counter() - t0
                state["timings"], state["counters"] = mb.timings(), mb.counters()
            mb.close()
            return out

        def run_loop():
            out = []
            for k in range(a.problems):
                s = slice(k * a.size, (k + 1) * a.size)
                md = skm.MatrixDistance(db, funcs, q.residues, seq_off[s], seq_len[s])
                out.append(md.compute())
                md.close()
            return out

        def timed(fn, reps):
            res = fn()  # warm-up: code objects, allocator, clocks
            ts = []
            for _ in range(reps):
                t0 = time.perf_counter()
                fn()
                ts.append(time.perf_counter() - t0)
            return res, ts

        got_b, tb = timed(run_batch, a.repeats)  # its warm-up run also takes the stage timings
        got_l, tl = timed(run_loop, a.loop_repeats)
        db.close()

    equal = len(got_b) == len(got_l) and all(np.array_equal(x, y) for x, y in zip(got_b, got_l))
    mb_s, ml_s = statistics.median(tb), statistics.median(tl)
    res = {
        "workload": {"problems": a.problems, "size": a.size, "queries": n, "db_training_seqs": 3000, "families": fam},
        "batch_s": {"median": mb_s, "all": tb},
        "loop_s": {"median": ml_s, "all": tl},
        "loop_over_batch": ml_s / mb_s,
        "batch_device_rerun_s": state["rerun_s"],
        "batch_stage_ms": state["timings"],
        "batch_counters": state["counters"],
        "results_equal": bool(equal),
        "src_sha16": src_sha16(),
    }
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")
    print(json.dumps(res))
    if not equal:
        sys.exit("batch and loop results differ")


if __name__ == "__main__":
    main()
