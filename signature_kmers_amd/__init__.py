"""signature_kmers_amd -- MI355X-native signature-k-mer engine (host mirror over libskm's C-ABI).

The reference (olsonanl/signature_kmers) exposes its hot path as C++ templates:
``SignatureBuilder<8>`` (signature_build.h:55-147), the KmerDb concept ``CmphKmerDb``
(cmph_kmer.h:28-164) and ``FunctionCaller<KmerDb>`` (call_functions.h:60-136).  This module
mirrors those classes in Python on top of ``libskm.so`` (include/skm.h).  Every compute call goes
to the HIP library; there is no CPU fallback -- a missing library raises immediately.
"""
from __future__ import annotations

import ctypes as C
import os
from dataclasses import dataclass

import numpy as np

__all__ = [
    "SkmError", "lib", "K", "UNDEFINED_FUNCTION", "STORED_DTYPE", "CALL_DTYPE",
    "SignatureBuilder", "KeptKmers", "CmphKmerDb", "FunctionCaller", "mph_build",
    "kmer_to_str", "str_to_kmer", "keys_from_strings", "device_count", "MatrixDistance", "SeqIdMap",
    "matrix_tile_rows", "KeptKmerDb", "DeviceKeptKmerDb", "kept_db_plan", "kept_slot",
]

K = 8
UNDEFINED_FUNCTION = 0xFFFF
_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("SKM_LIB_PATH") or os.path.join(_HERE, "libskm.so")  # override: A/B builds

STORED_DTYPE = np.dtype([("avg_from_end", "<u2"), ("function_index", "<u2"), ("mean", "<u2"),
                         ("median", "<u2"), ("var", "<u2")])  # StoredKmerData, kmer_data.h:114-128
CALL_DTYPE = np.dtype([("start", "<u4"), ("end", "<u4"), ("count", "<i4"), ("function_index", "<u2"),
                       ("pad", "<u2"), ("protein_length_median", "<u4"),
                       ("protein_length_med_avg_dev", "<f4")])  # KmerCall, call_functions.h:23-48
# skm_best_call: find_best_call's result for one sequence; flags & BEST_PAIR: "name(fi_a) ?? name(fi_b)"
BEST_DTYPE = np.dtype([("fi", "<u2"), ("fi_a", "<u2"), ("fi_b", "<u2"), ("flags", "<u2"), ("score", "<f4"),
                       ("offset", "<f4")])
BEST_PAIR = 1
BEST_MAX_PARTS = 8
BEST_MAX_CALLS = 64


class SkmError(RuntimeError):
    pass


class _BuildOpts(C.Structure):
    _fields_ = [("k", C.c_int32), ("max_seqs_per_file", C.c_uint32), ("n_functions", C.c_uint32),
                ("canonical_order", C.c_int32), ("rank", C.c_int32), ("world_size", C.c_int32)]


_A2A_T = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.c_void_p,
                     C.POINTER(C.c_uint64), C.POINTER(C.c_uint64))
_RED_T = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_uint64, C.c_int)
_AGV_T = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_uint64))


class _Transport(C.Structure):
    _fields_ = [("ctx", C.c_void_p), ("alltoallv", _A2A_T), ("allreduce", _RED_T), ("allgatherv", _AGV_T)]


class _Kept(C.Structure):
    _fields_ = [("keys", C.POINTER(C.c_uint64)), ("data", C.c_void_p), ("n", C.c_uint64),
                ("distinct_functions", C.POINTER(C.c_uint32)), ("seqs_with_func", C.POINTER(C.c_uint32)),
                ("n_functions", C.c_uint32), ("n_seqs_with_signature", C.c_uint64),
                ("distinct_signatures", C.c_uint64), ("n_windows", C.c_uint64), ("n_records", C.c_uint64)]


class _AnnotOpts(C.Structure):
    _fields_ = [("min_hits", C.c_int32), ("max_gap", C.c_int32), ("ignore_hypo", C.c_int32),
                ("hypo_index", C.c_int32), ("mean_mode", C.c_int32), ("mad_mode", C.c_int32)]


class _Calls(C.Structure):
    _fields_ = [("call_off", C.POINTER(C.c_uint64)), ("calls", C.c_void_p), ("n_seqs", C.c_uint64),
                ("n_calls", C.c_uint64), ("n_windows", C.c_uint64)]


class _BestCalls(C.Structure):
    _fields_ = [("best", C.c_void_p), ("n_seqs", C.c_uint64), ("n_calls", C.c_uint64), ("n_windows", C.c_uint64),
                ("n_deferred", C.c_uint64), ("kernel_ms", C.c_float)]


class _FastaTable(C.Structure):
    _fields_ = [("n_files", C.c_uint64), ("n_recs", C.c_uint64), ("n_residues", C.c_uint64), ("n_windows", C.c_uint64),
                ("file_rec", C.POINTER(C.c_uint64)), ("seq_len", C.POINTER(C.c_uint32)),
                ("hdr_pos", C.POINTER(C.c_uint64)), ("residues", C.POINTER(C.c_uint8)), ("parse_ms", C.c_float)]


class _MatrixOpts(C.Structure):
    _fields_ = [("hypo_index", C.c_int32), ("row_begin", C.c_uint32), ("row_end", C.c_uint32), ("pad", C.c_uint32),
                ("max_tile_bytes", C.c_uint64)]


class _MatrixBatchOpts(C.Structure):
    _fields_ = [("hypo_index", C.c_int32), ("small_cols", C.c_uint32)]


class _KeptDbOpts(C.Structure):
    _fields_ = [("load_pct", C.c_uint32), ("release_work", C.c_int32), ("slots", C.c_uint64)]


class _MphDbOpts(C.Structure):
    _fields_ = [("seed", C.c_uint32), ("release_work", C.c_int32), ("verify", C.c_int32), ("pad", C.c_int32),
                ("mph_path", C.c_char_p), ("dat_path", C.c_char_p)]


class _FinalKmersStats(C.Structure):
    _fields_ = [("n_kmers", C.c_uint64), ("bytes", C.c_uint64), ("chunks", C.c_uint64), ("pieces", C.c_uint64),
                ("total_s", C.c_double), ("wait_s", C.c_double), ("write_s", C.c_double),
                ("select_ms", C.c_float), ("sort_ms", C.c_float), ("gather_ms", C.c_float), ("format_ms", C.c_float),
                ("d2h_ms", C.c_float), ("wide_index", C.c_uint32)]


class _RecallOpts(C.Structure):
    _fields_ = [("batch_residues", C.c_uint64), ("first_seq", C.c_uint64), ("n_seqs", C.c_uint64)]


class _RecallStats(C.Structure):
    _fields_ = [("n_seqs", C.c_uint64), ("n_windows", C.c_uint64), ("n_calls", C.c_uint64), ("n_deferred", C.c_uint64),
                ("n_batches", C.c_uint64), ("resident_bytes", C.c_uint64), ("view_ms", C.c_float),
                ("lookup_ms", C.c_float), ("calls_ms", C.c_float), ("best_ms", C.c_float), ("wall_s", C.c_double)]


class _Pairs(C.Structure):
    _fields_ = [("pairs", C.POINTER(C.c_uint32)), ("n", C.c_uint64), ("n_hits", C.c_uint64)]


_P = C.c_void_p
_SIGS = {
    "skm_last_error": (C.c_char_p, []),
    "skm_version": (C.c_char_p, []),
    "skm_device_count": (C.c_int, [C.POINTER(C.c_int)]),
    "skm_device_mem_info": (C.c_int, [C.c_int, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
    "skm_build_create": (C.c_int, [C.POINTER(_P), C.POINTER(C.c_int), C.c_int, C.POINTER(_BuildOpts)]),
    "skm_build_add_batch": (C.c_int, [_P, _P, _P, _P, _P, _P, C.c_size_t]),
    "skm_build_add_fasta": (C.c_int, [_P, _P, _P, C.c_size_t, _P, _P, C.c_uint64, C.POINTER(_FastaTable)]),
    "skm_build_debug_input": (C.c_int, [_P, _P, C.c_uint64, _P, C.c_uint64, C.POINTER(C.c_uint64),
                                        C.POINTER(C.c_uint64)]),
    "skm_build_prepare": (C.c_int, [_P]),
    "skm_build_run": (C.c_int, [_P]),
    "skm_build_last_timings": (C.c_int, [_P, C.POINTER(C.c_float), C.c_int]),
    "skm_build_set_kernel_timing": (C.c_int, [_P, C.c_int, C.c_char_p]),
    "skm_build_kernel_timings": (C.c_int, [_P, C.c_char_p, C.c_size_t, C.POINTER(C.c_float), C.POINTER(C.c_uint64),
                                           C.c_int]),
    "skm_build_finish": (C.c_int, [_P, C.POINTER(_Kept)]),
    "skm_build_finish_slice": (C.c_int, [_P, C.c_int, C.c_uint32, C.POINTER(_Kept)]),
    "skm_build_signature_flags": (C.c_int, [_P, _P, C.c_uint64]),
    "skm_build_set_option": (C.c_int, [_P, C.c_char_p, C.c_int64]),
    "skm_build_set_transport": (C.c_int, [_P, C.POINTER(_Transport)]),
    "skm_debug_exchange_plan": (C.c_int, [C.POINTER(_Transport), C.c_int, C.c_int, C.c_uint32, _P, _P, _P, _P]),
    "skm_debug_transport_check": (C.c_int, [C.POINTER(_Transport), C.c_int, C.c_int]),
    "skm_build_counters": (C.c_int, [_P, C.POINTER(C.c_uint64), C.c_int]),
    "skm_build_reserve": (C.c_int, [_P, C.c_uint64, C.c_uint64]),
    "skm_build_debug_jobs": (C.c_int, [_P, C.POINTER(C.c_uint32), C.c_int]),
    "skm_build_debug_overflow": (C.c_int, [_P, C.POINTER(C.c_uint32), C.c_int]),
    "skm_build_debug_front": (C.c_int, [_P, C.POINTER(C.c_uint64), C.c_int]),
    "skm_build_debug_stage_starts": (C.c_int, [_P, C.c_uint32, C.POINTER(C.c_uint64), C.c_int]),
    "skm_build_debug_pass_windows": (C.c_int, [_P, C.POINTER(C.c_uint64), C.c_int]),
    "skm_debug_chain_bench": (C.c_int, [C.c_uint32, C.c_uint32, C.c_int, C.POINTER(C.c_float)]),
    "skm_debug_chain_eval": (C.c_int, [_P, C.c_uint32, C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_double)]),
    "skm_build_debug_stamps": (C.c_int, [_P, C.c_int, C.POINTER(C.c_uint64), C.c_int]),
    "skm_kept_free": (None, [C.POINTER(_Kept)]),
    "skm_build_destroy": (None, [_P]),
    "skm_comm_unique_id": (C.c_int, [_P]),
    "skm_build_set_comm": (C.c_int, [_P, _P]),
    "skm_build_group_run": (C.c_int, [C.POINTER(_P), C.c_int]),
    "skm_debug_div_check": (C.c_int, [C.c_uint64, C.c_uint32, C.POINTER(C.c_uint64)]),
    "skm_db_open": (C.c_int, [C.POINTER(_P), C.c_char_p, C.c_char_p, C.c_int]),
    "skm_db_open_mem": (C.c_int, [C.POINTER(_P), _P, C.c_size_t, _P, C.c_size_t, C.c_int]),
    "skm_db_open_kept": (C.c_int, [C.POINTER(_P), _P, _P, C.c_size_t, C.c_int]),
    "skm_build_kept_db": (C.c_int, [_P, C.POINTER(_KeptDbOpts), C.POINTER(_P)]),
    "skm_kept_db_plan": (C.c_int, [C.c_uint64, C.POINTER(_KeptDbOpts), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
    "skm_debug_kept_slot": (C.c_int, [C.c_uint64, C.c_uint64, C.POINTER(C.c_uint64)]),
    "skm_build_mph_db": (C.c_int, [_P, C.POINTER(_MphDbOpts), C.POINTER(_P), C.c_void_p]),
    "skm_mph_db_plan": (C.c_int, [C.c_uint64, C.POINTER(C.c_uint64)]),
    "skm_build_write_final_kmers": (C.c_int, [_P, C.c_char_p, C.POINTER(_FinalKmersStats)]),
    "skm_build_stats": (C.c_int, [_P, C.POINTER(_Kept)]),
    "skm_final_kmers_info": (C.c_int, [C.POINTER(C.c_uint32)]),
    "skm_debug_final_kmers_host": (C.c_int, [_P, _P, C.c_size_t, _P, C.c_size_t, C.POINTER(C.c_uint64)]),
    "skm_db_lookup_fm": (C.c_int, [_P, _P, C.c_size_t, _P]),
    "skm_db_table_info": (C.c_int, [_P, C.POINTER(C.c_uint64), C.c_int]),
    "skm_db_size": (C.c_int, [_P, C.POINTER(C.c_uint32)]),
    "skm_db_lookup": (C.c_int, [_P, _P, C.c_size_t, _P]),
    "skm_debug_db_lookup_generic": (C.c_int, [_P, _P, C.c_size_t, _P]),
    "skm_db_close": (None, [_P]),
    "skm_mph_build": (C.c_int, [_P, _P, C.c_size_t, C.c_uint32, C.c_char_p, C.c_char_p]),
    "skm_mph_build_device": (C.c_int, [_P, _P, C.c_size_t, C.c_uint32, C.c_char_p, C.c_char_p, C.c_int]),
    "skm_mph_build_device_ex": (C.c_int, [_P, _P, C.c_size_t, C.c_uint32, C.c_char_p, C.c_char_p, C.c_int, C.c_int,
                                          C.c_void_p]),
    "skm_query_create": (C.c_int, [C.POINTER(_P), _P, _P, _P, _P, C.c_size_t]),
    "skm_query_run": (C.c_int, [_P, C.POINTER(_AnnotOpts)]),
    "skm_query_last_timings": (C.c_int, [_P, C.POINTER(C.c_float), C.c_int]),
    "skm_query_calls": (C.c_int, [_P, C.POINTER(_Calls)]),
    "skm_query_window_hits": (C.c_int, [_P, _P, _P, _P, C.c_uint64, C.POINTER(C.c_uint64)]),
    "skm_query_destroy": (None, [_P]),
    "skm_annotate": (C.c_int, [_P, _P, _P, _P, C.c_size_t, C.POINTER(_AnnotOpts), C.POINTER(_Calls)]),
    "skm_calls_free": (None, [C.POINTER(_Calls)]),
    "skm_fasta_parse_info": (C.c_int, [C.POINTER(C.c_uint32)]),
    "skm_fasta_parse_device": (C.c_int, [_P, _P, C.c_size_t, C.c_int, C.c_int, C.POINTER(_FastaTable)]),
    "skm_query_create_fasta": (C.c_int, [C.POINTER(_P), _P, _P, _P, C.c_size_t, C.POINTER(_FastaTable)]),
    "skm_annotate_fasta": (C.c_int, [_P, _P, _P, C.c_size_t, C.POINTER(_AnnotOpts), C.POINTER(_Calls),
                                     C.POINTER(_FastaTable)]),
    "skm_fasta_table_free": (None, [C.POINTER(_FastaTable)]),
    "skm_matrix_create": (C.c_int, [C.POINTER(_P), _P, _P, _P, _P, _P, C.c_size_t, C.c_uint32]),
    "skm_matrix_run": (C.c_int, [_P, C.POINTER(_MatrixOpts)]),
    "skm_matrix_set_transport": (C.c_int, [_P, C.c_int, C.c_int, C.POINTER(_Transport)]),
    "skm_matrix_set_comm": (C.c_int, [_P, C.c_int, C.c_int, _P]),
    "skm_matrix_last_timings": (C.c_int, [_P, C.POINTER(C.c_float), C.c_int]),
    "skm_matrix_counters": (C.c_int, [_P, C.POINTER(C.c_uint64), C.c_int]),
    "skm_matrix_pairs": (C.c_int, [_P, C.POINTER(_Pairs)]),
    "skm_pairs_free": (None, [C.POINTER(_Pairs)]),
    "skm_matrix_destroy": (None, [_P]),
    "skm_matrix_batch_create": (C.c_int, [C.POINTER(_P), _P, _P, _P, _P, _P, _P, _P, C.c_size_t]),
    "skm_matrix_batch_run": (C.c_int, [_P, C.POINTER(_MatrixBatchOpts)]),
    "skm_matrix_batch_pairs": (C.c_int, [_P, C.POINTER(_Pairs), C.POINTER(C.c_uint64)]),
    "skm_matrix_batch_counters": (C.c_int, [_P, C.POINTER(C.c_uint64), C.c_int]),
    "skm_matrix_batch_group_counts": (C.c_int, [_P, C.POINTER(C.c_uint64)]),
    "skm_matrix_batch_last_timings": (C.c_int, [_P, C.POINTER(C.c_float), C.c_int]),
    "skm_matrix_batch_destroy": (None, [_P]),
    "skm_matrix_tile_rows": (C.c_int, [C.c_uint32, C.c_int, C.c_int, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]),
    "skm_find_best_call": (C.c_int, [_P, C.c_size_t, C.POINTER(C.c_char_p), C.c_size_t, C.POINTER(C.c_uint16),
                                     C.POINTER(C.c_float), C.POINTER(C.c_float), C.c_char_p, C.c_size_t]),
    "skm_fidx_create": (C.c_int, [C.POINTER(_P), C.POINTER(C.c_char_p), C.c_size_t, C.c_int]),
    "skm_fidx_destroy": (None, [_P]),
    "skm_best_call_name": (C.c_int, [_P, _P, C.c_char_p, C.c_size_t]),
    "skm_best_calls_host": (C.c_int, [C.POINTER(_Calls), _P, C.c_int, C.POINTER(_BestCalls)]),
    "skm_query_best_calls": (C.c_int, [_P, _P, C.POINTER(_BestCalls)]),
    "skm_annotate_best": (C.c_int, [_P, _P, _P, _P, C.c_size_t, C.POINTER(_AnnotOpts), _P, C.POINTER(_BestCalls)]),
    "skm_annotate_fasta_best": (C.c_int, [_P, _P, _P, C.c_size_t, C.POINTER(_AnnotOpts), _P, C.POINTER(_BestCalls),
                                          C.POINTER(_FastaTable)]),
    "skm_debug_best_calls": (C.c_int, [_P, _P, C.c_size_t, _P, C.c_int, _P, _P, C.POINTER(C.c_float)]),
    "skm_best_calls_free": (None, [C.POINTER(_BestCalls)]),
    "skm_build_resident_seqs": (C.c_int, [_P, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
    "skm_build_recall": (C.c_int, [_P, _P, C.POINTER(_AnnotOpts), C.POINTER(_RecallOpts), _P, C.POINTER(_BestCalls),
                                   C.POINTER(_Calls), C.POINTER(_RecallStats)]),
    "skm_recall_plan": (C.c_int, [_P, C.c_uint64, C.c_uint64, C.c_uint64, C.c_uint64, _P, C.c_uint64,
                                  C.POINTER(C.c_uint64)]),
}

_lib = None


def lib():
    """Load libskm.so (built in-tree by __graft_entry__.build / `make`).  Fails loudly."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise SkmError(f"{LIB_PATH} is missing: run `make` (or __graft_entry__.build()) first")
        h = C.CDLL(LIB_PATH)
        for name, (res, args) in _SIGS.items():
            fn = getattr(h, name)
            fn.restype = res
            fn.argtypes = args
        _lib = h
    return _lib


def _check(rc: int):
    if rc != 0:
        raise SkmError(f"libskm error {rc}: {lib().skm_last_error().decode(errors='replace')}")


def _ptr(a: np.ndarray):
    return a.ctypes.data_as(C.c_void_p)


def debug_chain_bench(n: int, njobs: int, mode: int = 0) -> float:
    ms = C.c_float()
    _check(lib().skm_debug_chain_bench(n, njobs, mode, C.byref(ms)))
    return ms.value


def debug_chain_eval(samples, mode: int):
    """(P^2 median, variance) as raw doubles for one chain (samples in visit order)."""
    x = np.ascontiguousarray(samples, dtype=np.uint32)
    med, var = C.c_double(), C.c_double()
    _check(lib().skm_debug_chain_eval(_ptr(x), len(x), mode, C.byref(med), C.byref(var)))
    return med.value, var.value


def debug_div_check(nm: int, per: int) -> int:
    """Mismatches of the device exact-division helpers against IEEE division."""
    v = C.c_uint64(0)
    _check(lib().skm_debug_div_check(nm, per, C.byref(v)))
    return v.value


def device_count() -> int:
    n = C.c_int(0)
    _check(lib().skm_device_count(C.byref(n)))
    return n.value


def device_mem_info(device: int = 0) -> tuple:
    """(free, total) bytes of a device's memory (hipMemGetInfo)."""
    fr, tot = C.c_uint64(), C.c_uint64()
    _check(lib().skm_device_mem_info(device, C.byref(fr), C.byref(tot)))
    return fr.value, tot.value


def warm_device(device: int = 0) -> None:
    """Bring up the process's HIP runtime and the device context (one throwaway build handle), so
    that a timed one-shot build does not include the runtime's start-up."""
    SignatureBuilder(1, device=device).close()


def kmer_to_str(key: int) -> str:
    return int(key).to_bytes(8, "little").decode("latin-1")


def str_to_kmer(s: str) -> int:
    b = s.encode("latin-1")
    assert len(b) == K
    return int.from_bytes(b, "little")


def keys_from_strings(strs) -> np.ndarray:
    return np.array([str_to_kmer(s) for s in strs], dtype=np.uint64)


@dataclass
class KeptKmers:
    """KeptKmers<8> + KmerStatistics (signature_build.h:34-53), keys sorted ascending."""
    keys: np.ndarray                 # u64 little-endian k-mers
    data: np.ndarray                 # STORED_DTYPE
    distinct_functions: np.ndarray   # u32[n_functions]
    seqs_with_func: np.ndarray       # u32[n_functions]
    n_seqs_with_signature: int
    distinct_signatures: int
    n_windows: int
    n: int = 0                       # kept k-mers (len(keys), except from SignatureBuilder.stats)
    n_records: int = 0               # valid windows (occurrences)

    def stats_lines(self) -> str:
        """stdout of process_kmers (signature_build.tcc:210-212)."""
        return (f"Kept {len(self.keys)} kmers\ndistinct_signatures={self.distinct_signatures}\n"
                f"num_seqs_with_a_signature={self.n_seqs_with_signature}\n")

    def final_kmers_lines(self):
        """final.kmers rows (kmers-build-signatures.cc:212-216): KMER \\t avg_from_end \\t fi \\t"""
        for k, d in zip(self.keys, self.data):
            yield f"{kmer_to_str(k)}\t{int(d['avg_from_end'])}\t{int(d['function_index'])}\t\n"


class _KeptOwner:
    """Owns one skm_kept's library arrays; frees them when the last numpy view is gone."""

    def __init__(self, k):
        self.k = k

    def __del__(self):
        try:
            lib().skm_kept_free(C.byref(self.k))
        except Exception:
            pass


SEQ_META_DTYPE = np.dtype([("pstart", np.uint64), ("len", np.uint32), ("func", np.uint16), ("pad", np.uint16)])


class SignatureBuilder:
    """Device signature build (SignatureBuilder<8>::extract_kmers + process_kmers).

    Sequences are added in reference emission order with their FunctionIndex (0xFFFF = no kept
    function) and seq_id (file_number * max_seqs_per_file + k)."""

    def __init__(self, n_functions: int, max_seqs_per_file: int = 100000, device: int = 0, rank: int = 0,
                 world_size: int = 1):
        self._h = C.c_void_p()
        opts = _BuildOpts(8, max_seqs_per_file, n_functions, 1, rank, world_size)
        self.rank, self.world_size = rank, world_size
        dev = (C.c_int * 1)(device)
        _check(lib().skm_build_create(C.byref(self._h), dev, 1, C.byref(opts)))
        self.n_functions = n_functions
        self.device = device

    def add_batch(self, residues, seq_off, seq_len, seq_func, seq_id=None):
        residues = np.ascontiguousarray(residues, dtype=np.uint8)
        seq_off = np.ascontiguousarray(seq_off, dtype=np.uint64)
        seq_len = np.ascontiguousarray(seq_len, dtype=np.uint32)
        seq_func = np.ascontiguousarray(seq_func, dtype=np.uint16)
        n = len(seq_len)
        assert len(seq_off) == n and len(seq_func) == n
        if n:
            end = seq_off.astype(np.int64) + seq_len.astype(np.int64)
            if end.max() > len(residues):
                raise SkmError("seq_off/seq_len exceed the residue buffer")
        sid = None if seq_id is None else np.ascontiguousarray(seq_id, dtype=np.uint32)
        _check(lib().skm_build_add_batch(self._h, _ptr(residues), _ptr(seq_off), _ptr(seq_len), _ptr(seq_func),
                                         _ptr(sid) if sid is not None else None, n))

    def add_fasta(self, blobs, rec_func, rec_id=None) -> "FastaTable":
        """skm_build_add_fasta: add_batch with FastaParser in front of it, on the device.  blobs are
        the files' raw bytes (as _fasta_input takes them); rec_func[r] / rec_id[r] describe parser
        record r (the records with a non-empty id, in file order), 0xFFFF = not selected.  The
        selected records' residues go straight into the build's resident buffer.  Returns the
        FastaTable over every parser record (without residues)."""
        data, off = _fasta_input(blobs)
        rec_func = np.ascontiguousarray(rec_func, dtype=np.uint16)
        sid = None if rec_id is None else np.ascontiguousarray(rec_id, dtype=np.uint32)
        if sid is not None and len(sid) != len(rec_func):
            raise SkmError("rec_id and rec_func differ in length")
        t = _FastaTable()
        _check(lib().skm_build_add_fasta(self._h, _ptr(data), _ptr(off), len(off) - 1, _ptr(rec_func),
                                         _ptr(sid) if sid is not None else None, len(rec_func), C.byref(t)))
        try:
            return FastaTable(t)
        finally:
            lib().skm_fasta_table_free(C.byref(t))

    def debug_input(self) -> tuple:
        """skm_build_debug_input (after prepare): (the packed residues d_res[0, rp) as u8, the
        sequence table as a structured array with pstart u64, len u32, func u16, pad u16)."""
        rp, nseq = C.c_uint64(0), C.c_uint64(0)
        _check(lib().skm_build_debug_input(self._h, None, 0, None, 0, C.byref(rp), C.byref(nseq)))
        res = np.zeros(max(int(rp.value), 1), np.uint8)
        meta = np.zeros(max(int(nseq.value), 1), SEQ_META_DTYPE)
        _check(lib().skm_build_debug_input(self._h, _ptr(res), len(res), _ptr(meta), len(meta), C.byref(rp),
                                           C.byref(nseq)))
        return res[:int(rp.value)], meta[:int(nseq.value)]

    def reserve(self, n_residues: int, n_seqs: int):
        """skm_build_reserve: capacity hint so the HBM residue buffer is allocated once (batches
        stream to HBM through two alternating pinned staging buffers as they are added)."""
        _check(lib().skm_build_reserve(self._h, int(n_residues), int(n_seqs)))

    def set_transport(self, transport: "GlooTransport"):
        """Join the ranks through a host transport (skm_build_set_transport) instead of RCCL."""
        self._transport = transport  # the callbacks must outlive the handle's runs
        _check(lib().skm_build_set_transport(self._h, transport.ptr))

    def set_comm(self, unique_id: bytes):
        """Join the RCCL communicator (collective over the world_size ranks)."""
        buf = (C.c_uint8 * 128).from_buffer_copy(bytes(unique_id))
        _check(lib().skm_build_set_comm(self._h, buf))

    def prepare(self):
        _check(lib().skm_build_prepare(self._h))

    def run(self):
        _check(lib().skm_build_run(self._h))

    def timings(self) -> dict:
        ms = (C.c_float * 17)()
        n = lib().skm_build_last_timings(self._h, ms, 17)
        names = ["extract_count", "scan", "extract_scatter", "bucket_process", "overflow", "chains", "stats", "total",
                 "exchange", "partition", "bucket_kernel", "big_groups", "chain_tail", "giant_start", "giant_end",
                 "tail_wait", "groupby_wait"]
        return {names[i]: float(ms[i]) for i in range(n)}

    def set_kernel_timing(self, enable: bool, only: str | None = None):
        """Event pairs around every kernel launch of the next runs (or only kernel `only`)."""
        _check(lib().skm_build_set_kernel_timing(self._h, 1 if enable else 0, only.encode() if only else None))

    def kernel_timings(self) -> dict:
        """{kernel name: (total device ms, launches)} of the last run (set_kernel_timing)."""
        n = lib().skm_build_kernel_timings(self._h, None, 0, None, None, 0)
        if n <= 0:
            return {}
        ms = (C.c_float * n)()
        cnt = (C.c_uint64 * n)()
        buf = C.create_string_buffer(64 * n + 64)
        lib().skm_build_kernel_timings(self._h, buf, len(buf), ms, cnt, n)
        names = buf.value.decode().split("\n")[:n]
        return {names[i]: (float(ms[i]), int(cnt[i])) for i in range(n)}

    def set_option(self, name: str, value: int):
        """skm_build_set_option: "key_range_passes" (0 = automatic), "device_memory_budget_mb",
        and the diagnostic tunables named in include/skm.h."""
        _check(lib().skm_build_set_option(self._h, name.encode(), int(value)))

    def passes(self) -> int:
        """Key-range passes of the last run (1 when the shard fits the work buffers)."""
        return self.counters()["passes"]

    def counters(self) -> dict:
        v = (C.c_uint64 * 51)()
        n = lib().skm_build_counters(self._h, v, 51)
        names = ["windows", "kept", "overflow_subbuckets", "chain_jobs", "chain_samples", "sequences", "grouped",
                 "overflow_elements", "overflow_kept", "big_groups", "big_kept", "passes", "valid", "giant_chains",
                 "giant_max", "redone", "cap_overflow_scratch", "cap_split", "cap_long_samples", "cap_long_jobs",
                 "demand_overflow_scratch", "demand_split", "demand_long_samples", "demand_long_jobs",
                 "long_samples", "routed", "add_batch_us", "prepare_upload_us", "prepare_plan_us", "prepare_rest_us",
                 "pass_groups", "add_pack_us", "add_dma_wait_us", "finish_us", "finish_wait_us", "finish_copy_us",
                 "finish_chunks", "finish_select_dev_us", "finish_sort_dev_us", "finish_gather_dev_us",
                 "finish_d2h_dev_us", "finish_max_chunk", "finish_wide_index", "kept_cap",
                 "free_after_prepare", "recs_rot", "overflow_light_subbuckets", "overflow_light_elements",
                 "groupby_tasks", "groupby_batches", "add_fasta_us"]
        return {names[i]: int(v[i]) for i in range(n)}

    def debug_jobs(self, k: int = 64) -> list:
        v = (C.c_uint32 * k)()
        _check(lib().skm_build_debug_jobs(self._h, v, k))
        return [int(x) for x in v]

    def debug_overflow(self, k: int = 4096) -> list:
        """Element counts of the last pass's overflow sub-buckets, largest first."""
        v = (C.c_uint32 * k)()
        n = lib().skm_build_debug_overflow(self._h, v, k)
        return [int(x) for x in v[:min(max(n, 0), k)]]

    def debug_front(self) -> dict:
        """skm_build_debug_front: the geometry of the last run's extraction front end (the
        key-range-pass fields are 0 after a one-pass run)."""
        names = ["rp", "sel_wg", "sel_span", "emit_g", "pf_span", "pf_nwg", "nwg", "span", "pass_bits",
                 "owner_bits", "b1_bits"]
        v = (C.c_uint64 * len(names))()
        n = lib().skm_build_debug_front(self._h, v, len(names))
        _check(min(n, 0))
        assert n == len(names), n
        return {names[i]: int(v[i]) for i in range(n)}

    def debug_stage_starts(self, pass_id: int) -> np.ndarray:
        """skm_build_debug_stage_starts: the (pf_nwg + 1) x 64 table of exact staging starts of a
        key-range pass of the last run's last emission group (row w, column d: where staging
        workgroup w begins in level-0 slice d; the last row: the slices' ends)."""
        rows = self.debug_front()["pf_nwg"] + 1
        out = np.zeros(rows * 64, dtype=np.uint64)
        n = lib().skm_build_debug_stage_starts(self._h, pass_id, out.ctypes.data_as(C.POINTER(C.c_uint64)), out.size)
        _check(min(n, 0))
        assert n == out.size, (n, out.size)
        return out.reshape(rows, 64)

    def debug_pass_windows(self) -> list:
        """skm_build_debug_pass_windows: this rank's windows of every key-range pass of the last run
        (one value, the valid windows, after a one-pass run)."""
        v = (C.c_uint64 * 64)()
        n = lib().skm_build_debug_pass_windows(self._h, v, 64)
        _check(min(n, 0))
        return [int(x) for x in v[:n]]

    def debug_stamps(self, enable: bool) -> list:
        v = (C.c_uint64 * 32)()
        _check(lib().skm_build_debug_stamps(self._h, 1 if enable else 0, v, 32))
        return [int(x) for x in v]

    def finish(self) -> KeptKmers:
        k = _Kept()
        _check(lib().skm_build_finish(self._h, C.byref(k)))
        return self._kept(k)

    def finish_slice(self, slice_bits: int, slice_: int) -> KeptKmers:
        """skm_build_finish_slice: the kept k-mers whose slice hash (fmix64 of the key, top
        slice_bits bits) is slice_, keys sorted; statistics are the whole build's."""
        k = _Kept()
        _check(lib().skm_build_finish_slice(self._h, int(slice_bits), int(slice_), C.byref(k)))
        return self._kept(k)

    def signature_flags(self) -> np.ndarray:
        """Per-sequence signature flags of the last run (sequences with a kept function, add order)."""
        n = self.counters()["sequences"]
        out = np.zeros(max(n, 1), np.uint8)
        _check(lib().skm_build_signature_flags(self._h, _ptr(out), n))
        return out[:n]

    @staticmethod
    def _release_level(release_work) -> int:
        """release_work of kept_db / mph_db: False / True / 2 / "keep_sequences" -> 0 / 1 / 2."""
        if isinstance(release_work, str):
            if release_work != "keep_sequences":
                raise SkmError(f"release_work: unknown value {release_work!r} (False, True, 2 or 'keep_sequences')")
            return 2
        if isinstance(release_work, (bool, np.bool_)):
            return 1 if release_work else 0
        if release_work in (0, 1, 2):
            return int(release_work)
        raise SkmError(f"release_work: unknown value {release_work!r} (False, True, 2 or 'keep_sequences')")

    def resident_seqs(self) -> tuple:
        """skm_build_resident_seqs: (sequences the handle holds -- those added with a kept function, in
        add order -- , their packed bytes, len + 1 each); zeros once release_work=True freed them."""
        n, nb = C.c_uint64(0), C.c_uint64(0)
        _check(lib().skm_build_resident_seqs(self._h, C.byref(n), C.byref(nb)))
        return int(n.value), int(nb.value)

    def recall(self, db: "CmphKmerDb", tables: "FunctionIndexTables | None" = None, *, want_calls: bool = False,
               hypo_index=..., ignore_hypo: bool = False, min_hits: int = 5, max_gap: int = 200,
               batch_residues: int = 0, first_seq: int = 0, n_seqs: int = 0):
        """skm_build_recall: the recall pass (kmers-build-signatures.cc:266-349) over the resident
        sequences [first_seq, first_seq + n_seqs) against db, read in place from the build's HBM
        buffers -- no second upload of the proteins.  With tables: a BestCalls (what
        FunctionCaller.best_seqs gives for the same sequences); with want_calls: (call_off, calls)
        as QueryBatch.calls gives; with both: (BestCalls, call_off, calls).  The result carries
        .stats (skm_recall_stats).  hypo_index defaults to "hypothetical protein" in the tables'
        function index (-1 without tables or without that name)."""
        if tables is None and not want_calls:
            raise SkmError("recall: nothing asked for (tables=None and want_calls=False)")
        if hypo_index is ...:
            hypo_index = -1
            if tables is not None and "hypothetical protein" in tables.function_index:
                hypo_index = tables.function_index.index("hypothetical protein")
        opts = _AnnotOpts(int(min_hits), int(max_gap), int(bool(ignore_hypo)), int(hypo_index), 0, 0)
        ro = _RecallOpts(int(batch_residues), int(first_seq), int(n_seqs))
        best = _BestCalls() if tables is not None else None
        calls = _Calls() if want_calls else None
        st = _RecallStats()
        _check(lib().skm_build_recall(self._h, db._h, C.byref(opts), C.byref(ro), tables._h if tables is not None else None,
                                      C.byref(best) if best is not None else None,
                                      C.byref(calls) if calls is not None else None, C.byref(st)))
        stats = {n: getattr(st, n) for n, _ in _RecallStats._fields_}
        parts = []
        if best is not None:
            parts.append(_best_result(best, tables))
        if calls is not None:
            try:
                n, nc = int(calls.n_seqs), int(calls.n_calls)
                parts.append(np.ctypeslib.as_array(calls.call_off, shape=(n + 1,)).copy())
                parts.append(np.frombuffer(C.string_at(calls.calls, CALL_DTYPE.itemsize * nc), dtype=CALL_DTYPE).copy()
                             if nc else np.zeros(0, CALL_DTYPE))
            finally:
                lib().skm_calls_free(C.byref(calls))
        res = parts[0] if len(parts) == 1 else _RecallResult(parts)
        res.stats = stats
        return res

    def kept_db(self, load_pct: int = 0, slots: int = 0, release_work=False) -> "DeviceKeptKmerDb":
        """skm_build_kept_db: the exact-key DB (KeptKmerDB<8>) over the kept k-mers of the last run,
        built on the device from the resident arena -- no host copy of the kept set.  load_pct /
        slots size its range-reduced table (kept_db_plan); release_work frees the handle's per-pass
        work buffers first, after which the handle can only be read out (finish, finish_slice,
        signature_flags, counters) and closed: run / prepare / add_batch raise SkmError.
        release_work=2 (or "keep_sequences") frees the same except the resident sequences, which
        recall() reads."""
        opts = _KeptDbOpts(int(load_pct), self._release_level(release_work), int(slots))
        h = C.c_void_p()
        _check(lib().skm_build_kept_db(self._h, C.byref(opts), C.byref(h)))
        return DeviceKeptKmerDb(h, self.device)

    def mph_db(self, seed: int = 1, release_work=False, verify: bool = False, mph_path: str | None = None,
               dat_path: str | None = None) -> "CmphKmerDb":
        """skm_build_mph_db: the BDZ signature DB (build_perfect_hash + CmphKmerDb, perfect_hash.h:11-69,
        cmph_kmer.h:95-104) over the kept k-mers of the last run, built and opened on the device from
        the resident arena -- no host copy of the kept set and no file round trip.  The image and the
        .dat, written only where a path is given, are those of mph_build(sorted kept set, seed,
        device=...).  release_work as in kept_db.  The returned DB is independent of the builder; its
        `stats` are mph_build_device's dict (upload_s stays 0)."""
        opts = _MphDbOpts(int(seed), self._release_level(release_work), 1 if verify else 0, 0,
                          mph_path.encode() if mph_path else None, dat_path.encode() if dat_path else None)
        h = C.c_void_p()
        st = _MphStats()
        _check(lib().skm_build_mph_db(self._h, C.byref(opts), C.byref(h), C.byref(st)))
        db = CmphKmerDb(device=self.device, handle=h)
        db.stats = {n: getattr(st, n) for n, _ in _MphStats._fields_ if n != "pad"}
        return db

    def write_final_kmers(self, path: str) -> dict:
        """skm_build_write_final_kmers: final.kmers (kmers-build-signatures.cc:198-221) of the last
        run written to `path` from the resident arena -- sorted, formatted and streamed out by the
        device, no host copy of the kept set and no finish().  One GPU; works after kept_db / mph_db
        released the work buffers.  Returns the call's statistics (skm_final_kmers_stats)."""
        st = _FinalKmersStats()
        _check(lib().skm_build_write_final_kmers(self._h, os.fsencode(path), C.byref(st)))
        return {n: getattr(st, n) for n, _ in _FinalKmersStats._fields_}

    def stats(self) -> KeptKmers:
        """skm_build_stats: what finish() returns without the kept set -- keys and data are empty,
        `n` is the number of kept k-mers.  One GPU; works after a release."""
        k = _Kept()
        _check(lib().skm_build_stats(self._h, C.byref(k)))
        return self._kept(k)

    @staticmethod
    def _kept(k) -> KeptKmers:
        """The library's arrays without a copy: keys / data view the hand-off's host arrays, which
        skm_kept_free releases when the last view is gone."""
        owner = _KeptOwner(k)
        n = int(k.n)
        if n and k.keys:
            kb = (C.c_char * (8 * n)).from_address(C.cast(k.keys, C.c_void_p).value)
            db = (C.c_char * (10 * n)).from_address(C.cast(k.data, C.c_void_p).value)
            kb._owner = db._owner = owner
            keys = np.frombuffer(kb, np.uint64)
            data = np.frombuffer(db, STORED_DTYPE)
        else:
            keys, data = np.zeros(0, np.uint64), np.zeros(0, STORED_DTYPE)
        nf = int(k.n_functions)
        df = np.ctypeslib.as_array(k.distinct_functions, shape=(max(nf, 1),))[:nf].copy()
        sw = np.ctypeslib.as_array(k.seqs_with_func, shape=(max(nf, 1),))[:nf].copy()
        return KeptKmers(keys, data, df, sw, int(k.n_seqs_with_signature), int(k.distinct_signatures),
                         int(k.n_windows), int(k.n), int(k.n_records))

    def close(self):
        if self._h:
            lib().skm_build_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class _RecallResult(tuple):
    """SignatureBuilder.recall's tuple results, with the call's .stats."""


def recall_plan(seq_len, batch_residues: int = 0, first_seq: int = 0, n_seqs: int = 0) -> list:
    """skm_recall_plan (host only, no HIP call): the batches SignatureBuilder.recall cuts for resident
    sequences of these lengths -- a list of dicts first, n, base, pstart, end, windows (base = the
    batch's view start: its first sequence's packed start & ~15; end = after its last separator)."""
    seq_len = np.ascontiguousarray(seq_len, dtype=np.uint32)
    nb = C.c_uint64(0)
    args = (_ptr(seq_len) if len(seq_len) else None, len(seq_len), int(batch_residues), int(first_seq), int(n_seqs))
    _check(lib().skm_recall_plan(*args, None, 0, C.byref(nb)))
    out = np.zeros((max(int(nb.value), 1), 6), np.uint64)
    _check(lib().skm_recall_plan(*args, _ptr(out), int(nb.value), C.byref(nb)))
    names = ("first", "n", "base", "pstart", "end", "windows")
    return [dict(zip(names, (int(v) for v in row))) for row in out[:int(nb.value)]]


class GlooTransport:
    """skm_transport over torch.distributed (the default process group, e.g. gloo on the host):
    the rank collectives of a multi-process build without RCCL (tests; CPU-side channels).
    Callbacks run on the calling thread; an exception is reported as a failed collective."""

    def __init__(self):
        import torch.distributed as dist
        self.dist = dist
        self.rank, self.world = dist.get_rank(), dist.get_world_size()
        self._cbs = (_A2A_T(self._a2a), _RED_T(self._red), _AGV_T(self._agv))
        self.struct = _Transport(None, *self._cbs)
        self.ptr = C.pointer(self.struct)

    @staticmethod
    def _buf(addr, n):
        import torch
        if n == 0:
            return torch.zeros(0, dtype=torch.uint8)
        return torch.frombuffer((C.c_uint8 * n).from_address(addr), dtype=torch.uint8)

    def _a2a(self, ctx, send, scnt, soff, recv, rcnt, roff):
        try:
            W, me = self.world, self.rank
            sc = [int(scnt[i]) for i in range(W)]
            so = [int(soff[i]) for i in range(W)]
            rc = [int(rcnt[i]) for i in range(W)]
            ro = [int(roff[i]) for i in range(W)]
            if sc[me]:
                C.memmove(recv + ro[me], send + so[me], sc[me])
            reqs = []
            for q in range(W):
                if q == me:
                    continue
                if sc[q]:
                    reqs.append(self.dist.isend(self._buf(send + so[q], sc[q]).clone(), q))
                if rc[q]:
                    reqs.append(self.dist.irecv(self._buf(recv + ro[q], rc[q]), q))
            for r in reqs:
                r.wait()
            return 0
        except Exception:  # reported to the library as a failed collective
            import traceback
            traceback.print_exc()
            return -1

    def _red(self, ctx, data, count, op):
        try:
            import torch
            n = int(count)
            if op == 0:
                a = np.ctypeslib.as_array(C.cast(data, C.POINTER(C.c_uint32)), shape=(n,))
                t = torch.from_numpy(a.astype(np.int64))
                self.dist.all_reduce(t, op=self.dist.ReduceOp.SUM)
                a[:] = (t.numpy() & 0xFFFFFFFF).astype(np.uint32)
            else:
                a = np.ctypeslib.as_array(C.cast(data, C.POINTER(C.c_uint8)), shape=(n,))
                t = torch.from_numpy(a.astype(np.int32))
                self.dist.all_reduce(t, op=self.dist.ReduceOp.MAX)
                a[:] = t.numpy().astype(np.uint8)
            return 0
        except Exception:
            import traceback
            traceback.print_exc()
            return -1

    def _agv(self, ctx, send, recv, bytes_per_rank):
        try:
            import torch
            W = self.world
            nb = [int(bytes_per_rank[i]) for i in range(W)]
            m = max(1, max(nb))
            mine = torch.zeros(m, dtype=torch.uint8)
            if nb[self.rank]:
                mine[:nb[self.rank]] = self._buf(send, nb[self.rank])
            outs = [torch.zeros(m, dtype=torch.uint8) for _ in range(W)]
            self.dist.all_gather(outs, mine)
            o = 0
            for r in range(W):
                if nb[r]:
                    self._buf(recv + o, nb[r])[:] = outs[r][:nb[r]]
                o += nb[r]
            return 0
        except Exception:
            import traceback
            traceback.print_exc()
            return -1


def comm_unique_id() -> bytes:
    """128-byte RCCL unique id (rank 0 creates it; broadcast it to every rank's set_comm)."""
    buf = (C.c_uint8 * 128)()
    _check(lib().skm_comm_unique_id(buf))
    return bytes(buf)


def group_run(builders) -> None:
    """Run ranks 0..n-1 of one build inside this process (device-copy exchange instead of RCCL);
    used to test the multi-GPU path on one device."""
    arr = (C.c_void_p * len(builders))(*[b._h.value for b in builders])
    _check(lib().skm_build_group_run(arr, len(builders)))


def mph_build(keys: np.ndarray, data: np.ndarray, mph_path: str, dat_path: str, seed: int = 1,
              device: int | None = None):
    """build_perfect_hash (perfect_hash.h:11-69): cmph-compatible BDZ .mph + dense .dat.
    device=None: host construction; device=d: parallel peeling on GPU d."""
    keys = np.ascontiguousarray(keys, dtype=np.uint64)
    data = np.ascontiguousarray(data, dtype=STORED_DTYPE)
    if device is None:
        _check(lib().skm_mph_build(_ptr(keys), _ptr(data), len(keys), seed, mph_path.encode(), dat_path.encode()))
    else:
        _check(lib().skm_mph_build_device(_ptr(keys), _ptr(data), len(keys), seed, mph_path.encode(),
                                          dat_path.encode(), device))


class _MphStats(C.Structure):
    _fields_ = [(n, C.c_double) for n in ("upload_s", "peel_s", "assign_s", "rank_s", "place_s", "verify_s",
                                          "write_s", "total_s")] + \
               [("n_keys", C.c_uint64), ("n_vertices", C.c_uint64), ("attempts", C.c_uint32),
                ("peel_rounds", C.c_uint32), ("verified", C.c_int32), ("pad", C.c_int32)]


def mph_build_device(keys: np.ndarray, data: np.ndarray, mph_path: str | None = None, dat_path: str | None = None,
                     seed: int = 1, device: int = 0, verify: bool = True) -> dict:
    """skm_mph_build_device_ex: the device BDZ construction (perfect_hash.h:11-69) up to cmph's
    32-bit vertex space, with its phase times; None paths skip writing that image; verify checks
    on the device that the slots are a permutation, that the annotate kernels' pair-line search
    agrees with bdz_search for every key and that every .dat record is its key's."""
    keys = np.ascontiguousarray(keys, dtype=np.uint64)
    data = np.ascontiguousarray(data, dtype=STORED_DTYPE)
    st = _MphStats()
    _check(lib().skm_mph_build_device_ex(_ptr(keys), _ptr(data), len(keys), seed,
                                         mph_path.encode() if mph_path else None,
                                         dat_path.encode() if dat_path else None, device, 1 if verify else 0,
                                         C.byref(st)))
    return {n: getattr(st, n) for n, _ in _MphStats._fields_ if n != "pad"}


class CmphKmerDb:
    """CmphKmerDb<StoredKmerData, 8> (cmph_kmer.h:28-164) resident in HBM."""
    KmerSize = K

    def __init__(self, file_base: str | None = None, device: int = 0, mph: bytes | None = None,
                 dat: bytes | None = None, handle=None):
        self._h = C.c_void_p()
        self.device = device
        if handle is not None:  # an open skm_db (SignatureBuilder.mph_db); this object owns it
            self._h = handle
        elif file_base is not None:
            _check(lib().skm_db_open(C.byref(self._h), (file_base + ".mph").encode(), (file_base + ".dat").encode(),
                                     device))
        else:
            mb = np.frombuffer(mph, dtype=np.uint8)
            db = np.frombuffer(dat, dtype=np.uint8) if dat else np.zeros(0, np.uint8)
            _check(lib().skm_db_open_mem(C.byref(self._h), _ptr(mb), len(mb), _ptr(db), len(db), device))

    def hash_size(self) -> int:
        m = C.c_uint32()
        _check(lib().skm_db_size(self._h, C.byref(m)))
        return m.value

    def lookup_keys(self, keys: np.ndarray) -> np.ndarray:
        """cmph_search per key (lookup_key, cmph_kmer.h:90-92); >= hash_size means miss."""
        keys = np.ascontiguousarray(keys, dtype=np.uint64)
        out = np.zeros(len(keys), dtype=np.uint32)
        if len(keys):
            _check(lib().skm_db_lookup(self._h, _ptr(keys), len(keys), _ptr(out)))
        return out

    def lookup_keys_generic(self, keys: np.ndarray) -> np.ndarray:
        """Test hook: the generic bdz_search walk (skm_debug_db_lookup_generic), bypassing the
        b == 7 (g word, rank) pair lines that lookup_keys and the annotate kernels use."""
        keys = np.ascontiguousarray(keys, dtype=np.uint64)
        out = np.zeros(len(keys), dtype=np.uint32)
        if len(keys):
            _check(lib().skm_debug_db_lookup_generic(self._h, _ptr(keys), len(keys), _ptr(out)))
        return out

    def lookup_fm(self, keys: np.ndarray) -> np.ndarray:
        """skm_db_lookup_fm: per key the record word the call path reads, function_index << 16 |
        mean, or 0xFFFFFFFF for a miss (a BDZ DB: whatever record the search lands on, as fetch)."""
        keys = np.ascontiguousarray(keys, dtype=np.uint64)
        out = np.zeros(len(keys), dtype=np.uint32)
        if len(keys):
            _check(lib().skm_db_lookup_fm(self._h, _ptr(keys), len(keys), _ptr(out)))
        return out

    def table_info(self) -> tuple:
        """skm_db_table_info: (slots, table bytes, keys, longest probe sequence seen at insert, 1 if
        range-reduced); zeros for a BDZ DB."""
        v = (C.c_uint64 * 5)()
        n = lib().skm_db_table_info(self._h, v, 5)
        if n < 0:
            _check(n)
        return tuple(int(x) for x in v)

    def close(self):
        if self._h:
            lib().skm_db_close(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class KeptKmerDb(CmphKmerDb):
    """KeptKmerDB<8> (kept_kmer_db.h:9-31): exact-key DB over a build's kept k-mers, resident in HBM
    (the recall pass's DB, kmers-build-signatures.cc:238).  lookup_keys returns the record index
    of each key, len(keys) for a miss."""

    def __init__(self, keys: np.ndarray, data: np.ndarray, device: int = 0):
        self._h = C.c_void_p()
        self.device = device
        keys = np.ascontiguousarray(keys, dtype=np.uint64)
        data = np.ascontiguousarray(data, dtype=STORED_DTYPE)
        _check(lib().skm_db_open_kept(C.byref(self._h), _ptr(keys), _ptr(data), len(keys), device))


class DeviceKeptKmerDb(CmphKmerDb):
    """The KeptKmerDB<8> that SignatureBuilder.kept_db makes on the device (skm_build_kept_db): a
    range-reduced table of any size, independent of the builder.  lookup_keys returns each key's
    index in the builder's arena (a permutation of 0..n-1 over the members), hash_size() for a
    miss.  It holds no records: MatrixDistance over it raises SkmError."""

    def __init__(self, handle, device: int = 0):
        self._h = handle
        self.device = device


def kept_db_plan(n: int, load_pct: int = 0, slots: int = 0) -> tuple:
    """skm_kept_db_plan (host only): (slots, bytes) of the table SignatureBuilder.kept_db would
    allocate for n kept k-mers."""
    opts = _KeptDbOpts(int(load_pct), 0, int(slots))
    t, b = C.c_uint64(), C.c_uint64()
    _check(lib().skm_kept_db_plan(int(n), C.byref(opts), C.byref(t), C.byref(b)))
    return t.value, b.value


def mph_db_plan(n: int) -> tuple:
    """skm_mph_db_plan (host only): for n kept k-mers, (r of the first attempt, vertices 3r, device
    bytes of the open BDZ DB, most device bytes live while SignatureBuilder.mph_db builds it -- the
    arena not counted)."""
    v = (C.c_uint64 * 4)()
    _check(lib().skm_mph_db_plan(int(n), v))
    return tuple(int(x) for x in v)


def final_kmers_info() -> tuple:
    """skm_final_kmers_info (host only): the device final.kmers formatter's (lines per emit tile,
    threads per workgroup, longest line in bytes, 0)."""
    out = (C.c_uint32 * 4)()
    _check(lib().skm_final_kmers_info(out))
    return tuple(int(x) for x in out)


def final_kmers_host(keys: np.ndarray, data: np.ndarray) -> bytes:
    """skm_debug_final_kmers_host (host only): the final.kmers lines of (keys, data) through the
    formatter the device kernels run."""
    keys = np.ascontiguousarray(keys, dtype=np.uint64)
    data = np.ascontiguousarray(data, dtype=STORED_DTYPE)
    assert len(keys) == len(data)
    n = C.c_uint64()
    _check(lib().skm_debug_final_kmers_host(_ptr(keys), _ptr(data), len(keys), None, 0, C.byref(n)))
    out = np.zeros(max(int(n.value), 1), np.uint8)
    _check(lib().skm_debug_final_kmers_host(_ptr(keys), _ptr(data), len(keys), _ptr(out), int(n.value), C.byref(n)))
    return out[:int(n.value)].tobytes()


def kept_slot(key: int, slots: int) -> int:
    """skm_debug_kept_slot (host only): the home slot of key in a range-reduced table of `slots`."""
    v = C.c_uint64()
    _check(lib().skm_debug_kept_slot(int(key), int(slots), C.byref(v)))
    return v.value


def read_function_index(path: str) -> list:
    """FunctionCaller::read_function_index (call_functions.tcc:123-148): column 1 by id."""
    rows = []
    with open(path, "rb") as f:
        for line in f.read().split(b"\n"):
            if not line:
                continue
            parts = line.split(b"\t")
            rows.append((int(parts[0]), parts[1].decode("latin-1") if len(parts) > 1 else ""))
    n = max((i for i, _ in rows), default=-1) + 1
    out = [""] * n
    for i, s in rows:
        out[i] = s
    return out


def fasta_parse_info() -> tuple:
    """skm_fasta_parse_info: the device FASTA parser's (bytes per thread step, bytes per wave step,
    bytes per workgroup tile)."""
    out = (C.c_uint32 * 4)()
    _check(lib().skm_fasta_parse_info(out))
    return int(out[0]), int(out[1]), int(out[2])


def _fasta_input(blobs):
    """The files of a device parse as (bytes u8, file_off u64[n_files + 1]): a sequence of
    bytes-like objects laid back to back, or such a pair as it is."""
    if isinstance(blobs, tuple) and len(blobs) == 2 and isinstance(blobs[0], np.ndarray):
        return (np.ascontiguousarray(blobs[0], dtype=np.uint8), np.ascontiguousarray(blobs[1], dtype=np.uint64))
    off = np.zeros(len(blobs) + 1, np.uint64)
    if len(blobs):
        off[1:] = np.cumsum([len(b) for b in blobs], dtype=np.uint64)
    return np.frombuffer(b"".join(bytes(b) for b in blobs), dtype=np.uint8), off


class FastaTable:
    """skm_fasta_table: the kept records (non-empty id) of a device FASTA parse -- file_rec
    [n_files + 1], seq_len [n_recs], hdr_pos [n_recs] (the position of each record's '>'), the
    totals, the parse's device ms and, when asked for, the packed residues."""

    def __init__(self, t: "_FastaTable"):
        nf, nr = int(t.n_files), int(t.n_recs)
        self.n_files, self.n_recs = nf, nr
        self.n_residues, self.n_windows = int(t.n_residues), int(t.n_windows)
        self.parse_ms = float(t.parse_ms)
        self.file_rec = np.ctypeslib.as_array(t.file_rec, shape=(nf + 1,)).copy()
        self.seq_len = np.ctypeslib.as_array(t.seq_len, shape=(nr,)).copy() if nr else np.zeros(0, np.uint32)
        self.hdr_pos = np.ctypeslib.as_array(t.hdr_pos, shape=(nr,)).copy() if nr else np.zeros(0, np.uint64)
        rp = self.n_residues + nr
        self.residues = None
        if t.residues:
            self.residues = np.ctypeslib.as_array(t.residues, shape=(rp,)).copy() if rp else np.zeros(0, np.uint8)


def fasta_parse_device(blobs, device: int = 0, want_residues: bool = False) -> FastaTable:
    """skm_fasta_parse_device: FastaParser (fasta_parser.h:38-144) over the files' bytes on the
    device; blobs as _fasta_input takes them."""
    data, off = _fasta_input(blobs)
    t = _FastaTable()
    _check(lib().skm_fasta_parse_device(_ptr(data), _ptr(off), len(off) - 1, device, int(want_residues), C.byref(t)))
    try:
        return FastaTable(t)
    finally:
        lib().skm_fasta_table_free(C.byref(t))


class FunctionIndexTables:
    """skm_fidx: function.index reduced to the ids find_best_call needs (name ranks, part ids), on
    the host and -- device >= 0 -- on that device; device < 0 makes no HIP call."""

    def __init__(self, function_index, device: int = 0):
        self.function_index = list(function_index)
        self.device = device
        self._h = C.c_void_p()
        arr = _fi_array(self.function_index)
        _check(lib().skm_fidx_create(C.byref(self._h), arr, len(self.function_index), device))

    def name(self, best) -> str:
        """skm_best_call_name of one BEST_DTYPE element."""
        return self.names(np.array(best, dtype=BEST_DTYPE).reshape(1))[0]

    def names(self, best: np.ndarray) -> list:
        """skm_best_call_name of every element: name(fi), "f1 ?? f2" or ""."""
        best = np.ascontiguousarray(best, dtype=BEST_DTYPE)
        fn, h, base = lib().skm_best_call_name, self._h, best.ctypes.data
        cap = 4096
        buf = C.create_string_buffer(cap)
        out = []
        for k in range(len(best)):
            n = fn(h, base + 16 * k, buf, cap)
            if n < 0:
                _check(n)
            if n >= cap:
                cap = n + 1
                buf = C.create_string_buffer(cap)
                fn(h, base + 16 * k, buf, cap)
            out.append(buf.value.decode("latin-1"))
        return out

    def close(self):
        if self._h:
            lib().skm_fidx_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class BestCalls:
    """skm_best_calls: .best (BEST_DTYPE [n_seqs]), the counts, the kernel's device ms, and
    names() through the tables that made it."""

    def __init__(self, out: "_BestCalls", tables: FunctionIndexTables):
        n = int(out.n_seqs)
        self.best = (np.frombuffer(C.string_at(out.best, BEST_DTYPE.itemsize * n), dtype=BEST_DTYPE).copy()
                     if n else np.zeros(0, BEST_DTYPE))
        self.n_seqs, self.n_calls, self.n_windows = n, int(out.n_calls), int(out.n_windows)
        self.n_deferred = int(out.n_deferred)
        self.kernel_ms = float(out.kernel_ms)
        self.tables = tables

    def names(self) -> list:
        return self.tables.names(self.best)


def _best_result(out, tables):
    try:
        return BestCalls(out, tables)
    finally:
        lib().skm_best_calls_free(C.byref(out))


def best_calls_host(call_off, calls, tables: FunctionIndexTables, n_threads: int = 16) -> BestCalls:
    """skm_best_calls_host: find_best_call for every sequence of a CSR of calls, on host threads."""
    call_off = np.ascontiguousarray(call_off, dtype=np.uint64)
    calls = np.ascontiguousarray(calls, dtype=CALL_DTYPE)
    c = _Calls(call_off.ctypes.data_as(C.POINTER(C.c_uint64)), _ptr(calls) if len(calls) else None,
               len(call_off) - 1, len(calls), 0)
    out = _BestCalls()
    _check(lib().skm_best_calls_host(C.byref(c), tables._h, n_threads, C.byref(out)))
    return _best_result(out, tables)


def debug_best_calls(call_off, calls, tables: FunctionIndexTables, device: int = 0):
    """skm_debug_best_calls: a CSR of calls through the kernel alone -> (best, deferred u8, ms)."""
    call_off = np.ascontiguousarray(call_off, dtype=np.uint64)
    calls = np.ascontiguousarray(calls, dtype=CALL_DTYPE)
    n = len(call_off) - 1
    best = np.zeros(n, BEST_DTYPE)
    deferred = np.zeros(n, np.uint8)
    ms = C.c_float()
    _check(lib().skm_debug_best_calls(_ptr(calls) if len(calls) else None, _ptr(call_off), n, tables._h, device,
                                      _ptr(best) if n else None, _ptr(deferred) if n else None, C.byref(ms)))
    return best, deferred, ms.value


class QueryBatch:
    """A batch of query sequences resident in HBM (skm_query_*): run() repeats the device pipeline
    (window lookup + HitSet calls) without re-uploading; timings() = the last run's device ms."""

    @classmethod
    def from_fasta(cls, db: "CmphKmerDb", blobs) -> "QueryBatch":
        """skm_query_create_fasta: the queries are the kept records of the files' bytes, parsed on
        the device; .table is their FastaTable."""
        data, off = _fasta_input(blobs)
        q = cls.__new__(cls)
        q._h = C.c_void_p()
        q.db = db
        t = _FastaTable()
        _check(lib().skm_query_create_fasta(C.byref(q._h), db._h, _ptr(data), _ptr(off), len(off) - 1, C.byref(t)))
        try:
            q.table = FastaTable(t)
        finally:
            lib().skm_fasta_table_free(C.byref(t))
        q._n_seqs = q.table.n_recs
        return q

    def __init__(self, db: CmphKmerDb, residues, seq_off, seq_len):
        self._h = C.c_void_p()
        self.db = db
        residues = np.ascontiguousarray(residues, dtype=np.uint8)
        seq_off = np.ascontiguousarray(seq_off, dtype=np.uint64)
        seq_len = np.ascontiguousarray(seq_len, dtype=np.uint32)
        self._n_seqs = len(seq_len)
        _check(lib().skm_query_create(C.byref(self._h), db._h, _ptr(residues), _ptr(seq_off), _ptr(seq_len),
                                      len(seq_len)))

    def run(self, hypo_index: int, ignore_hypo: bool = False, min_hits: int = 5, max_gap: int = 200):
        opts = _AnnotOpts(min_hits, max_gap, int(ignore_hypo), hypo_index, 0, 0)
        _check(lib().skm_query_run(self._h, C.byref(opts)))

    def timings(self) -> dict:
        ms = (C.c_float * 4)()
        n = lib().skm_query_last_timings(self._h, ms, 4)
        return dict(zip(["lookup", "hitset", "compact", "total"], list(ms)[:n]))

    def calls(self):
        out = _Calls()
        _check(lib().skm_query_calls(self._h, C.byref(out)))
        try:
            n, nc = int(out.n_seqs), int(out.n_calls)
            off = np.ctypeslib.as_array(out.call_off, shape=(n + 1,)).copy()
            calls = (np.frombuffer(C.string_at(out.calls, CALL_DTYPE.itemsize * nc), dtype=CALL_DTYPE).copy()
                     if nc else np.zeros(0, CALL_DTYPE))
            return off, calls
        finally:
            lib().skm_calls_free(C.byref(out))

    def best_calls(self, tables: "FunctionIndexTables") -> "BestCalls":
        """skm_query_best_calls: find_best_call on the resident calls of the last run."""
        out = _BestCalls()
        _check(lib().skm_query_best_calls(self._h, tables._h, C.byref(out)))
        return _best_result(out, tables)

    def window_hits(self):
        """skm_query_window_hits: (hit_off [n+1], pos, fm) of the last run -- every window the
        device lookup found in the DB, as (offset in its sequence, function_index << 16 | mean)."""
        n_seqs = self._n_seqs
        off = np.zeros(n_seqs + 1, np.uint64)
        n = C.c_uint64(0)
        _check(lib().skm_query_window_hits(self._h, _ptr(off), None, None, 0, C.byref(n)))
        pos = np.zeros(max(int(n.value), 1), np.uint32)
        fm = np.zeros(max(int(n.value), 1), np.uint32)
        _check(lib().skm_query_window_hits(self._h, _ptr(off), _ptr(pos), _ptr(fm), len(pos), C.byref(n)))
        return off, pos[:n.value], fm[:n.value]

    def close(self):
        if self._h:
            lib().skm_query_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class FunctionCaller:
    """FunctionCaller<CmphKmerDb> (call_functions.h:60-136) with the per-window lookup and HitSet
    state machine on the GPU and find_best_call on the host (find_best_call, per sequence) or on
    the resident calls of the whole batch (best_seqs / best_fasta)."""

    def __init__(self, db: CmphKmerDb, function_index, min_hits: int = 5, max_gap: int = 200,
                 mean_mode: int = 0, mad_mode: int = 0):
        """mean_mode / mad_mode: the Boost.Math the reference was compiled against
        (call_functions.tcc:51-53): 0 / 0 = >= 1.76 (four-lane mean, |x(mid) - median| MAD),
        1 / 1 = the older single running mean and the MAD that returns |x(mid)|."""
        self.db = db
        self.function_index = read_function_index(function_index) if isinstance(function_index, str) \
            else list(function_index)
        self.min_hits = min_hits
        self.max_gap = max_gap
        self.ignore_hypothetical_ = False
        self.mean_mode = mean_mode
        self.mad_mode = mad_mode
        try:
            self.hypo_index = self.function_index.index("hypothetical protein")
        except ValueError:
            self.hypo_index = -1
        self._fi_arr = _fi_array(self.function_index)

    def ignore_hypothetical(self, x: bool):
        self.ignore_hypothetical_ = bool(x)

    def _opts(self):
        return _AnnotOpts(self.min_hits, self.max_gap, 1 if self.ignore_hypothetical_ else 0, self.hypo_index,
                          self.mean_mode, self.mad_mode)

    def process_seqs(self, residues, seq_off, seq_len):
        """process_aa_seq for a batch: returns (call_off u64[n+1], calls CALL_DTYPE)."""
        if self.hypo_index < 0:  # call_functions.tcc:269-274 exits the process
            raise SkmError("Cannot find hypothetical protein index")
        residues = np.ascontiguousarray(residues, dtype=np.uint8)
        seq_off = np.ascontiguousarray(seq_off, dtype=np.uint64)
        seq_len = np.ascontiguousarray(seq_len, dtype=np.uint32)
        out = _Calls()
        opts = self._opts()
        _check(lib().skm_annotate(self.db._h, _ptr(residues), _ptr(seq_off), _ptr(seq_len), len(seq_len),
                                  C.byref(opts), C.byref(out)))
        try:
            n = int(out.n_seqs)
            off = np.ctypeslib.as_array(out.call_off, shape=(n + 1,)).copy()
            nc = int(out.n_calls)
            calls = (np.frombuffer(C.string_at(out.calls, CALL_DTYPE.itemsize * nc), dtype=CALL_DTYPE).copy()
                     if nc else np.zeros(0, CALL_DTYPE))
            return off, calls
        finally:
            lib().skm_calls_free(C.byref(out))

    def process_fasta(self, blobs):
        """process_fasta_stream's device half (call_functions.tcc:217-255) from the files' bytes
        (skm_annotate_fasta: FastaParser on the device, then process_aa_seq per kept record):
        returns (file_rec, seq_len, hdr_pos, call_off, calls); self.last_fasta is the FastaTable."""
        if self.hypo_index < 0:  # call_functions.tcc:269-274 exits the process
            raise SkmError("Cannot find hypothetical protein index")
        data, foff = _fasta_input(blobs)
        out = _Calls()
        t = _FastaTable()
        opts = self._opts()
        _check(lib().skm_annotate_fasta(self.db._h, _ptr(data), _ptr(foff), len(foff) - 1, C.byref(opts), C.byref(out),
                                        C.byref(t)))
        try:
            tab = self.last_fasta = FastaTable(t)
            n, nc = int(out.n_seqs), int(out.n_calls)
            off = np.ctypeslib.as_array(out.call_off, shape=(n + 1,)).copy()
            calls = (np.frombuffer(C.string_at(out.calls, CALL_DTYPE.itemsize * nc), dtype=CALL_DTYPE).copy()
                     if nc else np.zeros(0, CALL_DTYPE))
            return tab.file_rec, tab.seq_len, tab.hdr_pos, off, calls
        finally:
            lib().skm_calls_free(C.byref(out))
            lib().skm_fasta_table_free(C.byref(t))

    def tables(self) -> "FunctionIndexTables":
        """The function-index tables on the DB's device, made on first use and kept."""
        if getattr(self, "_tables", None) is None:
            self._tables = FunctionIndexTables(self.function_index, self.db.device)
        return self._tables

    def best_seqs(self, residues, seq_off, seq_len) -> "BestCalls":
        """process_aa_seq + find_best_call for a batch, both on the device (skm_annotate_best)."""
        if self.hypo_index < 0:  # call_functions.tcc:269-274 exits the process
            raise SkmError("Cannot find hypothetical protein index")
        residues = np.ascontiguousarray(residues, dtype=np.uint8)
        seq_off = np.ascontiguousarray(seq_off, dtype=np.uint64)
        seq_len = np.ascontiguousarray(seq_len, dtype=np.uint32)
        out = _BestCalls()
        opts = self._opts()
        _check(lib().skm_annotate_best(self.db._h, _ptr(residues), _ptr(seq_off), _ptr(seq_len), len(seq_len),
                                       C.byref(opts), self.tables()._h, C.byref(out)))
        return _best_result(out, self.tables())

    def best_fasta(self, blobs) -> "BestCalls":
        """process_fasta + find_best_call from the files' bytes (skm_annotate_fasta_best);
        self.last_fasta is the FastaTable."""
        if self.hypo_index < 0:  # call_functions.tcc:269-274 exits the process
            raise SkmError("Cannot find hypothetical protein index")
        data, foff = _fasta_input(blobs)
        out = _BestCalls()
        t = _FastaTable()
        opts = self._opts()
        _check(lib().skm_annotate_fasta_best(self.db._h, _ptr(data), _ptr(foff), len(foff) - 1, C.byref(opts),
                                             self.tables()._h, C.byref(out), C.byref(t)))
        try:
            self.last_fasta = FastaTable(t)
        finally:
            lib().skm_fasta_table_free(C.byref(t))
        return _best_result(out, self.tables())

    def find_best_call(self, calls: np.ndarray):
        """find_best_call (call_functions.tcc:347-659) -> (function_index, function, score, offset)."""
        return _find_best_call(calls, self._fi_arr, len(self.function_index))


def _fi_array(function_index):
    return (C.c_char_p * max(1, len(function_index)))(*[s.encode("latin-1") for s in function_index])


def _find_best_call(calls, fi_arr, nfunc):
    calls = np.ascontiguousarray(calls, dtype=CALL_DTYPE)
    fi = C.c_uint16()
    score = C.c_float()
    off = C.c_float()
    buf = C.create_string_buffer(4096)
    _check(lib().skm_find_best_call(_ptr(calls) if len(calls) else None, len(calls), fi_arr, nfunc, C.byref(fi),
                                    C.byref(score), C.byref(off), buf, 4096))
    return fi.value, buf.value.decode("latin-1"), score.value, off.value


def find_best_call(calls: np.ndarray, function_index):
    """Host find_best_call (call_functions.tcc:347-659) over one sequence's calls, without a DB:
    -> (function_index, function, score, offset)."""
    return _find_best_call(calls, _fi_array(function_index), len(function_index))


class SeqIdMap:
    """SeqIdMap (seq_id_map.h:7-35): id -> index in order of first appearance."""

    def __init__(self):
        self._index = {}
        self._ids = []

    def lookup_id(self, id_: str) -> int:
        i = self._index.get(id_)
        if i is None:
            i = len(self._ids)
            self._index[id_] = i
            self._ids.append(id_)
        return i

    def lookup_index(self, i: int) -> str:
        return self._ids[i]

    def __len__(self):
        return len(self._ids)


def matrix_tile_rows(n_idx: int, rank: int, world: int):
    """Row band [begin, end) of GPU `rank` of `world` with (nearly) equal upper-triangle area."""
    a, b = C.c_uint32(), C.c_uint32()
    _check(lib().skm_matrix_tile_rows(n_idx, rank, world, C.byref(a), C.byref(b)))
    return a.value, b.value


class MatrixDistance:
    """MatrixDistance<FunctionCaller<CmphKmerDb>> (matrix_distance.h:30-179) / kmers-matrix-distance
    (kmers-matrix-distance.cc:94-212): shared-signature-k-mer counts over every pair of query
    sequences, on the GPU (skm_matrix_*).  seq_idx: SeqIdMap index per sequence (default: 0..n-1);
    rows=(begin, end) restricts the counts to pairs whose first index lies in [begin, end) -- one
    GPU's tile (matrix_tile_rows)."""

    def __init__(self, db: CmphKmerDb, function_index, residues, seq_off, seq_len, seq_idx=None,
                 n_idx: int | None = None):
        self.db = db
        fi = read_function_index(function_index) if isinstance(function_index, str) else list(function_index)
        if "hypothetical protein" not in fi:  # call_functions.tcc:269-274 exits the process
            raise SkmError("Cannot find hypothetical protein index")
        self.hypo_index = fi.index("hypothetical protein")
        residues = np.ascontiguousarray(residues, dtype=np.uint8)
        seq_off = np.ascontiguousarray(seq_off, dtype=np.uint64)
        seq_len = np.ascontiguousarray(seq_len, dtype=np.uint32)
        if seq_idx is None:
            seq_idx = np.arange(len(seq_len), dtype=np.uint32)
        seq_idx = np.ascontiguousarray(seq_idx, dtype=np.uint32)
        self.n_idx = int(n_idx if n_idx is not None else (int(seq_idx.max()) + 1 if len(seq_idx) else 0))
        self._h = C.c_void_p()
        _check(lib().skm_matrix_create(C.byref(self._h), db._h, _ptr(residues), _ptr(seq_off), _ptr(seq_len),
                                       _ptr(seq_idx), len(seq_len), self.n_idx))

    def set_transport(self, transport: "GlooTransport"):
        """Join the ranks of a multi-GPU matrix distance through a host transport: this handle's
        queries are rank transport.rank's range; run() becomes collective and pairs() returns the
        rank's row band (skm_matrix_tile_rows)."""
        self._transport = transport
        _check(lib().skm_matrix_set_transport(self._h, transport.rank, transport.world, transport.ptr))

    def set_comm(self, unique_id: bytes, rank: int, world: int):
        """Join the ranks over RCCL (collective; rank 0's comm_unique_id broadcast to every rank)."""
        buf = (C.c_uint8 * 128).from_buffer_copy(bytes(unique_id))
        _check(lib().skm_matrix_set_comm(self._h, rank, world, buf))

    def run(self, rows=None, max_tile_bytes: int = 0):
        a, b = rows if rows is not None else (0, 0)
        opts = _MatrixOpts(self.hypo_index, a, b, 0, max_tile_bytes)
        _check(lib().skm_matrix_run(self._h, C.byref(opts)))

    def timings(self) -> dict:
        ms = (C.c_float * 5)()
        n = lib().skm_matrix_last_timings(self._h, ms, 5)
        return dict(zip(["hits", "group", "pairs", "emit", "total"], list(ms)[:n]))

    def counters(self) -> dict:
        v = (C.c_uint64 * 7)()
        n = lib().skm_matrix_counters(self._h, v, 7)
        return dict(zip(["windows", "hits", "increments", "pairs", "kmers", "local_hits", "routed"],
                        [int(x) for x in list(v)[:n]]))

    def pairs(self) -> np.ndarray:
        """(n, 3) u32 (id1, id2, count), id1 < id2, sorted by (id1, id2)."""
        out = _Pairs()
        _check(lib().skm_matrix_pairs(self._h, C.byref(out)))
        try:
            n = int(out.n)
            if n == 0:
                return np.zeros((0, 3), np.uint32)
            return np.ctypeslib.as_array(out.pairs, shape=(n * 3,)).reshape(n, 3).copy()
        finally:
            lib().skm_pairs_free(C.byref(out))

    def compute(self, rows=None):
        self.run(rows)
        return self.pairs()

    def close(self):
        if self._h:
            lib().skm_matrix_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class MatrixDistanceBatch:
    """Many independent MatrixDistance problems in one device pass (skm_matrix_batch_*): what
    kmers-matrix-distance-folder / -merge run per family.  Problem p owns the sequences
    [prob_seq[p], prob_seq[p+1]) and its own SeqIdMap index space; seq_idx is local to each problem
    (default: 0..n-1 within each) and prob_nidx its index count (default: max index + 1, or the
    sequence count when seq_idx is None)."""

    def __init__(self, db: CmphKmerDb, function_index, residues, seq_off, seq_len, prob_seq, seq_idx=None,
                 prob_nidx=None):
        self.db = db
        fi = read_function_index(function_index) if isinstance(function_index, str) else list(function_index)
        if "hypothetical protein" not in fi:  # call_functions.tcc:269-274 exits the process
            raise SkmError("Cannot find hypothetical protein index")
        self.hypo_index = fi.index("hypothetical protein")
        residues = np.ascontiguousarray(residues, dtype=np.uint8)
        seq_off = np.ascontiguousarray(seq_off, dtype=np.uint64)
        seq_len = np.ascontiguousarray(seq_len, dtype=np.uint32)
        prob_seq = np.ascontiguousarray(prob_seq, dtype=np.uint64)
        self.n_prob = max(len(prob_seq) - 1, 0)
        if len(prob_seq) == 0:
            prob_seq = np.zeros(1, np.uint64)
        ps = prob_seq.astype(np.int64)
        if int(ps[-1]) != len(seq_len) or (len(ps) > 1 and np.any(np.diff(ps) < 0)) or int(ps[0]) != 0:
            raise SkmError("prob_seq must rise from 0 to the number of sequences")
        cnt = np.diff(ps)
        if seq_idx is None:
            seq_idx = np.arange(len(seq_len), dtype=np.int64) - np.repeat(ps[:-1], cnt)
            if prob_nidx is None:
                prob_nidx = cnt
        seq_idx = np.ascontiguousarray(seq_idx, dtype=np.uint32)
        if prob_nidx is None:
            prob_nidx = np.zeros(self.n_prob, np.int64)
            if len(seq_idx):
                np.maximum.at(prob_nidx, np.repeat(np.arange(self.n_prob), cnt), seq_idx.astype(np.int64) + 1)
        prob_nidx = np.ascontiguousarray(prob_nidx, dtype=np.uint32)
        if len(prob_nidx) != self.n_prob:
            raise SkmError("prob_nidx must have one entry per problem")
        self.prob_nidx = prob_nidx
        self._h = C.c_void_p()
        _check(lib().skm_matrix_batch_create(C.byref(self._h), db._h, _ptr(residues), _ptr(seq_off), _ptr(seq_len),
                                             _ptr(seq_idx), _ptr(prob_seq), _ptr(prob_nidx), self.n_prob))

    def run(self, small_cols: int = 0):
        opts = _MatrixBatchOpts(self.hypo_index, small_cols)
        _check(lib().skm_matrix_batch_run(self._h, C.byref(opts)))

    def timings(self) -> dict:
        ms = (C.c_float * 5)()
        n = lib().skm_matrix_batch_last_timings(self._h, ms, 5)
        return dict(zip(["hits", "group", "pairs", "emit", "total"], list(ms)[:n]))

    def counters(self) -> dict:
        v = (C.c_uint64 * 7)()
        n = lib().skm_matrix_batch_counters(self._h, v, 7)
        return dict(zip(["windows", "hits", "increments", "pairs", "groups", "rows_small", "rows_large"],
                        [int(x) for x in list(v)[:n]]))

    def group_counts(self) -> np.ndarray:
        """Distinct hit k-mers of each problem (its kmer_hit_map size, matrix_distance.h:110)."""
        v = (C.c_uint64 * max(self.n_prob, 1))()
        _check(lib().skm_matrix_batch_group_counts(self._h, v))
        return np.array(list(v)[:self.n_prob], np.uint64)

    def pairs_flat(self):
        """((n, 3) u32 triples of every problem back to back, prob_off[P+1])."""
        out = _Pairs()
        off = (C.c_uint64 * (self.n_prob + 1))()
        _check(lib().skm_matrix_batch_pairs(self._h, C.byref(out), off))
        try:
            n = int(out.n)
            flat = (np.ctypeslib.as_array(out.pairs, shape=(n * 3,)).reshape(n, 3).copy() if n
                    else np.zeros((0, 3), np.uint32))
            return flat, np.array(list(off), np.uint64)
        finally:
            lib().skm_pairs_free(C.byref(out))

    def pairs(self) -> list:
        """One (n, 3) u32 (id1, id2, count) array per problem, indices local to the problem, id1 < id2,
        sorted by (id1, id2)."""
        flat, off = self.pairs_flat()
        return [flat[int(off[p]):int(off[p + 1])] for p in range(self.n_prob)]

    def compute(self, small_cols: int = 0) -> list:
        self.run(small_cols)
        return self.pairs()

    def close(self):
        if self._h:
            lib().skm_matrix_batch_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
