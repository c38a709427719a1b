"""ctypes binding of include/phj.h (libphj_hip.so, built in-tree).

Plumbing for tests and bench.py: the product's host driver is C++
(partitionedhashjoin_amd/host, the `phjoin` CLI). This module fails loudly
when the HIP library is missing — there is no CPU fallback.
"""
from __future__ import annotations

import ctypes as C
import os

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("PHJ_LIB") or os.path.join(HERE, "libphj_hip.so")   # PHJ_LIB: an A/B build of the same sources

PHJ_OK = 0
PHJ_ERR_INVALID = -1
PHJ_ERR_NOMEM = -2
PHJ_ERR_HIP = -3
PHJ_ERR_STATE = -4
PHJ_ERR_RANGE = -5

ALGO_NO_PARTITIONING = 0
ALGO_RADIX = 1
HASH_XXH3 = 0
HASH_MURMUR3 = 1
SIDE_BUILD = 0
SIDE_PROBE = 1
MAX_TIMERS = 32
TIMER_NAME = 24

# Every symbol include/phj.h declares (tests check the .so exports them all).
EXPORTED = [
    "phj_abi_version", "phj_ctx_create", "phj_ctx_destroy", "phj_last_error",
    "phj_ctx_set_stream", "phj_ctx_synchronize", "phj_relation_upload",
    "phj_relation_bind_device", "phj_relation_device_ptr", "phj_relation_download",
    "phj_relation_generate_sequential", "phj_relation_generate_zipf",
    "phj_relation_count_in_range", "phj_join", "phj_partition", "phj_join_partitioned",
    "phj_partitioned_download", "phj_hash_keys", "phj_timers_report", "phj_join_partitioned_async",
    "phj_prepare", "phj_join_materialize", "phj_joined_rows", "phj_joined_download",
    "phj_ctx_create_ex", "phj_ctx_create_device", "phj_comm_unique_id", "phj_ctx_create_rank",
    "phj_ctx_info", "phj_shard_range", "phj_probe_pass1", "phj_debug_poison_chunk_table", "phj_debug_poison_alloc", "phj_debug_fail_member", "phj_debug_exchange_block", "phj_exchange_geometry",
    "phj_exchange_layout", "phj_count_contribution", "phj_count_verdict", "phj_join_path",
    "phj_join_inner_count", "phj_join_inner", "phj_join_rows_count", "phj_join_rows",
    "phj_debug_preagg", "phj_join_aggregate", "phj_group_rows", "phj_group_download",
    "phj_relation_upload_columns", "phj_relation_bind_columns", "phj_relation_to_columns",
    "phj_relation_columns", "phj_relation_info_get",
    "phj_join_indices", "phj_joined_indices", "phj_joined_indices_download", "phj_gather_column",
    "phj_join_member",
    "phj_index_build", "phj_index_info_get", "phj_index_lookup", "phj_index_destroy",
    "phj_index_build_ex", "phj_index_flags_get", "phj_index_uniques", "phj_index_encode", "phj_index_accumulate",
]
ABI_VERSION = 2
CTX_EXCHANGE = 0x1   # phj_ctx_create_ex: the multi-GPU path on one device (RCCL world of one)
CTX_LOCAL = 0x2      # ... exchange by device copies; devices may repeat (rehearsal on one GPU)
UNIQUE_ID_BYTES = 128
INDEX_ORDINALS = 0x1  # phj_index_build_ex: a dense id per distinct key (encode, accumulate, uniques)
PATH_NO_PARTITIONING, PATH_LDS_JOIN, PATH_CODE_TABLES, PATH_PARTITIONED = 0, 1, 2, 3   # phj_join_path
# phj_join_rows: the row classes and the join kinds they make
ROWS_PAIRS, ROWS_PROBE_ONLY, ROWS_BUILD_ONLY = 0x1, 0x2, 0x4
INNER, PROBE_OUTER, BUILD_OUTER, FULL_OUTER, PROBE_ANTI, BUILD_ANTI = 1, 3, 5, 7, 2, 4
NULL_PAYLOAD = -2**63   # the default marker for the missing side (INT64_MIN)
AGG_GROUPS, AGG_MATCHED_ONLY = 0x1, 0x2   # phj_join_aggregate's flags
LAYOUT_TUPLES, LAYOUT_COLUMNS = 0, 1   # phj_relation_info.layout
NO_ROW = -1   # PHJ_NO_ROW: the missing side's row number in phj_join_indices' columns
MEMBER_PROBE, MEMBER_BUILD = 0x1, 0x2   # phj_join_member's sides


class Tuple(C.Structure):
    """phj_tuple == Common::Tuple (src/Common/Table.hpp:20-25)."""
    _fields_ = [("id", C.c_int64), ("payload", C.c_int64)]


class JoinParams(C.Structure):
    _fields_ = [("algo", C.c_int32), ("hash", C.c_int32), ("hash_seed", C.c_uint64),
                ("num_partitions", C.c_uint32), ("radix_bits", C.c_uint8 * 2),
                ("flags", C.c_uint8), ("reserved", C.c_uint8),
                ("table_ratio", C.c_double)]


class JoinResult(C.Structure):
    _fields_ = [("matches", C.c_uint64), ("partition_ms", C.c_double), ("build_ms", C.c_double),
                ("probe_ms", C.c_double), ("total_ms", C.c_double), ("exchange_ms", C.c_double),
                ("algorithmic_bytes", C.c_uint64), ("num_partitions", C.c_uint32),
                ("num_timers", C.c_uint32), ("timer_ms", C.c_double * MAX_TIMERS),
                ("timer_bytes", C.c_uint64 * MAX_TIMERS),
                ("timer_name", (C.c_char * TIMER_NAME) * MAX_TIMERS)]

    def timers(self):
        return [(self.timer_name[i].value.decode(), self.timer_ms[i], self.timer_bytes[i])
                for i in range(self.num_timers)]

    def as_dict(self):
        return {"matches": self.matches, "partition_ms": self.partition_ms,
                "build_ms": self.build_ms, "probe_ms": self.probe_ms, "total_ms": self.total_ms,
                "exchange_ms": self.exchange_ms,
                "algorithmic_bytes": self.algorithmic_bytes,
                "num_partitions": self.num_partitions, "timers": self.timers()}


class RowCounts(C.Structure):
    """phj_row_counts: rows per class of phj_join_rows / phj_join_rows_count."""
    _fields_ = [("pairs", C.c_uint64), ("probe_only", C.c_uint64), ("build_only", C.c_uint64),
                ("rows", C.c_uint64)]

    def as_dict(self):
        return {"pairs": self.pairs, "probe_only": self.probe_only, "build_only": self.build_only,
                "rows": self.rows}


class JoinTotals(C.Structure):
    """phj_join_totals: the aggregates of phj_join_aggregate over R join S
    (every sum modulo 2^64)."""
    _fields_ = [("pairs", C.c_uint64), ("probe_matched", C.c_uint64), ("sum_a", C.c_int64),
                ("sum_b", C.c_int64), ("sum_ab", C.c_int64)]

    def as_dict(self):
        return {"pairs": self.pairs, "probe_matched": self.probe_matched, "sum_a": self.sum_a,
                "sum_b": self.sum_b, "sum_ab": self.sum_ab}


class MemberCounts(C.Structure):
    """phj_member_counts: rows with a partner, per side, of phj_join_member."""
    _fields_ = [("probe_matched", C.c_uint64), ("build_matched", C.c_uint64)]

    def as_dict(self):
        return {"probe_matched": self.probe_matched, "build_matched": self.build_matched}


class IndexInfo(C.Structure):
    """phj_index_info: what a retained key index holds and its table's geometry."""
    _fields_ = [("rows", C.c_uint64), ("distinct", C.c_uint64), ("table_bytes", C.c_uint64),
                ("nb", C.c_uint32), ("nbr", C.c_uint32), ("rbits", C.c_uint32), ("slots", C.c_uint32)]

    def as_dict(self):
        return {"rows": self.rows, "distinct": self.distinct, "table_bytes": self.table_bytes,
                "nb": self.nb, "nbr": self.nbr, "rbits": self.rbits, "slots": self.slots}


class GroupRow(C.Structure):
    """phj_group_row: a build tuple, its probe partners and the sum of their payloads."""
    _fields_ = [("id", C.c_int64), ("payload_a", C.c_int64), ("partners", C.c_uint64), ("sum_b", C.c_int64)]


class RelationInfo(C.Structure):
    """phj_relation_info: how a side is bound (tuples or columns; whether a
    payload column is bound; whether the context holds a packed tuple copy)."""
    _fields_ = [("n", C.c_uint64), ("layout", C.c_uint32), ("has_payloads", C.c_uint32),
                ("packed", C.c_uint32), ("owned", C.c_uint32)]

    def as_dict(self):
        return {"n": self.n, "layout": self.layout, "has_payloads": self.has_payloads,
                "packed": self.packed, "owned": self.owned}


class Partitioned(C.Structure):
    _fields_ = [("keys", C.c_void_p), ("payloads", C.c_void_p), ("bounds", C.c_void_p),
                ("n", C.c_uint64), ("num_partitions", C.c_uint32), ("reserved", C.c_uint32)]


_lib = None


class PhjError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"phj error {code}: {msg}")
        self.code = code


def load():
    """Load libphj_hip.so; raise if it was not built (no fallback path exists)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError(f"{LIB_PATH} is missing: run `make` or __graft_entry__.build() first "
                          "(the HIP extension is required; there is no CPU fallback)")
    L = C.CDLL(LIB_PATH)
    P = C.c_void_p
    u64, i64, i, d = C.c_uint64, C.c_int64, C.c_int, C.c_double
    sig = {
        "phj_abi_version": (i, []),
        "phj_ctx_create": (i, [i, C.POINTER(i), C.POINTER(P)]),
        "phj_ctx_create_ex": (i, [i, C.POINTER(i), C.c_uint32, C.POINTER(P)]),
        "phj_ctx_create_device": (i, [i, C.POINTER(P)]),
        "phj_comm_unique_id": (i, [C.c_char_p]),
        "phj_ctx_create_rank": (i, [i, i, i, C.c_char_p, C.POINTER(P)]),
        "phj_ctx_info": (i, [P, C.POINTER(i), C.POINTER(i), C.POINTER(i)]),
        "phj_shard_range": (None, [u64, i, i, C.POINTER(u64), C.POINTER(u64)]),
        "phj_exchange_layout": (None, [u64, C.c_uint32, C.POINTER(u64), C.POINTER(u64)]),
        "phj_count_contribution": (None, [u64, i, C.POINTER(u64)]),
        "phj_count_verdict": (i, [C.POINTER(u64), C.POINTER(u64)]),
        "phj_join_path": (i, [C.POINTER(JoinParams), u64, u64]),
        "phj_ctx_destroy": (None, [P]),
        "phj_last_error": (C.c_char_p, [P]),
        "phj_ctx_set_stream": (i, [P, P]),
        "phj_ctx_synchronize": (i, [P]),
        "phj_relation_upload": (i, [P, i, P, u64]),
        "phj_relation_bind_device": (i, [P, i, P, u64]),
        "phj_relation_device_ptr": (P, [P, i, C.POINTER(u64)]),
        "phj_relation_download": (i, [P, i, P, u64]),
        "phj_relation_upload_columns": (i, [P, i, P, P, u64]),
        "phj_relation_bind_columns": (i, [P, i, P, P, u64]),
        "phj_relation_to_columns": (i, [P, i, i]),
        "phj_relation_columns": (i, [P, i, C.POINTER(P), C.POINTER(P), C.POINTER(u64)]),
        "phj_relation_info_get": (i, [P, i, C.POINTER(RelationInfo)]),
        "phj_relation_generate_sequential": (i, [P, i, u64, i64, u64]),
        "phj_relation_generate_zipf": (i, [P, i, u64, d, i64, i64, u64, u64]),
        "phj_relation_count_in_range": (i, [P, i, i64, i64, C.POINTER(u64)]),
        "phj_join": (i, [P, C.POINTER(JoinParams), C.POINTER(JoinResult)]),
        "phj_partition": (i, [P, i, C.POINTER(JoinParams), C.POINTER(Partitioned)]),
        "phj_join_partitioned": (i, [P, C.POINTER(JoinParams), i, C.POINTER(Partitioned),
                                     C.POINTER(JoinResult)]),
        "phj_partitioned_download": (i, [P, C.POINTER(Partitioned), P, P, P]),
        "phj_hash_keys": (i, [P, i, u64, P, u64, P]),
        "phj_probe_pass1": (i, [P, P, P, u64, P, P, P]),
        "phj_debug_poison_chunk_table": (i, [P, i, P, i]),
        "phj_debug_poison_alloc": (i, [P, i]),
        "phj_debug_preagg": (i, [P, i, C.POINTER(u64)]),
        "phj_debug_fail_member": (i, [P, i]),
        "phj_debug_exchange_block": (i, [P, i, P, u64]),
        "phj_exchange_geometry": (i, [P, u64, P, P, P, P, P]),
        "phj_timers_report": (i, [P, C.POINTER(JoinResult)]),
        "phj_join_partitioned_async": (i, [P, C.POINTER(JoinParams), i, C.POINTER(Partitioned), P]),
        "phj_prepare": (i, [P, C.POINTER(JoinParams)]),
        "phj_join_materialize": (i, [P, C.POINTER(JoinParams), C.POINTER(JoinResult)]),
        "phj_join_inner_count": (i, [P, C.POINTER(JoinParams), C.POINTER(JoinResult)]),
        "phj_join_inner": (i, [P, C.POINTER(JoinParams), C.POINTER(JoinResult)]),
        "phj_join_rows_count": (i, [P, C.POINTER(JoinParams), C.c_uint32, C.POINTER(JoinResult),
                                    C.POINTER(RowCounts)]),
        "phj_join_rows": (i, [P, C.POINTER(JoinParams), C.c_uint32, i64, C.POINTER(JoinResult),
                              C.POINTER(RowCounts)]),
        "phj_joined_rows": (P, [P, C.POINTER(u64)]),
        "phj_joined_download": (i, [P, P, u64]),
        "phj_join_aggregate": (i, [P, C.POINTER(JoinParams), C.c_uint32, C.POINTER(JoinResult),
                                   C.POINTER(JoinTotals)]),
        "phj_group_rows": (P, [P, C.POINTER(u64)]),
        "phj_group_download": (i, [P, P, u64]),
        "phj_join_indices": (i, [P, C.POINTER(JoinParams), C.c_uint32, C.POINTER(JoinResult),
                                 C.POINTER(RowCounts)]),
        "phj_joined_indices": (i, [P, C.POINTER(P), C.POINTER(P), C.POINTER(u64)]),
        "phj_joined_indices_download": (i, [P, P, P, u64]),
        "phj_gather_column": (i, [P, P, u64, P, u64, C.POINTER(i64), P]),
        "phj_join_member": (i, [P, C.POINTER(JoinParams), C.c_uint32, P, P, C.POINTER(JoinResult),
                                C.POINTER(MemberCounts)]),
        "phj_index_build": (i, [P, C.POINTER(JoinParams), C.POINTER(P), C.POINTER(JoinResult)]),
        "phj_index_info_get": (i, [P, C.POINTER(IndexInfo)]),
        "phj_index_lookup": (i, [P, P, P, C.c_uint32, u64, P, P, P]),
        "phj_index_destroy": (None, [P, P]),
        "phj_index_build_ex": (i, [P, C.POINTER(JoinParams), C.c_uint32, C.POINTER(P), C.POINTER(JoinResult)]),
        "phj_index_flags_get": (i, [P, C.POINTER(C.c_uint32)]),
        "phj_index_uniques": (i, [P, P, C.POINTER(P), C.POINTER(u64)]),
        "phj_index_encode": (i, [P, P, P, C.c_uint32, u64, P, P, P]),
        "phj_index_accumulate": (i, [P, P, P, C.c_uint32, P, C.c_uint32, u64, P, P, P]),
    }
    for name, (res, args) in sig.items():
        f = getattr(L, name, None)
        if f is None:
            # only an A/B build of older sources (PHJ_LIB) may lack a symbol:
            # a call it lacks then fails at the call
            if os.environ.get("PHJ_LIB"):
                continue
            raise ImportError(f"{LIB_PATH} does not export {name}: rebuild it (`make`)")
        f.restype = res
        f.argtypes = args
    _lib = L
    return L
