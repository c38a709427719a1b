"""partitionedhashjoin_amd — MI355X-native radix-partitioned / no-partitioning hash join.

The product is the HIP library libphj_hip.so (C ABI: include/phj.h) plus the
C++ host driver `phjoin` that keeps the reference's CLI, Configuration and
Table<Tuple> API (ragoragino/partitionedhashjoin, src/main.cpp). This Python
module is plumbing over the same C ABI for tests, bench.py and the
torch.distributed multi-GPU driver. It never falls back to a CPU path:
without the built HIP library every entry point raises.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _capi
from ._capi import (AGG_GROUPS, AGG_MATCHED_ONLY, ALGO_NO_PARTITIONING, ALGO_RADIX, BUILD_ANTI, BUILD_OUTER, CTX_EXCHANGE, CTX_LOCAL, FULL_OUTER,
                    HASH_MURMUR3, HASH_XXH3, INNER, NULL_PAYLOAD, PATH_CODE_TABLES, PATH_LDS_JOIN,
                    PATH_NO_PARTITIONING, PATH_PARTITIONED, PROBE_ANTI, PROBE_OUTER, ROWS_BUILD_ONLY, ROWS_PAIRS,
                    ROWS_PROBE_ONLY, SIDE_BUILD, SIDE_PROBE, GroupRow, JoinParams, JoinResult, JoinTotals, Partitioned,
                    PhjError, RowCounts, LAYOUT_TUPLES, LAYOUT_COLUMNS, RelationInfo, NO_ROW,
                    MEMBER_PROBE, MEMBER_BUILD, MemberCounts, IndexInfo)

__all__ = ["Context", "shard_range", "exchange_layout", "join_path", "PATH_LDS_JOIN", "PATH_CODE_TABLES",
           "PATH_PARTITIONED", "PATH_NO_PARTITIONING", "count_contribution", "count_verdict", "comm_unique_id", "CTX_EXCHANGE", "CTX_LOCAL", "radix_params", "nopart_params", "JoinParams", "JoinResult",
           "Partitioned", "PhjError", "ALGO_RADIX", "ALGO_NO_PARTITIONING", "HASH_XXH3",
           "HASH_MURMUR3", "SIDE_BUILD", "SIDE_PROBE", "DEFAULT_SEED", "RowCounts", "ROWS_PAIRS", "ROWS_PROBE_ONLY",
           "ROWS_BUILD_ONLY", "INNER", "PROBE_OUTER", "BUILD_OUTER", "FULL_OUTER", "PROBE_ANTI", "BUILD_ANTI",
           "NULL_PAYLOAD", "JoinTotals", "GroupRow", "AGG_GROUPS", "AGG_MATCHED_ONLY",
           "RelationInfo", "LAYOUT_TUPLES", "LAYOUT_COLUMNS", "NO_ROW",
           "MEMBER_PROBE", "MEMBER_BUILD", "MemberCounts", "Index", "IndexInfo"]

DEFAULT_SEED = 0x9E3779B97F4A7C15
PART_STABLE = 0x1   # include/phj.h PHJ_PART_STABLE
TABLE_CHAINED = 0x2   # include/phj.h PHJ_TABLE_CHAINED
DEFER_TIMERS = 0x4   # include/phj.h PHJ_DEFER_TIMERS: timers read later by Context.timers_report()
LEAN_TIMERS = 0x8    # include/phj.h PHJ_LEAN_TIMERS: only the critical path's large kernels timed
PREAGG_AUTO, PREAGG_OFF, PREAGG_FORCED = 0, 1, 2   # include/phj.h phj_debug_preagg's modes


def radix_params(bits=(8, 8), num_partitions=0, hash=HASH_MURMUR3, seed=DEFAULT_SEED,
                 stable=False, chained=False) -> JoinParams:
    """RadixCluster parameters. num_partitions > 0 reproduces the reference's
    `hash % P` partitioning (`phjoin -p P`); otherwise q = hash & (2^(b0+b1)-1).
    stable=True asks `partition` for the reference's exact layout (input order
    inside each partition, RadixCluster/HashJoin.hpp:394-412); otherwise the
    order inside a partition is unspecified (PHJ_PART_STABLE, include/phj.h).
    chained=True builds bucket-chained tables, the reference's
    SeparateChainingHashTable (PHJ_TABLE_CHAINED)."""
    p = JoinParams()
    p.flags = (PART_STABLE if stable else 0) | (TABLE_CHAINED if chained else 0)
    p.algo = ALGO_RADIX
    p.hash = hash
    p.hash_seed = seed
    p.num_partitions = num_partitions
    p.radix_bits[0] = bits[0]
    p.radix_bits[1] = bits[1] if len(bits) > 1 else 0
    p.table_ratio = 0.0
    return p


def nopart_params(hash=HASH_XXH3, seed=DEFAULT_SEED, table_ratio=0.0) -> JoinParams:
    p = JoinParams()
    p.algo = ALGO_NO_PARTITIONING
    p.hash = hash
    p.hash_seed = seed
    p.table_ratio = table_ratio
    return p


def shard_range(n: int, rank: int, world: int):
    """Rows [lo, hi) of an n-row relation held by `rank` of `world` ranks: the
    range sharding of every multi-device context (phj_shard_range; host only)."""
    L = _capi.load()
    lo, hi = C.c_uint64(), C.c_uint64()
    L.phj_shard_range(n, rank, world, C.byref(lo), C.byref(hi))
    return lo.value, hi.value


def exchange_layout(max_shard: int, num_partitions: int):
    """(codes_elems, block_elems) of one rank's exchange block: codes, padding
    (unspecified, never read), then num_partitions + 1 uint32 bounds
    (phj_exchange_layout; host only)."""
    L = _capi.load()
    a, b = C.c_uint64(), C.c_uint64()
    L.phj_exchange_layout(max_shard, num_partitions, C.byref(a), C.byref(b))
    return a.value, b.value


def exchange_geometry(params: JoinParams, total_build: int):
    """(num_segments, shift, sub_bits, sub_shift, cluster) of the member step's
    exchange block for radix params and a global build side of total_build rows
    (phj_exchange_geometry; host only, default tuning)."""
    L = _capi.load()
    n, sh, sb, ss, cl = C.c_uint32(), C.c_uint32(), C.c_uint32(), C.c_uint32(), C.c_int()
    rc = L.phj_exchange_geometry(C.byref(params), total_build, C.byref(n), C.byref(sh), C.byref(sb), C.byref(ss),
                                 C.byref(cl))
    if rc != 0:
        raise PhjError(rc, "phj_exchange_geometry: radix params required")
    return n.value, sh.value, sb.value, ss.value, bool(cl.value)


def join_path(params: JoinParams, build_n: int, probe_n: int) -> int:
    """The counting path phj_join takes on one device (phj_join_path; host
    only, default tuning): PATH_LDS_JOIN, PATH_CODE_TABLES, PATH_PARTITIONED
    or PATH_NO_PARTITIONING."""
    rc = _capi.load().phj_join_path(C.byref(params), build_n, probe_n)
    if rc < 0:
        raise PhjError(rc, "phj_join_path: bad params")
    return rc


def count_contribution(count: int, failed: bool = False) -> np.ndarray:
    """The two uint64 words a rank adds to the count all-reduce (phj_count_contribution)."""
    L = _capi.load()
    w = (C.c_uint64 * 2)()
    L.phj_count_contribution(count, 1 if failed else 0, w)
    return np.array([w[0], w[1]], dtype=np.uint64)


def count_verdict(words) -> int:
    """The global count from the all-reduced words; PhjError(PHJ_ERR_STATE) when a
    rank failed (phj_count_verdict)."""
    L = _capi.load()
    w = (C.c_uint64 * 2)(int(words[0]), int(words[1]))
    m = C.c_uint64()
    rc = L.phj_count_verdict(w, C.byref(m))
    if rc != 0:
        raise PhjError(rc, f"{int(words[1])} rank(s) failed during the join")
    return m.value


def comm_unique_id() -> bytes:
    """A fresh RCCL unique id (rank 0 makes it; every rank passes it to
    Context.rank)."""
    L = _capi.load()
    buf = C.create_string_buffer(_capi.UNIQUE_ID_BYTES)
    rc = L.phj_comm_unique_id(buf)
    if rc != 0:
        raise PhjError(rc, "phj_comm_unique_id failed (RCCL unavailable?)")
    return buf.raw


class Context:
    """A phj_ctx: one HIP device (Context(device)), several devices driven by
    this process (Context(devices=[...]), the multi-GPU join; flags
    CTX_EXCHANGE / CTX_LOCAL), or one rank of a multi-process job
    (Context.rank)."""

    def __init__(self, device: int = 0, devices=None, flags: int = 0, _handle=None):
        self._L = _capi.load()
        self._keep = {}
        if _handle is not None:
            self._h = _handle
            self.device = device
            return
        h = C.c_void_p()
        if devices is None:
            rc = self._L.phj_ctx_create_device(device, C.byref(h))
            what = f"phj_ctx_create_device({device})"
        else:
            arr = (C.c_int * len(devices))(*devices)
            rc = self._L.phj_ctx_create_ex(len(devices), arr, flags, C.byref(h))
            what = f"phj_ctx_create_ex({list(devices)}, flags={flags})"
            device = devices[0]
        if rc != 0:
            raise PhjError(rc, f"{what} failed")
        self._h = h
        self.device = device

    @classmethod
    def rank(cls, device: int, nranks: int, rank: int, unique_id: bytes) -> "Context":
        """One device of a multi-process job (phj_ctx_create_rank): every call
        on it is collective over the ranks."""
        L = _capi.load()
        h = C.c_void_p()
        rc = L.phj_ctx_create_rank(device, nranks, rank, unique_id, C.byref(h))
        if rc != 0:
            raise PhjError(rc, f"phj_ctx_create_rank(device={device}, {rank}/{nranks}) failed")
        return cls(device, _handle=h)

    def info(self):
        """(world, rank of the first local device, local devices)"""
        w, r, n = C.c_int(), C.c_int(), C.c_int()
        self._check(self._L.phj_ctx_info(self._h, C.byref(w), C.byref(r), C.byref(n)))
        return w.value, r.value, n.value

    # -- lifecycle --
    def close(self):
        if getattr(self, "_h", None):
            for ix in getattr(self, "_indexes", []):   # phj_ctx_destroy frees the survivors
                ix._h = None
            self._indexes = []
            self._L.phj_ctx_destroy(self._h)
            self._h = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc):
        if rc != 0:
            raise PhjError(rc, self._L.phj_last_error(self._h).decode())

    def set_stream(self, stream_ptr: int | None):
        self._check(self._L.phj_ctx_set_stream(self._h, C.c_void_p(stream_ptr or 0)))

    def synchronize(self):
        self._check(self._L.phj_ctx_synchronize(self._h))

    # -- relations --
    def upload(self, side: int, rel: np.ndarray):
        rel = np.ascontiguousarray(rel, dtype=np.int64)
        assert rel.ndim == 2 and rel.shape[1] == 2
        self._check(self._L.phj_relation_upload(self._h, side, rel.ctypes.data_as(C.c_void_p),
                                                rel.shape[0]))

    def bind_device(self, side: int, ptr: int, n: int, keepalive=None):
        self._keep[side] = keepalive
        self._check(self._L.phj_relation_bind_device(self._h, side, C.c_void_p(ptr), n))

    def upload_columns(self, side: int, keys, payloads=None):
        """phj_relation_upload_columns: bind host columns (int64 key column and,
        unless None, a payload column of the same length) as the relation of
        `side`, copied to context-owned device memory."""
        keys = np.ascontiguousarray(keys, dtype=np.int64)
        assert keys.ndim == 1
        pp = None
        if payloads is not None:
            payloads = np.ascontiguousarray(payloads, dtype=np.int64)
            assert payloads.shape == keys.shape
            pp = payloads.ctypes.data_as(C.c_void_p)
        self._keep[side] = None
        self._check(self._L.phj_relation_upload_columns(self._h, side, keys.ctypes.data_as(C.c_void_p), pp,
                                                        keys.shape[0]))

    def bind_columns(self, side: int, keys_ptr: int, payloads_ptr: int | None, n: int, keepalive=None):
        """phj_relation_bind_columns: borrow device columns (8-byte aligned
        addresses, e.g. two torch tensors' data_ptr(); payloads_ptr None or 0:
        the key column alone). `keepalive` is held while they are bound."""
        self._keep[side] = keepalive
        self._check(self._L.phj_relation_bind_columns(self._h, side, C.c_void_p(keys_ptr),
                                                      C.c_void_p(payloads_ptr or 0), n))

    def to_columns(self, side: int, payloads: bool = True):
        """phj_relation_to_columns: split the bound tuple relation into
        context-owned columns on the device (payloads=False: the keys alone)."""
        self._check(self._L.phj_relation_to_columns(self._h, side, 1 if payloads else 0))

    def columns_ptr(self, side: int):
        """(keys_ptr, payloads_ptr, n) of a columnar binding; the pointers are
        None for a tuple binding (and payloads_ptr for a key column alone)."""
        k, p, n = C.c_void_p(), C.c_void_p(), C.c_uint64()
        self._check(self._L.phj_relation_columns(self._h, side, C.byref(k), C.byref(p), C.byref(n)))
        return k.value, p.value, n.value

    def relation_info(self, side: int) -> RelationInfo:
        info = RelationInfo()
        self._check(self._L.phj_relation_info_get(self._h, side, C.byref(info)))
        return info

    def relation_ptr(self, side: int):
        n = C.c_uint64()
        p = self._L.phj_relation_device_ptr(self._h, side, C.byref(n))
        return p, n.value

    def download(self, side: int, n: int | None = None) -> np.ndarray:
        if n is None:
            n = self.relation_ptr(side)[1]
        out = np.zeros((n, 2), dtype=np.int64)
        self._check(self._L.phj_relation_download(self._h, side, out.ctypes.data_as(C.c_void_p), n))
        return out

    def generate_sequential(self, side: int, n: int, start: int = 1, first_index: int = 0):
        self._check(self._L.phj_relation_generate_sequential(self._h, side, n, start, first_index))

    def generate_zipf(self, side: int, n: int, alpha: float, lo: int, hi: int, seed: int,
                      first_index: int = 0):
        self._check(self._L.phj_relation_generate_zipf(self._h, side, n, alpha, lo, hi, seed,
                                                       first_index))

    def count_in_range(self, side: int, lo: int, hi: int) -> int:
        c = C.c_uint64()
        self._check(self._L.phj_relation_count_in_range(self._h, side, lo, hi, C.byref(c)))
        return c.value

    # -- join --
    def prepare(self, params: JoinParams) -> None:
        """Allocate join's workspace for the bound relations (nothing runs)."""
        self._check(self._L.phj_prepare(self._h, C.byref(params)))

    def join(self, params: JoinParams) -> JoinResult:
        r = JoinResult()
        self._check(self._L.phj_join(self._h, C.byref(params), C.byref(r)))
        return r

    def join_materialize(self, params: JoinParams) -> JoinResult:
        """phj_join_materialize: the join's rows (JoinedTuple) in a device buffer;
        r.matches rows. Read them with joined()."""
        r = JoinResult()
        self._check(self._L.phj_join_materialize(self._h, C.byref(params), C.byref(r)))
        return r

    def join_inner_count(self, params: JoinParams) -> JoinResult:
        """phj_join_inner_count: r.matches = |R join S|, the number of (build
        tuple, probe tuple) pairs with equal ids (64-bit exact); no rows."""
        r = JoinResult()
        self._check(self._L.phj_join_inner_count(self._h, C.byref(params), C.byref(r)))
        return r

    def join_inner(self, params: JoinParams) -> JoinResult:
        """phj_join_inner: the inner join's rows, one per (build tuple, probe
        tuple) pair, grouped by probe tuple; r.matches rows. Read them with
        joined(). Raises PhjError (PHJ_ERR_RANGE) at 2^32 pairs or more."""
        r = JoinResult()
        self._check(self._L.phj_join_inner(self._h, C.byref(params), C.byref(r)))
        return r

    def join_rows_count(self, params: JoinParams, classes: int):
        """phj_join_rows_count: (JoinResult, RowCounts) of the join kind
        `classes` (a set of ROWS_PAIRS / ROWS_PROBE_ONLY / ROWS_BUILD_ONLY, or
        one of INNER ... BUILD_ANTI); no rows. r.matches == counts.rows."""
        r, n = JoinResult(), RowCounts()
        self._check(self._L.phj_join_rows_count(self._h, C.byref(params), classes, C.byref(r), C.byref(n)))
        return r, n

    def join_rows(self, params: JoinParams, classes: int, null_payload: int = NULL_PAYLOAD):
        """phj_join_rows: the rows of the join kind `classes`: the probe part
        (pair rows and, for a probe tuple without a partner, {id, null_payload,
        payloadB}) grouped by probe tuple, then {id, payloadA, null_payload}
        per build tuple nobody asked for. Returns (JoinResult, RowCounts);
        read the rows with joined(). Raises PhjError (PHJ_ERR_RANGE) at 2^32
        rows or more."""
        r, n = JoinResult(), RowCounts()
        self._check(self._L.phj_join_rows(self._h, C.byref(params), classes, null_payload, C.byref(r),
                                          C.byref(n)))
        return r, n

    def joined(self, n: int | None = None) -> np.ndarray:
        """Rows of the last materialised join as an (n, 3) int64 array
        {id, payloadA (build), payloadB (probe)}."""
        total = C.c_uint64(0)
        self._L.phj_joined_rows(self._h, C.byref(total))
        n = total.value if n is None else n
        out = np.zeros((n, 3), dtype=np.int64)
        self._check(self._L.phj_joined_download(self._h, out.ctypes.data_as(C.c_void_p), n))
        return out

    def join_indices(self, params: JoinParams, classes: int):
        """phj_join_indices: the join kind `classes` as two int64 index columns
        (build row, probe row; NO_ROW for the missing side), in join_rows' row
        order. Only keys are read: any binding will do, a key column alone
        included, and nothing is packed. Returns (JoinResult, RowCounts); read
        the columns with joined_indices() or hand joined_indices_ptr() to a
        gather. Raises PhjError (PHJ_ERR_RANGE) at 2^32 rows or more."""
        r, n = JoinResult(), RowCounts()
        self._check(self._L.phj_join_indices(self._h, C.byref(params), classes, C.byref(r), C.byref(n)))
        return r, n

    def joined_indices_ptr(self):
        """(build_rows device pointer, probe_rows device pointer, n) of the last
        join_indices: ctx-owned, valid until the next materialised or index
        join; the pointers are None when there are no rows."""
        b, p, n = C.c_void_p(), C.c_void_p(), C.c_uint64(0)
        self._check(self._L.phj_joined_indices(self._h, C.byref(b), C.byref(p), C.byref(n)))
        return b.value, p.value, n.value

    def joined_indices(self, n: int | None = None):
        """The index columns of the last join_indices as two np.int64 arrays
        (build_rows, probe_rows)."""
        n = self.joined_indices_ptr()[2] if n is None else n
        b, p = np.zeros(n, dtype=np.int64), np.zeros(n, dtype=np.int64)
        self._check(self._L.phj_joined_indices_download(self._h, b.ctypes.data_as(C.c_void_p),
                                                        p.ctypes.data_as(C.c_void_p), n))
        return b, p

    def joined_indices_to(self, build_ptr: int | None, probe_ptr: int | None, n: int) -> None:
        """Copy the first n entries of the index columns to device memory at
        build_ptr / probe_ptr (None: skip that column)."""
        self._check(self._L.phj_joined_indices_download(self._h, C.c_void_p(build_ptr), C.c_void_p(probe_ptr), n))

    def gather_column(self, src_ptr: int, src_n: int, idx_ptr: int, n: int, null_value: int | None,
                      out_ptr: int) -> None:
        """phj_gather_column on device pointers: out[i] = src[idx[i]]; where
        idx[i] == NO_ROW, out[i] = null_value, or stays as it is when
        null_value is None. Raises PhjError (PHJ_ERR_RANGE) when other indices
        lay outside [0, src_n): they are not dereferenced."""
        nv = None if null_value is None else C.byref(C.c_int64(null_value))
        self._check(self._L.phj_gather_column(self._h, C.c_void_p(src_ptr), src_n, C.c_void_p(idx_ptr), n, nv,
                                              C.c_void_p(out_ptr)))

    def join_aggregate(self, params: JoinParams, groups: bool = False, matched_only: bool = False):
        """phj_join_aggregate: (JoinResult, JoinTotals) of R join S without its
        rows: pairs, probe tuples with a partner, and the sums over the pairs
        of the build payload, the probe payload and their product (modulo
        2^64); no limit at 2^32 pairs. groups=True also leaves one row per
        build tuple (matched_only=True: per build tuple with a partner) for
        groups(). r.matches == totals.pairs."""
        flags = (AGG_GROUPS if groups else 0) | (AGG_MATCHED_ONLY if matched_only else 0)
        r, t = JoinResult(), JoinTotals()
        self._check(self._L.phj_join_aggregate(self._h, C.byref(params), flags, C.byref(r), C.byref(t)))
        return r, t

    def join_member(self, params: JoinParams, probe: bool = True, build: bool = False,
                    probe_mask_ptr: int | None = None, build_mask_ptr: int | None = None):
        """phj_join_member: which rows have a partner on the other side, one
        byte per row in the relation's own order (probe: the probe side's mask,
        build: the build side's). Only keys are read and nothing is packed; the
        schedule is the same whatever `params` asks for beyond hash and seed.
        Returns (JoinResult, MemberCounts, probe_mask, build_mask). A mask whose
        device pointer is passed (any alignment, e.g. a torch.bool tensor's
        data_ptr()) is written there and None is returned in its place;
        otherwise the call allocates it on the device, downloads it and returns
        a numpy bool array (None for a side that is not asked)."""
        sides = (MEMBER_PROBE if probe else 0) | (MEMBER_BUILD if build else 0)
        ptrs, own = [], []   # own[k]: None, or (scratch context holding the mask or None, rows) of a mask made here
        r, cnt = JoinResult(), MemberCounts()
        try:
            for side, asked, ptr in ((SIDE_PROBE, probe, probe_mask_ptr), (SIDE_BUILD, build, build_mask_ptr)):
                own.append(None)
                if asked and ptr is None:
                    n = self.relation_ptr(side)[1]
                    donor = None
                    if n:   # device memory for the mask: a scratch context's key column of ceil(n / 8) words
                        donor = Context(self.device)
                        own[-1] = (donor, n)
                        donor.upload_columns(SIDE_PROBE, np.zeros((n + 7) // 8, dtype=np.int64))
                        ptr = donor.columns_ptr(SIDE_PROBE)[0]
                    own[-1] = (donor, n)
                ptrs.append(ptr if asked else None)
            self._check(self._L.phj_join_member(self._h, C.byref(params), sides, C.c_void_p(ptrs[0] or 0),
                                                C.c_void_p(ptrs[1] or 0), C.byref(r), C.byref(cnt)))
            masks = []
            for o in own:
                if o is None:
                    masks.append(None)
                elif o[0] is None:
                    masks.append(np.zeros(0, dtype=bool))
                else:
                    words = np.ascontiguousarray(o[0].download(SIDE_PROBE)[:, 0])
                    masks.append(words.view(np.uint8)[:o[1]].astype(bool))
        finally:
            for o in own:
                if o is not None and o[0] is not None:
                    o[0].close()
        return r, cnt, masks[0], masks[1]

    def build_index(self, params: JoinParams, ordinals: bool = False) -> "Index":
        """phj_index_build: a retained key index over the build side as bound
        (keys only; any binding, a key column alone included): each distinct
        key once with the lowest row that carries it. The index owns its
        memory and outlives later joins and rebinds of this context; close it
        with Index.close() (closing the context closes its indexes). The
        build's JoinResult is Index.result (matches = the distinct keys).
        ordinals=True (phj_index_build_ex, PHJ_INDEX_ORDINALS) also numbers the
        distinct keys 0 .. distinct-1 in first-appearance order: Index.encode,
        Index.accumulate and Index.first_rows need it."""
        h, r = C.c_void_p(), JoinResult()
        if ordinals:
            self._check(self._L.phj_index_build_ex(self._h, C.byref(params), _capi.INDEX_ORDINALS, C.byref(h), C.byref(r)))
        else:
            self._check(self._L.phj_index_build(self._h, C.byref(params), C.byref(h), C.byref(r)))
        ix = Index(self, h, r)
        if not hasattr(self, "_indexes"):
            self._indexes = []
        self._indexes.append(ix)
        return ix

    def groups(self, n: int | None = None) -> np.ndarray:
        """Group rows of the last join_aggregate as an (n, 4) int64 array
        {id, payloadA, partners, sum of the partners' payloads}, in unspecified
        order; the partners column is a uint64 reinterpreted as int64."""
        total = C.c_uint64(0)
        self._L.phj_group_rows(self._h, C.byref(total))
        n = total.value if n is None else n
        out = np.zeros((n, 4), dtype=np.int64)
        self._check(self._L.phj_group_download(self._h, out.ctypes.data_as(C.c_void_p), n))
        return out

    def partition(self, side: int, params: JoinParams) -> Partitioned:
        v = Partitioned()
        self._check(self._L.phj_partition(self._h, side, C.byref(params), C.byref(v)))
        return v

    def join_partitioned(self, params: JoinParams, segments) -> JoinResult:
        arr = (Partitioned * len(segments))(*segments)
        r = JoinResult()
        self._check(self._L.phj_join_partitioned(self._h, C.byref(params), len(segments), arr,
                                                 C.byref(r)))
        return r

    def join_partitioned_async(self, params: JoinParams, segments, dev_count: int) -> None:
        """Enqueue build + probe; the count lands at device address dev_count (uint64)."""
        arr = (Partitioned * len(segments))(*segments)
        self._check(self._L.phj_join_partitioned_async(self._h, C.byref(params), len(segments), arr,
                                                       C.c_void_p(dev_count)))

    def timers_report(self) -> JoinResult:
        r = JoinResult()
        self._check(self._L.phj_timers_report(self._h, C.byref(r)))
        return r

    def download_partitioned(self, v: Partitioned):
        keys = np.zeros(v.n, dtype=np.int64)
        pays = np.zeros(v.n, dtype=np.int64)
        bounds = np.zeros(v.num_partitions + 1, dtype=np.uint32)
        self._check(self._L.phj_partitioned_download(
            self._h, C.byref(v), keys.ctypes.data_as(C.c_void_p), pays.ctypes.data_as(C.c_void_p),
            bounds.ctypes.data_as(C.c_void_p)))
        return keys, pays, bounds

    def probe_pass1(self, params: JoinParams):
        """Test hook (phj_probe_pass1): the probe side's pass-1 output as the
        counting join's on-chip probe consumes it, pass-1 digit major.
        Returns (keys or hash codes, bounds1 (nb1 + 1), is_codes)."""
        n = self.relation_ptr(SIDE_PROBE)[1]
        out = np.zeros(n, dtype=np.int64)
        b1 = np.zeros(2049, dtype=np.uint32)
        nb1, codes = C.c_uint32(), C.c_int()
        self._check(self._L.phj_probe_pass1(self._h, C.byref(params), out.ctypes.data_as(C.c_void_p), n,
                                            b1.ctypes.data_as(C.c_void_p), C.byref(nb1), C.byref(codes)))
        return out, b1[:nb1.value + 1].copy(), bool(codes.value)

    def debug_poison_chunk_table(self, side: int, params: JoinParams, byte: int = 0xFF) -> None:
        """Test hook (phj_debug_poison_chunk_table): leave `side`'s chunk table
        as a stale one would be (every byte = `byte`, marked clean)."""
        self._check(self._L.phj_debug_poison_chunk_table(self._h, side, C.byref(params), byte))

    def debug_poison_alloc(self, byte: int = 0xFF) -> None:
        """Test hook (phj_debug_poison_alloc): every workspace buffer this
        context (and each of its members) allocates from now on is filled with
        `byte` (-1: off), so a read of a word nothing wrote shows."""
        self._check(self._L.phj_debug_poison_alloc(self._h, byte))

    def debug_preagg(self, mode: int = -1) -> tuple:
        """Test hook (phj_debug_preagg): set when phj_join pre-aggregates hot
        probe keys (PREAGG_AUTO / PREAGG_OFF / PREAGG_FORCED; -1 keeps the
        mode) and return the last join's (hot entries, pre-aggregated probe
        tuples), both 0 when it did not take that path."""
        stats = (C.c_uint64 * 2)()
        self._check(self._L.phj_debug_preagg(self._h, mode, stats))
        return int(stats[0]), int(stats[1])

    def debug_fail_member(self, member: int) -> None:
        """Test hook (phj_debug_fail_member): local member `member` fails the
        next join before the exchange (-1: none)."""
        self._check(self._L.phj_debug_fail_member(self._h, member))

    def debug_exchange_block(self, member: int, elems: int) -> np.ndarray:
        """Test hook (phj_debug_exchange_block): local member `member`'s packed
        exchange block of the last radix join (`elems` int64)."""
        out = np.zeros(elems, dtype=np.int64)
        self._check(self._L.phj_debug_exchange_block(self._h, member, out.ctypes.data_as(C.c_void_p), elems))
        return out

    def hash_keys(self, kind: int, seed: int, keys) -> np.ndarray:
        keys = np.ascontiguousarray(np.asarray(keys, dtype=np.int64))
        out = np.zeros(keys.shape[0], dtype=np.uint64)
        self._check(self._L.phj_hash_keys(self._h, kind, seed, keys.ctypes.data_as(C.c_void_p),
                                          keys.shape[0], out.ctypes.data_as(C.c_void_p)))
        return out


class Index:
    """A phj_index: a retained key index of one Context (Context.build_index).
    lookup() is enqueue-only on the context's stream; lookup_host() is the
    numpy convenience around it."""

    def __init__(self, ctx: Context, handle, result: JoinResult):
        self._ctx, self._h, self.result = ctx, handle, result

    def _handle(self):
        if not self._h or not self._ctx._h:
            raise PhjError(_capi.PHJ_ERR_STATE, "the index is closed")
        return self._h

    def info(self) -> IndexInfo:
        out = IndexInfo()
        rc = self._ctx._L.phj_index_info_get(self._handle(), C.byref(out))
        if rc != 0:
            raise PhjError(rc, "phj_index_info_get failed")
        return out

    def lookup(self, keys_ptr: int, n: int, rows_ptr: int, found_ptr: int | None = None,
               count_ptr: int | None = None, key_stride: int = 1) -> None:
        """phj_index_lookup on device pointers, enqueued on the context's stream
        (nothing is synchronised or read back): rows[i] = the lowest build row
        whose key equals keys[i * key_stride], or NO_ROW; found[i] (optional,
        one byte per key, any alignment) = 0 / 1; the number of found keys is
        added to the uint64 at count_ptr (optional; the caller zeroes it)."""
        c = self._ctx
        c._check(c._L.phj_index_lookup(c._h, self._handle(), C.c_void_p(keys_ptr or 0), key_stride, n,
                                       C.c_void_p(rows_ptr or 0), C.c_void_p(found_ptr or 0),
                                       C.c_void_p(count_ptr or 0)))

    def lookup_host(self, keys):
        """(rows, found) for a host array of int64 keys: uploads them, looks
        them up, synchronises and downloads. rows is int64 (NO_ROW where the
        key is absent), found a bool array."""
        keys = np.ascontiguousarray(keys, dtype=np.int64)
        assert keys.ndim == 1
        n = keys.shape[0]
        if n == 0:
            self._handle()
            return np.zeros(0, dtype=np.int64), np.zeros(0, dtype=bool)
        # device memory: a scratch context's columns (the C ABI has no allocator)
        with Context(self._ctx.device) as donor:
            donor.upload_columns(SIDE_PROBE, keys, np.zeros(n, dtype=np.int64))
            donor.upload_columns(SIDE_BUILD, np.zeros((n + 7) // 8, dtype=np.int64))
            kp, rp, _ = donor.columns_ptr(SIDE_PROBE)
            fp = donor.columns_ptr(SIDE_BUILD)[0]
            self.lookup(kp, n, rp, fp)
            self._ctx.synchronize()
            rows = np.ascontiguousarray(donor.download(SIDE_PROBE)[:, 1])
            found = np.ascontiguousarray(donor.download(SIDE_BUILD)[:, 0]).view(np.uint8)[:n].astype(bool)
        return rows, found

    @property
    def ordinals(self) -> bool:
        """Whether the index was built with ordinals (phj_index_flags_get)."""
        f = C.c_uint32(0)
        rc = self._ctx._L.phj_index_flags_get(self._handle(), C.byref(f))
        if rc != 0:
            raise PhjError(rc, "phj_index_flags_get failed")
        return bool(f.value & _capi.INDEX_ORDINALS)

    def first_rows_ptr(self) -> tuple:
        """phj_index_uniques: (device address, n) of first_rows, int64, n ==
        distinct, ascending: first_rows[j] is the first build row of the key
        with ordinal j. The index's memory; the address is 0 when n is 0."""
        c = self._ctx
        p, n = C.c_void_p(), C.c_uint64(0)
        c._check(c._L.phj_index_uniques(c._h, self._handle(), C.byref(p), C.byref(n)))
        return p.value or 0, n.value

    def first_rows(self) -> np.ndarray:
        """A host copy of first_rows: keys[first_rows()] are the distinct keys
        in ordinal order."""
        ptr, n = self.first_rows_ptr()
        if n == 0:
            return np.zeros(0, dtype=np.int64)
        c = self._ctx
        c.synchronize()
        with Context(c.device) as donor:   # a device-to-host copy through a borrowed key column
            donor.bind_columns(SIDE_PROBE, ptr, None, n)
            return np.ascontiguousarray(donor.download(SIDE_PROBE)[:, 0])

    def encode(self, keys_ptr: int, n: int, codes_ptr: int, found_ptr: int | None = None,
               count_ptr: int | None = None, key_stride: int = 1) -> None:
        """phj_index_encode on device pointers, enqueue-only like lookup():
        codes[i] = the ordinal of keys[i * key_stride], or NO_ROW."""
        c = self._ctx
        c._check(c._L.phj_index_encode(c._h, self._handle(), C.c_void_p(keys_ptr or 0), key_stride, n,
                                       C.c_void_p(codes_ptr or 0), C.c_void_p(found_ptr or 0),
                                       C.c_void_p(count_ptr or 0)))

    def accumulate(self, keys_ptr: int, n: int, counts_ptr: int, values_ptr: int | None = None,
                   sums_ptr: int | None = None, missing_ptr: int | None = None, key_stride: int = 1,
                   value_stride: int = 1) -> None:
        """phj_index_accumulate on device pointers, enqueue-only: counts[ordinal]
        += 1 and sums[ordinal] += values[i * value_stride] (modulo 2^64) for
        every key the index holds; absent keys are added to the uint64 at
        missing_ptr. The caller zeroes the accumulators (distinct entries)."""
        c = self._ctx
        c._check(c._L.phj_index_accumulate(c._h, self._handle(), C.c_void_p(keys_ptr or 0), key_stride,
                                           C.c_void_p(values_ptr or 0), value_stride, n, C.c_void_p(counts_ptr or 0),
                                           C.c_void_p(sums_ptr or 0), C.c_void_p(missing_ptr or 0)))

    def encode_host(self, keys):
        """(codes, found) for a host array of int64 keys (lookup_host's shape)."""
        keys = np.ascontiguousarray(keys, dtype=np.int64)
        assert keys.ndim == 1
        n = keys.shape[0]
        if n == 0:
            self.first_rows_ptr()   # (the state checks of an encode)
            return np.zeros(0, dtype=np.int64), np.zeros(0, dtype=bool)
        with Context(self._ctx.device) as donor:
            donor.upload_columns(SIDE_PROBE, keys, np.zeros(n, dtype=np.int64))
            donor.upload_columns(SIDE_BUILD, np.zeros((n + 7) // 8, dtype=np.int64))
            kp, cp, _ = donor.columns_ptr(SIDE_PROBE)
            fp = donor.columns_ptr(SIDE_BUILD)[0]
            self.encode(kp, n, cp, fp)
            self._ctx.synchronize()
            codes = np.ascontiguousarray(donor.download(SIDE_PROBE)[:, 1])
            found = np.ascontiguousarray(donor.download(SIDE_BUILD)[:, 0]).view(np.uint8)[:n].astype(bool)
        return codes, found

    def accumulate_host(self, keys, values=None):
        """(counts, sums, missing) of one batch of host keys (and int64
        values): counts uint64 and sums int64 with `distinct` entries, sums
        None without values, missing the number of keys the index lacks."""
        keys = np.ascontiguousarray(keys, dtype=np.int64)
        assert keys.ndim == 1
        n = keys.shape[0]
        d = self.first_rows_ptr()[1]
        if values is not None:
            values = np.ascontiguousarray(values, dtype=np.int64)
            assert values.shape == keys.shape
        counts = np.zeros(d, dtype=np.uint64)
        sums = np.zeros(d, dtype=np.int64) if values is not None else None
        if n == 0:
            return counts, sums, 0
        with Context(self._ctx.device) as donor:
            donor.upload_columns(SIDE_PROBE, keys, values)
            # the accumulators and the missing counter, zeroed: {counts | missing}, {sums}
            donor.upload_columns(SIDE_BUILD, np.zeros(d + 1, dtype=np.int64), np.zeros(d + 1, dtype=np.int64))
            kp, vp, _ = donor.columns_ptr(SIDE_PROBE)
            ap, sp, _ = donor.columns_ptr(SIDE_BUILD)
            self.accumulate(kp, n, ap, vp if values is not None else None, sp if values is not None else None, ap + 8 * d)
            self._ctx.synchronize()
            acc = donor.download(SIDE_BUILD)
        counts = np.ascontiguousarray(acc[:d, 0]).view(np.uint64)
        if values is not None:
            sums = np.ascontiguousarray(acc[:d, 1])
        return counts, sums, int(np.uint64(acc[d, 0]))

    def close(self):
        c = self._ctx
        if self._h and c._h:
            c._L.phj_index_destroy(c._h, self._h)
            if self in getattr(c, "_indexes", []):
                c._indexes.remove(self)
        self._h = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
