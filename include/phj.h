/*
 * phj.h — C ABI of the MI355X-native partitioned hash join (libphj_hip.so).
 *
 * This is the drop-in boundary under the reference's join API. The reference
 * (ragoragino/partitionedhashjoin, C++17, CPU only) exposes
 *
 *   RadixClustering::HashJoiner<HashTableFactory, HasherType>::Run(
 *       shared_ptr<Table<Tuple>> tableA /+build+/, shared_ptr<Table<Tuple>> tableB /+probe+/,
 *       shared_ptr<IHashJoinTimer> timer)                 src/RadixCluster/HashJoin.hpp:100-104
 *   NoPartitioning::HashJoiner<HashTableFactory>::Run(...) src/NoPartitioning/HashJoin.hpp:23-27
 *
 * and reads the relations through Table<Tuple>::operator[] / GetSize()
 * (src/Common/Table.hpp:42-46). Those entry points are kept in C++ by the
 * host driver (partitionedhashjoin_amd/host/Gpu/HashJoin.hpp); underneath, they call
 * only the functions below: plain pointers and sizes, no exceptions, no
 * torch types. Conventions: 0 = PHJ_OK, negative = error (message via
 * phj_last_error). A context owns every device buffer it allocates (grow
 * only, allocated outside the timed phases) and is not thread-safe. It spans
 * one device (one stream) or several (SURVEY.md §8(b),(e)): the relations
 * are range-sharded across the devices, phj_join runs the multi-GPU join
 * (partition the shards, RCCL all-gather of the partitioned build keys over
 * xGMI, local build + probe, all-reduce of the count) and one worker thread
 * per local device issues its work, as the reference's thread pool carries
 * its parallelism (src/main.cpp:235-241).
 */
#ifndef PHJ_H
#define PHJ_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PHJ_ABI_VERSION 2

/* Common::Tuple (src/Common/Table.hpp:20-25): alignas(16) {int64 id; int64 payload}. */
typedef struct phj_tuple {
    int64_t id;
    int64_t payload;
} phj_tuple;

typedef struct phj_ctx phj_ctx;

/* status codes */
#define PHJ_OK 0
#define PHJ_ERR_INVALID -1 /* bad argument (reference: std::invalid_argument) */
#define PHJ_ERR_NOMEM -2   /* device allocation failed */
#define PHJ_ERR_HIP -3     /* HIP runtime / kernel launch error */
#define PHJ_ERR_STATE -4   /* call order (e.g. join before relations are bound) */
#define PHJ_ERR_RANGE -5   /* size beyond a documented limit */

/* Common::JoinAlgorithmType values (src/Common/Configuration.hpp:12-15). */
#define PHJ_ALGO_NO_PARTITIONING 0
#define PHJ_ALGO_RADIX 1

/* hash functions: XXH3_64bits_withSeed over the 8-byte key (XXHasher.hpp:19-22)
 * and the Murmur3 fmix64 finalizer over key ^ seed (BASELINE config C2). */
#define PHJ_HASH_XXH3 0
#define PHJ_HASH_MURMUR3 1

/* relation sides: tableA = build (R), tableB = probe (S) (HashJoin.hpp:99) */
#define PHJ_SIDE_BUILD 0
#define PHJ_SIDE_PROBE 1

typedef struct phj_join_params {
    int32_t algo;            /* PHJ_ALGO_* */
    int32_t hash;            /* PHJ_HASH_* */
    uint64_t hash_seed;      /* XXHasher seed (random in the reference, explicit here) */
    /* Radix partition id q(key):
     *   num_partitions > 0 : q = hash % num_partitions  (reference `-p P`, HashJoin.hpp:349-351)
     *   num_partitions == 0: q = hash & (2^(b0+b1) - 1) (power-of-two radix, radix_bits = {b0, b1})
     * Partitioning takes one pass when q has <= 11 bits and two otherwise
     * (pass digits: high bits first). Maximum 22 bits (4,194,304 partitions). */
    uint32_t num_partitions;
    uint8_t radix_bits[2];
    uint8_t flags;           /* PHJ_PART_* */
    uint8_t reserved;
    /* NoPartitioning: hash-table slots per build tuple (>= 1). 0 selects the default. */
    double table_ratio;
} phj_join_params;

/* flags: PHJ_PART_STABLE asks phj_partition for the reference's exact layout
 * (a STABLE partition: partition-major, then input order, as partitionTable
 * writes it, RadixCluster/HashJoin.hpp:394-412). Without it a 2-pass
 * partition may order the tuples inside each partition arbitrarily (the
 * first pass then needs no histogram pass over the relation); partition
 * contents, bounds and every join count are identical either way. */
#define PHJ_PART_STABLE 0x1
/* flags: PHJ_TABLE_CHAINED (radix join) builds every partition's table as the
 * reference's SeparateChainingHashTable does (SeparateChaining.hpp:143-277:
 * buckets of slots, overflow chained on), in compacted form: per partition a
 * bucket-chained table in HBM whose buckets are contiguous runs (CSR offsets,
 * phj_join.h k_build_small / k_build_big), probed by k_probe. Without it the
 * counting join uses the open-addressed code tables of LinearProbing
 * semantics (phj_table.h). Counts are identical either way; the host driver's
 * SeparateChainingFactory sets it. Ignored by NoPartitioning. */
#define PHJ_TABLE_CHAINED 0x2
/* flags: PHJ_DEFER_TIMERS (one device) leaves this join's timers in the
 * context instead of reading them into the result: no event queries and no
 * extra synchronisation after the count is read back. Timers accumulate over
 * such joins; phj_timers_report returns their sums (the LDS join's build /
 * probe split then uses the last join's clocks) and resets them. Result
 * fields partition_ms .. total_ms and the timer list stay zero. A benchmark
 * loop sets it to keep the readout off its timed steps (bench.py). */
#define PHJ_DEFER_TIMERS 0x4
/* flags: PHJ_LEAN_TIMERS records only the timers of the large kernels (the
 * probe side's pass 1, the LDS join's build and probe, the exchange): every
 * event recorded between two kernels delays the second by ~4 us. The build
 * side's pass-1 timers are not recorded, the big clusters' tables
 * (`build.big`) are listed at zero. */
#define PHJ_LEAN_TIMERS 0x8
#define PHJ_MAX_TIMERS 32
#define PHJ_TIMER_NAME 24

typedef struct phj_join_result {
    uint64_t matches;            /* #probe tuples with >= 1 equal build key (semi-join count:
                                    the "Joined N tuples" of RadixCluster/HashJoin.hpp:320-321) */
    double partition_ms;         /* reference phase keys (Results.hpp:274-276), device time */
    double build_ms;
    double probe_ms;             /* probe alone (the reference's NoPartitioning probe also
                                    counts its build, Results.hpp:202; see phj host driver) */
    double total_ms;             /* first kernel start .. count on host */
    double exchange_ms;          /* multi-device: the build-side exchange (RCCL all-gather), 0 on one device */
    uint64_t algorithmic_bytes;  /* HBM bytes the algorithm must move */
    uint32_t num_partitions;     /* final partition count (radix) */
    uint32_t num_timers;
    double timer_ms[PHJ_MAX_TIMERS];        /* per-kernel device time (hipEvents on the ctx stream),
                                               summed over the records of that name */
    uint64_t timer_bytes[PHJ_MAX_TIMERS];   /* algorithmic bytes of those launches (summed) */
    char timer_name[PHJ_MAX_TIMERS][PHJ_TIMER_NAME];
} phj_join_result;

/* A partitioned relation on the device: SoA key/payload columns in partition
 * order, bounds[num_partitions + 1] offsets (uint32). Views are owned by the
 * ctx that produced them (valid until the next partition call on that side)
 * or by the caller (gathered shards on multi-GPU). */
typedef struct phj_partitioned {
    const int64_t *keys;
    const int64_t *payloads;
    const uint32_t *bounds;
    uint64_t n;
    uint32_t num_partitions;
    uint32_t reserved;
} phj_partitioned;

/* ---- context ---- */
/* One context over `ngpus` HIP devices (devs[i] = device of rank i; NULL means
 * 0 .. ngpus-1), SURVEY.md §8(b). ngpus == 1 gives a single-device context.
 * With ngpus > 1 every relation call takes the whole relation and range-shards
 * it (rank r holds rows [r*n/ngpus, (r+1)*n/ngpus)), and phj_join / phj_prepare
 * run the multi-GPU join with RCCL collectives (at most 16 ranks: ngpus, or
 * phj_ctx_create_rank's nranks, outside [1, 16] gives PHJ_ERR_INVALID and no
 * context). This is the reference's Run() with its thread pool
 * (src/main.cpp:235-241, dispatch :260-276) replaced by devices. */
int phj_ctx_create(int ngpus, const int *devs, phj_ctx **out);
/* flags for phj_ctx_create_ex */
#define PHJ_CTX_EXCHANGE 0x1 /* take the multi-GPU path even on one device (an RCCL world of one) */
#define PHJ_CTX_LOCAL 0x2    /* exchange by device copies between this process's members instead of
                                RCCL; devices may repeat (rehearses N ranks on one GPU) */
int phj_ctx_create_ex(int ngpus, const int *devs, uint32_t flags, phj_ctx **out);
/* A single-device context (ABI v1's phj_ctx_create(device)). */
int phj_ctx_create_device(int device, phj_ctx **out);
/* One device of a multi-process job (one process per GPU, e.g. torchrun):
 * rank 0 makes an id with phj_comm_unique_id and hands it to every rank (any
 * channel); each rank creates its context with it. On such a context every
 * call is collective (all ranks make the same calls in the same order), the
 * relation calls take this rank's shard (generators: rows [first_index,
 * first_index + n) of the global relation), and phj_join returns the global
 * count. */
#define PHJ_UNIQUE_ID_BYTES 128
int phj_comm_unique_id(uint8_t *id /* [PHJ_UNIQUE_ID_BYTES] */);
int phj_ctx_create_rank(int device, int nranks, int rank, const uint8_t *id, phj_ctx **out);
/* ranks of the job, global rank of this context's first device, devices in this context */
int phj_ctx_info(const phj_ctx *ctx, int *world, int *rank0, int *nlocal);
/* Host-only: rows [lo, hi) of an n-row relation held by `rank` of `world` ranks
 * (the range sharding of every multi-device context). */
void phj_shard_range(uint64_t n, int rank, int world, uint64_t *lo, uint64_t *hi);
/* ---- the multi-GPU exchange protocol (host-only; csrc/phj_group.h) ----
 * Replaces nothing in the reference (its parallel split is a thread pool,
 * src/main.cpp:235-241). These ARE the rules phj_join's member step applies,
 * exported so that a caller driving its own transport, and the CPU tests over
 * gloo, follow the same layout and reduction:
 *  - the exchange block of one rank (the all-gathered unit, int64 elements):
 *    its build codes in final partition order, then padding up to *codes_elems
 *    (a multiple of 64, >= the largest rank's shard; the padding's value is
 *    unspecified, no rank writes it and none reads it: a segment ends at its
 *    last bound), then the partition bounds (num_partitions + 1 uint32, two
 *    per element), *block_elems in all; a rank
 *    that failed before the all-gather still takes part with an all-zero
 *    block (bounds all 0: an empty build segment);
 *  - the count all-reduce (sum, uint64): every rank contributes the two words
 *    of phj_count_contribution; phj_count_verdict turns the sum into the global
 *    count, or PHJ_ERR_STATE when any rank failed. */
void phj_exchange_layout(uint64_t max_shard, uint32_t num_partitions, uint64_t *codes_elems,
                         uint64_t *block_elems);
/* The counting path phj_join takes on one device for params p over a build
 * side of build_n and a probe side of probe_n rows (default tuning; host
 * only, no device touched): PHJ_PATH_LDS_JOIN (the clusters' tables built in
 * LDS, phj_cluster.h), PHJ_PATH_CODE_TABLES (code tables in HBM, the probe
 * side's pass 2 on chip), PHJ_PATH_PARTITIONED (both sides fully partitioned,
 * fused or HBM-table join), PHJ_PATH_NO_PARTITIONING; negative: an error code.
 * The LDS join needs the probe side's keys-only chunked pass 1, whose chunk
 * pools address slots with 32 bits: above that bound it is declined. Replaces
 * the choice main() makes between the reference's joins (src/main.cpp:260-276),
 * refined inside RadixCluster by size. */
#define PHJ_PATH_NO_PARTITIONING 0
#define PHJ_PATH_LDS_JOIN 1
#define PHJ_PATH_CODE_TABLES 2
#define PHJ_PATH_PARTITIONED 3
int phj_join_path(const phj_join_params *p, uint64_t build_n, uint64_t probe_n);

/* The segment geometry phj_join's member step uses for radix params p and a
 * global build side of total_build rows (default tuning): the block's codes
 * are grouped by d(c) = (q(c) >> *shift), q = the plan's (sub-)partition
 * number of code c (q = c & (P - 1) for radix bits; (c % P) << s | bits
 * 40.. for h % P, s = *sub_bits; radix bits below the cluster width take
 * *sub_bits hash bits just above them), with *num_segments + 1 bounds.
 * *cluster = 1: the LDS join's clusters (phj_cluster.h), else the final
 * partitions of the code tables. PHJ_ERR_INVALID for bad params. */
int phj_exchange_geometry(const phj_join_params *p, uint64_t total_build, uint32_t *num_segments,
                          uint32_t *shift, uint32_t *sub_bits, uint32_t *sub_shift, int *cluster);
void phj_count_contribution(uint64_t count, int failed, uint64_t words[2]);
int phj_count_verdict(const uint64_t words[2], uint64_t *matches);
void phj_ctx_destroy(phj_ctx *ctx);
const char *phj_last_error(const phj_ctx *ctx);
/* Run on an external stream (e.g. torch.cuda.current_stream()); NULL = ctx-owned stream.
 * Multi-device contexts: only with one local device. The building blocks below
 * (phj_partition ... phj_hash_keys) likewise act on the single local device of a
 * rank context and return PHJ_ERR_STATE on a context with several local devices;
 * phj_join_materialize is single-device only. */
int phj_ctx_set_stream(phj_ctx *ctx, void *hip_stream);
int phj_ctx_synchronize(phj_ctx *ctx);
int phj_abi_version(void);

/* ---- relations (Table<Tuple>: &(*table)[0], GetSize(), Table.hpp:42-46) ---- */
/* Copy a host relation to ctx-owned device memory (H2D, synchronous). */
int phj_relation_upload(phj_ctx *ctx, int side, const phj_tuple *host, uint64_t n);
/* Borrow a device relation (caller keeps it alive while the ctx uses it). */
int phj_relation_bind_device(phj_ctx *ctx, int side, const phj_tuple *dev, uint64_t n);
/* Device pointer of the bound relation (NULL if none; NULL with *n = the rows
 * of all local devices on a context with several). */
const phj_tuple *phj_relation_device_ptr(phj_ctx *ctx, int side, uint64_t *n);
/* Copy the bound relation back to host (n tuples). */
int phj_relation_download(phj_ctx *ctx, int side, phj_tuple *host, uint64_t n);
/* On-device generators: Sequential::FillTable (Sequential.cpp:6-40)
 * and Zipf::FillTable (Zipf.cpp:58-108) over [lo, hi] with LCG streams seeded
 * per 4096-tuple batch. Rows [first_index, first_index + n) of the full
 * relation are generated (a range shard on multi-GPU; 0 = the whole table),
 * so shards concatenate to exactly the single-device relation. The Zipf
 * kernel draws with phj_pow.h, a restatement of glibc's pow (the one the
 * reference's std::pow calls) evaluated in glibc's FMA-build operation order,
 * so its samples equal the host generator's and the reference's bit for bit
 * (tests/test_gpu_generators.py). */
int phj_relation_generate_sequential(phj_ctx *ctx, int side, uint64_t n, int64_t start,
                                     uint64_t first_index);
int phj_relation_generate_zipf(phj_ctx *ctx, int side, uint64_t n, double alpha, int64_t lo,
                               int64_t hi, uint64_t seed, uint64_t first_index);
/* Count tuples of the bound relation with lo <= id <= hi (device reduction). */
int phj_relation_count_in_range(phj_ctx *ctx, int side, int64_t lo, int64_t hi, uint64_t *count);

/* ---- relations bound as columns ----
 * Replaces nothing in the reference, whose Table<Tuple> is an array of tuples.
 * A caller that keeps a relation as a key column and a payload column (torch
 * tensors, Arrow, a dataframe, this library's own partitioned views) binds the
 * two columns instead of interleaving them, and a caller that only wants the
 * count binds the key column alone.
 *  - Single-device contexts only: a group or rank context returns
 *    PHJ_ERR_STATE ("single-device contexts only") from all five calls.
 *  - Columns need 8-byte alignment and nothing more; the size limits are those
 *    of a tuple relation. Binding either layout on a side replaces the other.
 *  - phj_join's counting LDS join (PHJ_PATH_LDS_JOIN) in its default schedule
 *    reads the key column itself: 8 B per tuple in pass 1 instead of the 16-B
 *    tuple, no copy made, the payload column never touched.
 *  - phj_join_indices reads the key column of either side on every path and
 *    packs nothing (see "row-number joins" below).
 *  - Every other call (phj_join on its other paths, phj_join_materialize,
 *    phj_join_inner[_count], phj_join_rows[_count], phj_join_aggregate,
 *    phj_partition, phj_probe_pass1 off the native pass) packs the side once
 *    into a ctx-owned tuple buffer and runs on that copy as on a tuple
 *    relation. The copy stays until the side is rebound and DOUBLES that
 *    side's footprint (16 B per tuple beside the columns). The call that packs
 *    lists the timer `S.pack` / `R.pack` (32 B per tuple); later calls do not.
 *  - A key column alone packs with payload 0 for the calls that never look at
 *    payloads (phj_join, phj_join_inner_count, phj_join_rows_count). A call
 *    whose result holds payloads or sums of them (phj_join_materialize,
 *    phj_join_inner, phj_join_rows, phj_join_aggregate) returns PHJ_ERR_STATE
 *    ("payload column not bound") before any launch.
 *  - On a side bound as columns phj_relation_device_ptr returns NULL with *n =
 *    the rows, phj_relation_download writes tuples (payload 0 without a payload
 *    column), phj_relation_count_in_range counts over the key column. */
#define PHJ_LAYOUT_TUPLES  0
#define PHJ_LAYOUT_COLUMNS 1
typedef struct phj_relation_info {   /* 24 B */
    uint64_t n;
    uint32_t layout;        /* PHJ_LAYOUT_* of the bound relation */
    uint32_t has_payloads;  /* 0: a key column alone */
    uint32_t packed;        /* 1: the context holds a tuple copy it packed from the columns */
    uint32_t owned;         /* 1: the columns (or tuples) are context-owned memory */
} phj_relation_info;
/* Copy host columns to ctx-owned device memory (H2D, synchronous); payloads may be NULL. */
int phj_relation_upload_columns(phj_ctx *ctx, int side, const int64_t *keys, const int64_t *payloads,
                                uint64_t n);
/* Borrow device columns (the caller keeps them alive while the ctx uses them); dev_payloads may be NULL. */
int phj_relation_bind_columns(phj_ctx *ctx, int side, const int64_t *dev_keys, const int64_t *dev_payloads,
                              uint64_t n);
/* Split the bound tuple relation into ctx-owned columns on the device and make
 * them the bound relation (with_payloads == 0: the keys alone), e.g. after
 * phj_relation_generate_*. On a side already bound as columns it does nothing,
 * except that with_payloads == 0 drops the payload column. */
int phj_relation_to_columns(phj_ctx *ctx, int side, int with_payloads);
/* Device pointers of a columnar binding (*payloads NULL for a key column
 * alone); for a tuple binding both NULL. *n = the rows either way. */
int phj_relation_columns(phj_ctx *ctx, int side, const int64_t **keys, const int64_t **payloads, uint64_t *n);
int phj_relation_info_get(phj_ctx *ctx, int side, phj_relation_info *out);

/* ---- the join (HashJoiner::Run) ---- */
/* Synchronous: partition (radix) / build / probe on the device, count back on the host. */
int phj_join(phj_ctx *ctx, const phj_join_params *p, phj_join_result *r);

/* Allocate (grow-only) every workspace buffer phj_join with these params needs
 * for the relations currently bound, launching nothing: the reference keeps
 * its allocations outside the timed phases (RadixCluster/HashJoin.hpp:195-198),
 * and a first phj_join after phj_prepare allocates nothing. Optional. */
int phj_prepare(phj_ctx *ctx, const phj_join_params *p);

/* ---- materialised join ---- */
/* Common::JoinedTuple (src/Common/Table.hpp:27-33): {id, payloadA, payloadB}, 24 B. */
typedef struct phj_joined {
    int64_t id;
    int64_t payload_a; /* build (tableA) payload of the first match: HashTable::Get (LinearProbing.hpp:160-180) */
    int64_t payload_b; /* probe (tableB) payload */
} phj_joined;
/* The join of phj_join (same params, same count), materialised: one row per
 * probe tuple with a match, into a ctx-owned device buffer. This is the
 * Table<JoinedTuple> the reference's Run() declares but returns empty
 * (NoPartitioning/HashJoin.hpp:186, RadixCluster/HashJoin.hpp:240). Rows are
 * in the probe side's storage order (input order for NoPartitioning,
 * partition order for the radix join). The radix form needs one build
 * segment. Synchronous; r->matches = number of rows. */
int phj_join_materialize(phj_ctx *ctx, const phj_join_params *p, phj_join_result *r);
/* ---- inner join with duplicate build keys ----
 * Replaces nothing in the reference, whose Get() stops at the first hit:
 * phj_join and phj_join_materialize answer the semi-join question (one count /
 * one row per probe tuple that has a match). These two compute R ⋈ S itself.
 *
 * phj_join_inner_count: r->matches = |R ⋈ S|, the number of (build tuple,
 * probe tuple) pairs with equal ids, exact in 64 bits; no rows. No size limit
 * beyond those of phj_join (each side below 2^32 tuples). The rows of an
 * earlier materialised join stay as they are.
 *
 * phj_join_inner: the same join, materialised: one phj_joined row {id, that
 * build tuple's payload, the probe tuple's payload} per pair, into the
 * ctx-owned row buffer that phj_joined_rows / phj_joined_download serve;
 * r->matches = number of rows. A later phj_join_materialize replaces the rows,
 * and the reverse holds too.
 *  - PHJ_ALGO_RADIX and PHJ_ALGO_NO_PARTITIONING are both supported; the radix
 *    form has phj_join_materialize's precondition (the fused LDS join: one
 *    build segment, partitions of ~170 build tuples on average, which the
 *    default sub-partitioning provides).
 *  - Single-device contexts only: a group or rank context returns
 *    PHJ_ERR_STATE ("single-device contexts only").
 *  - Rows are grouped by probe tuple: all rows of one probe tuple are
 *    contiguous, and the groups come in the probe side's storage order (input
 *    order for NoPartitioning, partition order for the radix join). The order
 *    of the build matches inside a group is unspecified.
 *  - Rows are addressed with 32 bits. With 2^32 pairs or more phj_join_inner
 *    returns PHJ_ERR_RANGE before any row is written or the row buffer is
 *    grown; r->matches still holds the 64-bit pair count, and phj_joined_rows
 *    then reports 0 rows.
 *  - An empty build or probe side gives 0 pairs and no error.
 *  - Two passes over the same join (count, then emit at scanned offsets):
 *    timers `inner.count` and `inner.emit` beside the partition / build timers;
 *    algorithmic_bytes counts what both passes must move (DESIGN.md §Inner join).
 * Synchronous. */
int phj_join_inner_count(phj_ctx *ctx, const phj_join_params *p, phj_join_result *r);
int phj_join_inner(phj_ctx *ctx, const phj_join_params *p, phj_join_result *r);

/* ---- outer and anti joins: rows for tuples without a partner ----
 * Replaces nothing in the reference. Rows fall into three classes, and a join
 * kind is a set of classes: */
#define PHJ_ROWS_PAIRS      0x1  /* {id, payload_a, payload_b} per (build tuple, probe tuple) pair: phj_join_inner's rows */
#define PHJ_ROWS_PROBE_ONLY 0x2  /* {id, null_payload, payload_b} per probe tuple with no equal build key */
#define PHJ_ROWS_BUILD_ONLY 0x4  /* {id, payload_a, null_payload} per build tuple with no equal probe key */
/*   classes 1: inner              3: probe-preserving outer   5: build-preserving outer
 *           7: full outer         2: probe anti               4: build anti
 *           6: both anti sides
 * classes == 0 or any bit above 0x4 gives PHJ_ERR_INVALID. */
typedef struct phj_row_counts {
    uint64_t pairs;       /* always filled: phj_join_inner_count's matches, 64-bit exact */
    uint64_t probe_only;  /* filled when PHJ_ROWS_PROBE_ONLY is asked, else 0 */
    uint64_t build_only;  /* filled when PHJ_ROWS_BUILD_ONLY is asked, else 0 */
    uint64_t rows;        /* the sum of the classes asked for == r->matches */
} phj_row_counts;
/* phj_join_rows_count fills r and n and writes no rows (the rows of an earlier
 * materialised join stay as they are); phj_join_rows also materialises the
 * rows into the ctx-owned row buffer that phj_joined_rows / phj_joined_download
 * serve.
 *  - Row layout. First the probe part: the rows of classes 0x1 and 0x2,
 *    grouped by probe tuple, the groups in the probe side's storage order
 *    (input order for NoPartitioning, partition order for the radix join),
 *    exactly as phj_join_inner orders them. A probe tuple without a partner
 *    contributes its one null row at its place in that order (class 0x2) or
 *    nothing. The build_only rows follow the probe part, in unspecified order.
 *    The order inside a group is unspecified.
 *  - null_payload is the caller's marker for the missing side; the library
 *    does not interpret it.
 *  - Rows are addressed with 32 bits. With n->rows >= 2^32 phj_join_rows
 *    returns PHJ_ERR_RANGE before any row is written or the row buffer is
 *    grown; the counts are still filled, and phj_joined_rows then reports 0
 *    rows.
 *  - An empty side is not an error: every tuple of the other side is then
 *    "only", its rows are copied from the bound relation in input order and
 *    no join runs. Both sides empty gives 0 rows.
 *  - Single-device contexts only: a group or rank context returns
 *    PHJ_ERR_STATE ("single-device contexts only").
 *  - PHJ_ALGO_RADIX and PHJ_ALGO_NO_PARTITIONING; the radix form has
 *    phj_join_inner's precondition.
 *  - A later phj_join_materialize or phj_join_inner replaces the rows, and the
 *    reverse.
 *  - Timers beside the partition / np.build timers: `rows.count` (the join,
 *    marking the build tuples it hits when class 0x4 is asked, plus the
 *    reduction of the per-probe pair counts), `rows.emit` (offsets, pair rows,
 *    null rows), `rows.build_only` (count and compaction of the unhit build
 *    tuples). algorithmic_bytes counts what each pass must move (DESIGN.md
 *    §Outer and anti joins).
 * Synchronous. */
int phj_join_rows_count(phj_ctx *ctx, const phj_join_params *p, uint32_t classes,
                        phj_join_result *r, phj_row_counts *n);
int phj_join_rows(phj_ctx *ctx, const phj_join_params *p, uint32_t classes, int64_t null_payload,
                  phj_join_result *r, phj_row_counts *n);
/* The rows of the last phj_join_materialize / phj_join_inner / phj_join_rows:
 * device pointer (ctx-owned, valid until the next materialised join) and count. */
const phj_joined *phj_joined_rows(phj_ctx *ctx, uint64_t *n);
/* Copy the first n rows of the last phj_join_materialize / phj_join_inner / phj_join_rows to host memory. */
int phj_joined_download(phj_ctx *ctx, phj_joined *host, uint64_t n);

/* ---- row-number joins: index pairs from key columns, and a gather ----
 * Replaces nothing in the reference, whose relations have one payload. A
 * caller with many columns per relation wants the gather map of a join: which
 * build row goes with which probe row. phj_join_indices is phj_join_rows
 * returning that map as two int64 index columns, and it reads nothing but
 * keys; the caller then gathers any number of columns with the map (torch's
 * index_select takes the columns as they are, or phj_gather_column).
 *  - One row (build_rows[k], probe_rows[k]) per row that phj_join_rows would
 *    write for the same classes. Row numbers are positions in the relation as
 *    bound, 0-based.
 *  - Row order is phj_join_rows' contract: the probe part first, grouped by
 *    probe tuple in the probe side's storage order; a probe tuple without a
 *    partner sits at its place with build_rows == PHJ_NO_ROW; the build-only
 *    rows follow in unspecified order with probe_rows == PHJ_NO_ROW. On
 *    NoPartitioning storage order is input order, so probe_rows of the probe
 *    part is non-decreasing.
 *  - Every binding works and only keys are read: of a side bound as columns
 *    the key column (the payload column is never touched, and a key column
 *    alone is enough), of a side bound as tuples the ids (8 B at stride 16).
 *    Nothing is packed: phj_relation_info.packed stays as it was and no
 *    `*.pack` timer appears. Pass 1 (and the NoPartitioning probe) take each
 *    tuple's position as the payload they move.
 *  - phj_join_rows' rules carry over: PHJ_ALGO_RADIX with its precondition and
 *    PHJ_ALGO_NO_PARTITIONING; single-device contexts only (PHJ_ERR_STATE,
 *    "single-device contexts only"); classes == 0 or a bit above 0x4 gives
 *    PHJ_ERR_INVALID; with 2^32 rows or more PHJ_ERR_RANGE before anything is
 *    written or grown, the counts still filled and 0 index rows reported; an
 *    empty side is not an error (the other side's tuples are "only", with
 *    indices 0 .. n-1, no join runs; both sides empty: 0 rows).
 *  - One result at a time, and the two kinds may share memory: an index join
 *    replaces the rows of an earlier materialised join (phj_joined_rows then
 *    reports 0), and phj_join_materialize, phj_join_inner and phj_join_rows
 *    replace the index columns (phj_joined_indices then reports 0).
 *    phj_join_rows_count, phj_join_inner_count and phj_join_aggregate disturb
 *    neither.
 *  - Timers are phj_join_rows' (`rows.count`, `rows.emit`, `rows.build_only`)
 *    beside the partition / np.build timers. Bytes: 16 per row written where
 *    phj_join_rows writes 24; a side whose pass 1 reads a key column is
 *    accounted 8 B read per tuple where the tuple form reads 16 (`X.p1.hist`
 *    n * 8, `X.p1.scatter` n * 24; the chunked pass n * 24);
 *    algorithmic_bytes follows (DESIGN.md §3 "Row-number joins").
 * Synchronous. */
#define PHJ_NO_ROW (-1)   /* the missing side's row number in an outer / anti join */
int phj_join_indices(phj_ctx *ctx, const phj_join_params *p, uint32_t classes,
                     phj_join_result *r, phj_row_counts *n);
/* Device pointers of the last index join's columns (ctx-owned, valid until the
 * next materialised or index join; NULL when there are no rows) and the row count. */
int phj_joined_indices(phj_ctx *ctx, const int64_t **build_rows, const int64_t **probe_rows, uint64_t *n);
/* Copy the first n entries of either column (NULL: skip it) to host OR device memory. */
int phj_joined_indices_download(phj_ctx *ctx, int64_t *build_rows, int64_t *probe_rows, uint64_t n);
/* out[i] = src[idx[i]] for i in [0, n); idx[i] == PHJ_NO_ROW gives *null_value,
 * or leaves out[i] as it is when null_value is NULL (so two gathers compose a
 * coalesce). All pointers but null_value are device addresses, 8-byte aligned.
 *  - Synchronous, on the context's stream; n == 0 is PHJ_OK.
 *  - An index outside [0, src_n) other than PHJ_NO_ROW is never dereferenced:
 *    its out[i] gets the null treatment and the call returns PHJ_ERR_RANGE
 *    after the kernel, the message saying how many there were.
 *  - Single-device contexts only: a group or rank context returns PHJ_ERR_STATE. */
int phj_gather_column(phj_ctx *ctx, const int64_t *src, uint64_t src_n, const int64_t *idx, uint64_t n,
                      const int64_t *null_value, int64_t *out);

/* ---- aggregates over the join, without its rows ----
 * Replaces nothing in the reference, which only counts. What a caller usually
 * wants of R ⋈ S is an aggregate: Σ payload over the pairs, or, per build
 * tuple, its number of probe partners and the sum of their payloads (dimension
 * ⋈ fact, GROUP BY dimension). One accumulating pass over the join the inner
 * join's count pass does; nothing is stored or addressed per pair. */
#define PHJ_AGG_GROUPS        0x1  /* also produce one phj_group_row per build tuple */
#define PHJ_AGG_MATCHED_ONLY  0x2  /* with GROUPS: drop build tuples with no partner */
typedef struct phj_join_totals {   /* 40 B; every sum is modulo 2^64 (two's complement wrap) */
    uint64_t pairs;          /* |R ⋈ S| == the matches of the inner join's count */
    uint64_t probe_matched;  /* probe tuples with >= 1 partner == the matches of the counting join */
    int64_t  sum_a;          /* Σ over pairs of the build payload */
    int64_t  sum_b;          /* Σ over pairs of the probe payload */
    int64_t  sum_ab;         /* Σ over pairs of build payload * probe payload */
} phj_join_totals;
typedef struct phj_group_row {     /* 32 B */
    int64_t id;
    int64_t payload_a;             /* the build tuple */
    uint64_t partners;             /* probe tuples with its id */
    int64_t sum_b;                 /* Σ of their payloads, modulo 2^64 */
} phj_group_row;
/* The totals of R ⋈ S into *t and, with PHJ_AGG_GROUPS, the group rows.
 *  - Synchronous; r->matches == t->pairs.
 *  - PHJ_ALGO_RADIX (with the inner join's precondition: the fused LDS join)
 *    and PHJ_ALGO_NO_PARTITIONING.
 *  - Single-device contexts only: a group or rank context returns
 *    PHJ_ERR_STATE ("single-device contexts only").
 *  - flags with a bit above 0x2, or MATCHED_ONLY without GROUPS, give
 *    PHJ_ERR_INVALID.
 *  - No limit at 2^32 pairs: all five totals stay exact (the sums modulo 2^64)
 *    whatever the pair count. The sides' own limits are those of the inner
 *    join's count.
 *  - Group rows live in a ctx-owned buffer of their own, valid until the next
 *    aggregate join. The rows of an earlier materialised join stay untouched,
 *    and a later materialised join does not disturb the group rows. One row
 *    per build tuple, in unspecified order: |R| rows, or only those with
 *    partners > 0 under MATCHED_ONLY. Without GROUPS the group rows are 0
 *    after the call.
 *  - An empty side is not an error: the totals are all zero. With GROUPS and
 *    an empty probe side every build tuple gets a {id, payload_a, 0, 0} row
 *    copied from the bound relation (none under MATCHED_ONLY); no join runs.
 *  - Timers beside the partition / np.build timers: `agg.join` (the
 *    accumulating pass) and, with GROUPS, `agg.groups` (the clear of the
 *    accumulators and the compaction). algorithmic_bytes counts what each
 *    pass must move (DESIGN.md §Aggregate joins). */
int phj_join_aggregate(phj_ctx *ctx, const phj_join_params *p, uint32_t flags, phj_join_result *r,
                       phj_join_totals *t);
/* The group rows of the last aggregate join: device pointer (ctx-owned, valid
 * until the next one) and count. */
const phj_group_row *phj_group_rows(phj_ctx *ctx, uint64_t *n);
/* Copy the first n group rows of the last aggregate join to host memory. */
int phj_group_download(phj_ctx *ctx, phj_group_row *host, uint64_t n);

/* ---- membership (semi / anti join) as masks in the caller's row order ----
 * Replaces nothing in the reference, which counts the probe tuples with a
 * partner but does not say which they are. phj_join_member answers "which of
 * my rows have a partner on the other side?" (SQL's IN / EXISTS, torch.isin):
 * one byte per row, row i at byte i, so `cols[mask]` is the semi join and
 * `cols[~mask]` the anti join of any number of columns.
 *  - Masks. Each mask is a caller's DEVICE buffer of one byte per row of the
 *    relation as bound (probe_mask: probe side, build_mask: build side), the
 *    byte layout of a torch.bool tensor. Every byte in [0, n) is written as 0
 *    or 1 and no byte outside that range is touched. The pointers need no
 *    alignment: a slice of a tensor at an odd offset is valid.
 *  - sides is a set of PHJ_MEMBER_PROBE / PHJ_MEMBER_BUILD. A mask whose side
 *    is not asked may be NULL and is not touched; a side asked with a NULL
 *    mask gives PHJ_ERR_INVALID unless that relation has 0 rows; sides == 0 or
 *    a bit above 0x2 gives PHJ_ERR_INVALID.
 *  - Synchronous, on the context's stream. r->matches == n->probe_matched ==
 *    phj_join's matches for the same relations; n->build_matched is filled
 *    when PHJ_MEMBER_BUILD is asked, else 0.
 *  - Keys only, nothing packed: of a side bound as columns the key column is
 *    read (the payload column is never touched, and a key column alone is
 *    enough), of a side bound as tuples the ids (8 B at stride 16).
 *    phj_relation_info.packed stays as it was and no `*.pack` timer appears.
 *  - One schedule, whatever p asks for. p must pass the usual validation (a
 *    known algo and hash; radix_bits / num_partitions in range for
 *    PHJ_ALGO_RADIX) and p->hash / p->hash_seed are used, but algo, the radix
 *    bits, num_partitions and table_ratio do not change what runs: R is
 *    partitioned into region code tables (the NoPartitioning count's build)
 *    and S is probed unpartitioned, in input order, so the answer for row i
 *    comes out at lane i and the mask is a coalesced write. With
 *    PHJ_MEMBER_BUILD every probe hit also marks the table slot it matched,
 *    and a second pass over R in input order reads its key's mark.
 *  - Single-device contexts only: a group or rank context returns
 *    PHJ_ERR_STATE ("single-device contexts only").
 *  - An empty side is not an error (unlike NoPartitioning's phj_join): the
 *    other side's mask is all 0, the counts are 0, no join runs. The build
 *    side is limited to 2^30 - 1 rows (PHJ_ERR_RANGE above).
 *  - Nothing else is disturbed: the rows and index columns of earlier
 *    materialised or index joins and the group rows stay as they are, and a
 *    phj_join on the same context afterwards is exact (the code-table
 *    workspace is shared, the marks are a buffer of their own that the call
 *    clears before each join that asks for the build side).
 *  - Timers: `R.p1.*` / `R.p2.scatter` and `np.build` as phj_join's
 *    NoPartitioning count reports them (a key column is accounted 8 B per row
 *    read where tuples are 16), `member.probe` (S's keys read, 8 B or 16 B per
 *    row, the tables, the mask written) and, with PHJ_MEMBER_BUILD,
 *    `member.build` (R's keys read again, a bucket and a mark per row, the
 *    mask written). algorithmic_bytes follows these (DESIGN.md §3 "Membership
 *    joins"). phj_prepare is not extended: the call grows what it needs
 *    before its first launch. */
#define PHJ_MEMBER_PROBE 0x1   /* probe_mask[i] = 1 iff probe row i's key equals some build key */
#define PHJ_MEMBER_BUILD 0x2   /* build_mask[i] = 1 iff build row i's key equals some probe key */
typedef struct phj_member_counts {   /* 16 B */
    uint64_t probe_matched;   /* always filled == phj_join's matches for the same relations */
    uint64_t build_matched;   /* filled when PHJ_MEMBER_BUILD is asked, else 0 */
} phj_member_counts;
int phj_join_member(phj_ctx *ctx, const phj_join_params *p, uint32_t sides,
                    uint8_t *probe_mask, uint8_t *build_mask,
                    phj_join_result *r, phj_member_counts *n);

/* ---- a retained key index: build once, look up key batches in-stream ----
 * Replaces nothing in the reference, whose tables live for one Run(). Every
 * join above takes both relations and rebuilds R's tables per call; a caller
 * with one dimension or dictionary table and a stream of key batches wants
 * "key -> row of the table" per batch, on its own stream, with nothing coming
 * back to the host (pandas.Index.get_indexer, an embedding-id lookup, a
 * foreign-key resolve). phj_index_build makes the table once and keeps it;
 * phj_index_lookup is one kernel launch.
 *
 * phj_index_build indexes the build side as bound (tuples, columns, or a key
 * column alone). It reads keys only and packs nothing: phj_relation_info.packed
 * stays as it was and no `*.pack` timer appears.
 *  - Entries: each distinct key once, with the lowest build row that carries
 *    it (its first occurrence). A key repeated a million times is one entry
 *    and lengthens no lookup's walk.
 *  - Synchronous; fills r: r->matches = the distinct key count; timers
 *    `R.p1.*` / `R.p2.scatter` as the NoPartitioning joins report them and
 *    `index.build` (the partitioned keys and rows read, 16 B per row, and every
 *    bucket written); algorithmic_bytes is the sum of the timers' bytes.
 *  - p passes the usual validation; p->hash, p->hash_seed and p->table_ratio
 *    (slots per build row, >= 1; 0 selects the default 2.0) are used; algo and
 *    the radix fields do not change what runs (phj_join_member's rule).
 *  - Geometry (phj_index_info) depends on the row count and table_ratio alone:
 *    nb buckets of `slots` = 5 entries in 2^rbits regions of nbr buckets,
 *    1 <= rbits <= 22. A key's region is the low rbits of its hash code, its
 *    home bucket inside the region (high word of the code * nbr) >> 32; the
 *    walk goes bucket by bucket over the whole table and wraps at its end. A
 *    bucket is one 64-byte line holding five codes, their five rows and a fill
 *    count, so a lookup that settles at home reads one line. Liveness is the
 *    fill count: no key value is reserved (0, -1, INT64_MIN, INT64_MAX are
 *    keys like any other).
 *  - The index owns its memory (phj_index_info.table_bytes) and stays valid
 *    until phj_index_destroy or phj_ctx_destroy, which frees survivors. No
 *    later join on the context, no rebinding of either side and no freeing of
 *    a borrowed key column disturbs it. Several indexes may coexist.
 *  - An empty build side gives a valid index over which every lookup misses.
 *    The build side is limited to 2^30 - 1 rows (PHJ_ERR_RANGE above, before
 *    any launch). Single-device contexts only: a group or rank context returns
 *    PHJ_ERR_STATE ("single-device contexts only").
 *
 * phj_index_lookup enqueues one kernel on the context's stream
 * (phj_ctx_set_stream, or the context's own) and returns at once: it does not
 * synchronise, read anything back, record events or timers, or allocate.
 *  - dev_keys: any device address, 8-byte aligned, not a bound relation; key i
 *    is dev_keys[i * key_stride], key_stride 1 (a key column) or 2 (the ids of
 *    a tuple array); anything else gives PHJ_ERR_INVALID.
 *  - out_rows[i] = the lowest build row whose key equals key i, or PHJ_NO_ROW:
 *    an index column for phj_gather_column or torch's index_select. 8-byte
 *    aligned, required unless n == 0.
 *  - out_found (optional): one byte per key, 0 or 1, at any alignment (a
 *    torch.bool tensor or an odd-offset slice of one).
 *  - dev_found_count (optional, 8-byte aligned): a device counter to which the
 *    number of found keys is added; the caller zeroes it.
 *  - Exactly [0, n) of each output is written. n == 0 is PHJ_OK and launches
 *    nothing.
 *  - The index must belong to ctx. Lookups of one context run in stream order;
 *    phj_ctx_synchronize (or the caller's own stream) waits for them. */
typedef struct phj_index phj_index;
typedef struct phj_index_info {   /* 40 B */
    uint64_t rows;        /* build rows indexed */
    uint64_t distinct;    /* distinct keys among them == entries of the table */
    uint64_t table_bytes; /* device memory the index holds */
    uint32_t nb, nbr, rbits, slots;  /* geometry: buckets, buckets per region, region bits, key slots per bucket */
} phj_index_info;
int phj_index_build(phj_ctx *ctx, const phj_join_params *p, phj_index **out, phj_join_result *r);
int phj_index_info_get(const phj_index *index, phj_index_info *out);
int phj_index_lookup(phj_ctx *ctx, const phj_index *index, const int64_t *dev_keys, uint32_t key_stride, uint64_t n,
                     int64_t *out_rows, uint8_t *out_found, unsigned long long *dev_found_count);
/* Frees the index (after the lookups already in the stream). An index that
 * ctx does not hold (destroyed before, or another context's) is ignored. */
void phj_index_destroy(phj_ctx *ctx, phj_index *index);

/* ---- ordinals on the key index: a dense id per distinct key ----
 * phj_index_build_ex(flags = PHJ_INDEX_ORDINALS) builds the index above and
 * gives every distinct key its ordinal: the number of distinct build keys whose
 * first row is lower than this key's first row. That is first-appearance
 * order, 0 .. distinct-1: pandas.factorize of the build key column, or the
 * inverse of torch.unique in the order keys first appear. flags == 0 is
 * phj_index_build exactly; any other bit gives PHJ_ERR_INVALID. The ordinal
 * build adds one timer, `index.ordinals`, and its rules are phj_index_build's
 * (single-device contexts, fewer than 2^30 build rows, an empty build side
 * gives a valid index with distinct == 0).
 *
 *  - phj_index_uniques: *dev_first_rows (int64, the index's own device memory,
 *    *n == distinct entries, strictly ascending, valid as long as the index) is
 *    the first row of the key with ordinal j: uniques =
 *    keys.index_select(0, first_rows), and uniques[encode(keys)] == keys.
 *    phj_index_info.table_bytes counts the array.
 *  - phj_index_encode has phj_index_lookup's contract word for word (enqueue
 *    only on the context's stream; no synchronise, event, allocation or copy
 *    back; key_stride 1 or 2; 8-byte aligned pointers, out_found at any
 *    alignment; exactly [0, n) of each output written; n == 0 launches
 *    nothing) and writes out_codes[i] = the key's ordinal, or PHJ_NO_ROW for a
 *    key the index does not hold. The bucket holds the ordinal, so a key that
 *    settles at home reads one 64-byte line. dev_keys may be the column the
 *    index was built from (it is only read): that is factorize.
 *  - phj_index_lookup on an ordinal index returns rows as on a plain one, at
 *    the price of one dependent read of first_rows per found key.
 *  - phj_index_accumulate, enqueue-only like encode: for every key the index
 *    holds, dev_counts[ordinal] += 1 and, when dev_values and dev_sums are
 *    given (both or neither, else PHJ_ERR_INVALID), dev_sums[ordinal] +=
 *    dev_values[i * value_stride] modulo 2^64 (value_stride 1 or 2), so the
 *    result does not depend on the order of arrival. Absent keys are skipped
 *    and added to *dev_missing_count (optional). The caller owns and zeroes
 *    the accumulators (distinct entries each, 8-byte aligned); successive
 *    batches add up. dev_counts is required unless n == 0. Nothing else is
 *    written.
 *  - On an index built without the flag, uniques, encode and accumulate return
 *    PHJ_ERR_STATE ("index built without ordinals") and launch nothing. The
 *    index must belong to ctx. */
#define PHJ_INDEX_ORDINALS 0x1
int phj_index_build_ex(phj_ctx *ctx, const phj_join_params *p, uint32_t flags, phj_index **out, phj_join_result *r);
int phj_index_flags_get(const phj_index *index, uint32_t *flags);
int phj_index_uniques(phj_ctx *ctx, const phj_index *index, const int64_t **dev_first_rows, uint64_t *n);
int phj_index_encode(phj_ctx *ctx, const phj_index *index, const int64_t *dev_keys, uint32_t key_stride, uint64_t n,
                     int64_t *out_codes, uint8_t *out_found, unsigned long long *dev_found_count);
int phj_index_accumulate(phj_ctx *ctx, const phj_index *index, const int64_t *dev_keys, uint32_t key_stride,
                         const int64_t *dev_values, uint32_t value_stride, uint64_t n, unsigned long long *dev_counts,
                         int64_t *dev_sums, unsigned long long *dev_missing_count);

/* ---- building blocks (multi-GPU: range-sharded relations, RCCL exchange) ---- */
/* Radix-partition the bound relation of `side`; fills `out` with ctx-owned views.
 * Asynchronous on the ctx stream (order later work on the same stream). */
int phj_partition(phj_ctx *ctx, int side, const phj_join_params *p, phj_partitioned *out);
/* Build bucket-chained tables over the union of `nbuild` partitioned build
 * segments (e.g. every rank's shard after an all-gather) and probe the ctx's
 * partitioned probe relation. Build segments may omit payloads (NULL in every
 * segment): the join only tests key equality, as the reference's Join() only
 * tests Get() for null (RadixCluster/HashJoin.hpp:295-301). Probe the ctx's
 * partitioned probe relation (phj_partition(PHJ_SIDE_PROBE) with the same
 * params must precede). Synchronous; fills r (build_ms, probe_ms, matches). */
int phj_join_partitioned(phj_ctx *ctx, const phj_join_params *p, int nbuild,
                         const phj_partitioned *build, phj_join_result *r);
/* Asynchronous form of phj_join_partitioned for stream-ordered pipelines
 * (multi-GPU: the count feeds an RCCL all-reduce on the same stream): enqueues
 * build and probe on the ctx stream and stores the count (uint64) at
 * `dev_count`, a device address; no host synchronization. The phase timers
 * are read later with phj_timers_report. */
int phj_join_partitioned_async(phj_ctx *ctx, const phj_join_params *p, int nbuild,
                               const phj_partitioned *build, uint64_t *dev_count);
/* Per-kernel device timers recorded since the last report (e.g. after
 * phj_partition / phj_join_partitioned_async calls, possibly several joins),
 * summed by timer name; synchronizes the ctx stream, then resets. */
int phj_timers_report(phj_ctx *ctx, phj_join_result *r);
/* Copy a partitioned view (keys, payloads: n; bounds: P+1) to host or device
 * buffers (any may be NULL). Synchronous when any destination is host memory;
 * with device destinations only, the copies are enqueued on the ctx stream
 * and the call returns at once. */
int phj_partitioned_download(phj_ctx *ctx, const phj_partitioned *v, int64_t *keys,
                             int64_t *payloads, uint32_t *bounds);

/* ---- hashing on the device (tests / host parity) ---- */
/* out[i] = hash(keys[i]) for n host keys, evaluated by the device kernel. */
int phj_hash_keys(phj_ctx *ctx, int hash, uint64_t seed, const int64_t *keys, uint64_t n,
                  uint64_t *out);

/* ---- test hook: the probe side's pass 1 of the counting join ----
 * Replaces nothing in the reference: it exposes the intermediate that
 * phj_join's on-chip probe consumes instead of the reference's partitioned
 * probe table (src/RadixCluster/HashJoin.hpp:394-412, first of two passes),
 * so tests can compare it with the oracle at full size. Runs the probe side's
 * pass 1 for params (single-device ctx, radix join taking the on-chip path)
 * and copies its output, concatenated in pass-2 tile order (pass-1 digit
 * major, unordered inside a digit), to keys[0, n) (n = |S|), and the digit
 * bounds to bounds1[0, nb1 + 1). *nb1 = pass-1 digits; *codes = 1 when the
 * output holds hash codes h(key) (the keys-only pass), 0 for keys. bounds1
 * must hold at least 2049 entries. */
int phj_probe_pass1(phj_ctx *ctx, const phj_join_params *p, int64_t *keys, uint64_t n, uint32_t *bounds1,
                    uint32_t *nb1, int *codes);

/* ---- test hook: a stale chunk table ----
 * Replaces nothing in the reference. Fills the chunk table of `side`'s chunked
 * pass 1 (the one the last chunked pass on that side used; if there is none
 * yet, the one phj_join with params p would use) with `byte` and marks it
 * clean, as a table left stale by an earlier pass would be. The chunked passes bound-check every
 * chunk id and chain index they read back, so the next join returns
 * PHJ_ERR_STATE (nothing is written through a stale entry) and clears the
 * table; the join after it is exact again. Single-device ctx. */
int phj_debug_poison_chunk_table(phj_ctx *ctx, int side, const phj_join_params *p, int byte);

/* ---- test hook: poisoned workspace ----
 * Replaces nothing in the reference. From now on every device buffer the
 * context (each member of a multi-device or rank context) allocates for its
 * workspace is filled with `byte` (-1: off) before first use, as memory an
 * earlier context freed may come back. No join may read a word it did not
 * write first: the chunk tables, cursors, count pairs and exchange blocks are
 * cleared or written by the library itself, so every count stays exact. */
int phj_debug_poison_alloc(phj_ctx *ctx, int byte);

/* ---- test hook: hot-key pre-aggregation ----
 * Replaces nothing in the reference. phj_join's counting LDS join, in its
 * default schedule on one device, samples the probe side, counts its hottest
 * keys in pass 1 instead of writing them, and resolves them against the build
 * side in the build side's pass 1. `mode` sets when: 0 auto (probe sides of
 * 16.8M tuples and more, and only a table covering an eighth of the sample),
 * 1 off, 2 forced (any size, the lowest sample threshold, any coverage), -1
 * leaves the mode as it is. `stats` (may be null) receives the last phj_join's
 * {entries of the hot table, probe tuples pre-aggregated}: both 0 when that
 * join did not take the path. A multi-device or rank context never takes it. */
int phj_debug_preagg(phj_ctx *ctx, int mode, uint64_t *stats);

/* ---- test hook: a failing rank ----
 * Replaces nothing in the reference. On a multi-device or rank context, local
 * member `member` (-1: none) fails the next phj_join before the exchange. The
 * protocol must still end cleanly: with the local exchange every member returns
 * PHJ_ERR_STATE; over RCCL the failed rank sends a zeroed (valid, empty) block
 * into the all-gather and {0, 1} into the count all-reduce, so every rank
 * returns PHJ_ERR_STATE ("1 rank(s) failed") with no collective left waiting. */
int phj_debug_fail_member(phj_ctx *ctx, int member);

/* ---- test hook: the exchange block a member packed ----
 * Replaces nothing in the reference. Copies local member `member`'s exchange
 * block of the last radix phj_join (phj_exchange_layout's layout, `elems`
 * int64) to host memory, so tests can compare the library's own pack with the
 * protocol's definition. */
int phj_debug_exchange_block(phj_ctx *ctx, int member, int64_t *out, uint64_t elems);

#ifdef __cplusplus
}
#endif

#endif /* PHJ_H */
